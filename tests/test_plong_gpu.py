"""BeamPeriodSearchLong on the MI355X: xengPlong* against the restatement (tests/plong_ref.py).  The stacked spectrum A against the
float64 restatement at NT = 2^15 (the smallest), 2^16 (odd log, N1 != N2) and 2^20 (the largest; one row per work-group of the rows
pass), both products, masks, stacks of 1 and 3 and a dead series; the records word for word against the float32 banded restatement
run on the device's own A (levels, bands, a band that is empty at level 16, edges inside a tile of the sums, a NaN and an Inf
series); an integer-valued stack with planted equal maxima in different tiles and bands; bit identity across splits of a run over
calls, after Reset, across two batch sizes and beside an X-engine contraction and xengBeamformRun; two planted pulse trains in
different bands; the ABI; and Source -> BeamDedisperse -> BeamPeriodSearchLong on device rings.  The input bytes are compared
after every call (the read-only contract), the output sits between two poisoned guard bands that are checked after every call,
the state's guards at every close.  No wall-clock assertions.

The bar of the float tests.  A numpy float32 evaluation of the same contract (plong_ref.float_gap: tests/period_ref.py with dtype
float32; numpy.fft.rfft stays in single precision on float32 input) differs from the float64 restatement, on chi^2 powers with
mean / sigma = 55 and B = 64, by at most 5.6e-7 of max(1, S) at NT = 2^15 (15 series), 6.2e-7 at 2^16 (15 series) and 6.1e-7 at
2^20 (4 series).  TOL is five times the largest, 3.1e-6 (the kernel's radix-2 butterflies, table twiddles and contractions are
not numpy's algorithm), and a stack of nseg segments is held to TOL * max(1, A_ref) * nseg.  The host emulation of the kernels
(tests/test_plong_emul_cpu.py) shows 4.2e-7 at 2^15 and 9.1e-7 at 2^16 (B = 2^13).  Measured on the MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamDedisperse, BeamPeriodSearchLong, period_bands, period_candidates_long, period_sift  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.period_search import RECORD, as_records_long  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks  # noqa: E402
from tests.plong_ref import harmonic_records, plane_of, series, stacks  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
TOL = 3.1e-6
# worst |A - A_ref| / (max(1, A_ref) * nseg) over test_spectrum_within_tol_of_the_float64_restatement on the MI355X
MEASURED = "7.95e-7 at NT = 2^15, 9.05e-7 at 2^16 (B = 2^13), 9.78e-7 at 2^20"


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    n, s, k = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong()
    ffi.call("xengPlongGetInfo", ctypes.byref(n), ctypes.byref(s), ctypes.byref(k))
    return n.value, s.value, k.value


def _batch():
    a, b = ctypes.c_int(), ctypes.c_int()
    ffi.call("xengPlongGetBatch", ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


class PL:
    """The xengPlong context (one per process), an input buffer and an output plane between two poisoned guard bands."""

    def __init__(self, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kedge):
        self.npair, self.ndm, self.nwin, self.nprod, self.nt, self.nstack, self.nlevel = npair, ndm, nwin, nprod, nt, nstack, nlevel
        self.nwhite, self.kedge, self.nband = nwhite, [int(k) for k in kedge], len(kedge) - 1
        ffi.call("xengPlongInitialize", 0, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, self.nband, (ctypes.c_int * len(kedge))(*self.kedge))
        self.din = ffi.DeviceBuffer(nwin * npair * ndm * nprod * 4)
        self.nbytes = npair * ndm * nlevel * self.nband * 8
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nbytes)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        self.sent = None

    def enqueue(self, x, out=True):
        """One call; returns `completed`."""
        nc = x.shape[0]
        assert x.shape == (nc, self.npair, self.ndm, self.nprod)
        self.sent = np.ascontiguousarray(x, np.float32)
        self.din.upload(self.sent)
        done = ctypes.c_int(-1)
        ffi.call("xengPlongRun", self.din.ptr, nc, self.dout.ptr + GUARD if out else None, ctypes.byref(done))
        assert done.value in (0, 1)
        return done.value

    def result(self, completed):
        """After a sync: the input bytes are what was uploaded; the plane of a completing call (the poison is put back behind it),
        or None after having checked that a call which completed nothing left the poison in the output too; every byte before and
        after it must still be poison."""
        if self.sent is not None:
            assert self.din.download(np.uint8, self.sent.nbytes).tobytes() == self.sent.tobytes(), "the input was written"
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.nbytes:] == POISON).all(), "bytes past the output's records were written"
        if not completed:
            assert (raw[GUARD:GUARD + self.nbytes] == POISON).all(), "a call that completed no stack wrote its output"
            return None
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + self.nbytes].copy().view(RECORD).reshape(self.npair, self.ndm, self.nlevel, self.nband)

    def run(self, x):
        done = self.enqueue(x)
        ffi.call("xengPlongSync")
        return self.result(done)

    def stream(self, x, sizes):
        """Consecutive calls of the given sizes over the windows of x; the planes of the calls that completed a stack."""
        planes, n, total = [], 0, _info()[0]
        for nc in sizes:
            want = (total + nc) // (self.nt * self.nstack) > total // (self.nt * self.nstack)
            p = self.run(x[n:n + nc])
            assert (p is not None) == want
            if p is not None:
                planes.append(p)
            n += nc
            total += nc
        assert n == x.shape[0]
        return planes

    def spectrum(self, series0=0, nser=None):
        nser = self.npair * self.ndm - series0 if nser is None else nser
        A, nseg = np.empty((nser, self.nt // 2), np.float32), ctypes.c_int()
        ffi.call("xengPlongGetSpectrum", series0, nser, _fp(A), ctypes.byref(nseg))
        return (A.reshape(self.npair, self.ndm, -1) if nser == self.npair * self.ndm else A), nseg.value

    def set_mask(self, keep):
        ffi.call("xengPlongSetMask", None if keep is None else np.ascontiguousarray(keep, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengPlongCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengPlongDestroy")
        self.din.free()
        self.dout.free()


def _sizes(rng, total, nwin, fixed=None):
    out = []
    while total:
        nc = fixed if fixed else int(rng.integers(1, nwin + 1))
        out.append(min(total, nc))
        total -= out[-1]
    return out


def float_case(rng, nwindows, npair, ndm, nprod):
    """chi^2 powers with mean / sigma = 55 (2 * 55^2 degrees of freedom) times a gain in [0.5, 1.5] per series; with nprod = 4, XX
    and YY take half each (their sum has the same ratio) and the cross terms are noise."""
    gain = rng.uniform(0.5, 1.5, (npair, ndm))
    dof = 2 * 55 ** 2
    if nprod == 1:
        return (rng.chisquare(dof, (nwindows, npair, ndm)) * gain).astype(np.float32)[..., None]
    x = rng.standard_normal((nwindows, npair, ndm, 4)) * 100
    x[..., 0] = rng.chisquare(dof // 2, (nwindows, npair, ndm)) * gain
    x[..., 1] = rng.chisquare(dof // 2, (nwindows, npair, ndm)) * gain
    return x.astype(np.float32)


def check_records(pl, plane, A):
    """The plane of a completed stack equals, bit for bit, the float32 banded restatement run on the device's own A."""
    exp = plane_of(harmonic_records(A, pl.nlevel, pl.kedge))
    assert plane.tobytes() == exp.tobytes(), "records differ from the restatement on the device's A: %r" % (
        np.argwhere((plane['k'] != exp['k']) | (plane['H'].view(np.uint32) != exp['H'].view(np.uint32)))[:5],)


# ---------------------------------------------------------------- 1. the spectrum against float64
def edge_mask(n, B):
    keep = np.ones(n, np.uint8)
    keep[3 * B - 3:3 * B + 2] = 0               # a run that crosses the edge between blocks 2 and 3
    return keep


def block_mask(n, B):
    keep = np.ones(n, np.uint8)
    keep[B:2 * B] = 0                           # the whole of block 1
    return keep


SPECTRUM_CASES = {
    # nt: (npair, ndm, nprod, nstack, nwhite, masks, nwin)
    1 << 15: (3, 5, 1, 3, 64, (edge_mask, block_mask), (1 << 14) + 5),
    1 << 16: (3, 5, 4, 1, 1 << 13, (block_mask,), (1 << 15) + 5),
    1 << 20: (1, 2, 1, 1, 64, (edge_mask,), 1 << 18),
}


@pytest.mark.parametrize("nt", sorted(SPECTRUM_CASES))
def test_spectrum_within_tol_of_the_float64_restatement(nt):
    """3 pairs x 5 trials (not a multiple of the ingest tile; 2 series at 2^20), chi^2 powers with mean / sigma = 55, one dead
    series: the three splits of N -- 2^7 x 2^7, 2^7 x 2^8 and 2^9 x 2^10, with four, two and one row per work-group of the rows pass
    (the split's rule, min(LN div 2, 9), gives LN div 2 at every size) -- and between them both products, stacks of 1 and 3,
    B = 64 and 2^13, a mask that zaps a run across a block edge and one that zaps a whole block.  After every completed segment A
    is read back and held to TOL * max(1, A_ref) * nseg against the float64 restatement; bin 0 reads +0, zapped bins and the dead
    series exactly nseg.  A completed stack's plane (5 levels, 7 bands) equals the float32 restatement of the device's A."""
    npair, ndm, nprod, nstack, nwhite, masks, nwin = SPECTRUM_CASES[nt]
    nlevel, kedge = 5, period_bands(nt, 7, 2)
    nsegs = nstack + 1 if nt < 1 << 20 else 1
    rng = np.random.default_rng(nt)
    x = float_case(rng, nsegs * nt, npair, ndm, nprod)
    x[:, 0, 1, :] = 0.0
    keep = np.ones(nt // 2, np.uint8)
    for m in masks:
        keep &= m(nt // 2, nwhite)
    ref = stacks(series(x, np.float64).reshape(x.shape[0], -1), nt, nstack, nwhite, keep, np.float64)
    pl = PL(npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kedge)
    pl.set_mask(keep)
    worst, n, seg = 0.0, 0, 0
    for nc in _sizes(rng, x.shape[0], nwin, nwin if nt == 1 << 20 else None):
        plane = pl.run(x[n:n + nc])
        n += nc
        if n // nt == seg:
            continue
        A_ref, nseg_ref = ref[seg]
        seg += 1
        A, nseg = pl.spectrum()
        assert nseg == nseg_ref and _info() == (n, seg % nstack, seg // nstack)
        A_ref = A_ref.reshape(A.shape)
        err = np.abs(A - A_ref) / (np.maximum(1.0, A_ref) * nseg)
        worst = max(worst, float(err.max()))
        print("plong spectrum nt=%d segment %d: worst |A - A_ref| / (max(1, A_ref) nseg) = %.3g (TOL %.3g)" % (nt, seg, err.max(), TOL))
        assert (err <= TOL).all(), "nt=%d segment %d: worst |A - A_ref| / (max(1, A_ref) nseg) = %.3g, TOL %.3g" % (nt, seg, err.max(), TOL)
        assert (A[..., 0] == 0).all() and not np.signbit(A[..., 0]).any()
        assert (A[..., keep == 0][..., 1:] == nseg).all() and (A[0, 1, 1:] == nseg).all()
        assert (plane is not None) == (nseg == nstack)
        if plane is not None:
            check_records(pl, plane, A)
    assert seg == nsegs
    pl.close()
    print("plong spectrum nt=%d nprod=%d nstack=%d B=%d: worst |A - A_ref| / (max(1, A_ref) nseg) = %.3g (TOL %.3g)" % (nt, nprod, nstack, nwhite, worst, TOL))


# ---------------------------------------------------------------- 2. the records word for word
NT = 1 << 15
BANDS = {1: [31, NT // 2], 7: [3, 700, 1500, 2000, 5000, 9000, 12000, NT // 2], 32: period_bands(NT, 32, 2)}


@pytest.fixture(scope="module")
def record_case():
    npair, ndm = 2, 5
    clean = float_case(np.random.default_rng(100), NT, npair, ndm, 1)
    x = clean.copy()
    x[300, 0, 1, 0] = np.nan
    x[NT - 17, 1, 3, 0] = np.inf
    return clean, x


@pytest.mark.parametrize("nlevel,nband", [(1, 1), (1, 7), (5, 1), (5, 7), (5, 32), (1, 32)])
def test_records_equal_the_restatement_on_the_devices_spectrum(record_case, nlevel, nband):
    """NT = 2^15, nlevel 1 and 5, 1, 7 and 32 bands.  The 7 edges 700 and 1500 fall inside tiles of the sums (1024 bins) at every
    level, and the bands from 1500 up are empty at level 16 (16 * 1500 > N), those from 5000 up from level 4 on; the 32 log-spaced
    bands begin one bin wide.  Series
    (0, 1) holds a NaN and (1, 3) an Inf: both read {+0, -1} everywhere, and every other series -- A and records -- is bit for bit
    what it is in a run without the defects."""
    npair, ndm, nwhite, kedge = 2, 5, 64, BANDS[nband]
    clean, x = record_case
    pl = PL(npair, ndm, 8192, 1, NT, 1, nlevel, nwhite, kedge)
    good, = pl.stream(clean, [8192] * 4)
    A_good, nseg = pl.spectrum()
    assert nseg == 1
    check_records(pl, good, A_good)
    N = NT // 2
    for lv in range(nlevel):
        for b in range(nband):
            lo, hi = kedge[b] << lv, min(kedge[b + 1] << lv, N)
            if lo < hi:
                assert (good['k'][:, :, lv, b] >= lo).all() and (good['k'][:, :, lv, b] < hi).all() and (good['H'][:, :, lv, b] > 0).all()
            else:
                assert (good['k'][:, :, lv, b] == -1).all() and (good['H'][:, :, lv, b] == 0).all() and not np.signbit(good['H'][:, :, lv, b]).any()
    bad, = pl.stream(x, [8192] * 4)
    A_bad, _ = pl.spectrum()
    check_records(pl, bad, A_bad)
    part, _ = pl.spectrum(3, 2)                 # (a range of the series)
    assert part.tobytes() == A_bad.reshape(-1, N)[3:5].tobytes()
    pl.close()
    others = np.ones((npair, ndm), bool)
    others[0, 1] = others[1, 3] = False
    assert good[others].tobytes() == bad[others].tobytes() and A_good[others].tobytes() == A_bad[others].tobytes()
    none = np.array([(0.0, -1)] * (nlevel * nband), RECORD).tobytes()
    for s in ((0, 1), (1, 3)):
        assert bad[s].tobytes() == none and np.isnan(A_bad[s][1:]).all() and A_bad[s][0] == 0


def test_integer_valued_stack_with_planted_equal_maxima():
    """NT = 2^15, a stack of 3, B = 8, every bin zapped but 40, 41, 104, 105, 3000, 3001, 9000 and 9001; each series is a constant
    plus four tones of equal amplitude at 40, 104, 3000 and 9000.  A zapped bin reads 1.0 per segment, and in a tone's block the
    tone's bin holds all the power that counts, so S = P / (P / 2) = 2.0: A is 3.0 everywhere, 6.0 at the tones, a tiny number
    beside them -- every harmonic sum is exact and equal maxima abound.  Bands [1, 64), [64, 2000), [2000, N): 40 and 104 tie in
    one tile of the sums but in different bands, 3000 and 9000 in one band but in tiles 2 and 8: the smallest k wins, exactly."""
    npair, ndm, nt, nstack, nlevel = 2, 5, NT, 3, 5
    kedge = [1, 64, 2000, nt // 2]
    n = np.arange(nstack * nt)
    amp = np.arange(1, npair * ndm + 1).reshape(npair, ndm) * 8.0
    tone = sum(np.cos(2 * np.pi * k * n / nt) for k in (40, 104, 3000, 9000))
    x = (100.0 + amp[None] * tone[:, None, None]).astype(np.float32)[..., None]
    keep = np.zeros(nt // 2, np.uint8)
    keep[[40, 41, 104, 105, 3000, 3001, 9000, 9001]] = 1
    pl = PL(npair, ndm, 8192, 1, nt, nstack, nlevel, 8, kedge)
    pl.set_mask(keep)
    plane, = pl.stream(x, [8192] * (nstack * nt // 8192))
    A, nseg = pl.spectrum()
    pl.close()
    assert nseg == 3 and (A[..., keep == 0][..., 1:] == 3.0).all() and (A[..., 0] == 0).all()
    assert (A[..., [40, 104, 3000, 9000]] == 6.0).all() and (A[..., [41, 105, 3001, 9001]] < 1e-6).all()
    check_records(pl, plane, A)
    assert (plane['H'][..., 0, :] == 6.0).all() and (plane['k'][..., 0, :] == [40, 104, 3000]).all()
    # level 1: A[(k + 1) div 2] + A[k] = 3 + 6, first reached at k = 40 (band 0), at k = 2 * 40 - 1 = 79 ... but 79 < 128 is band 0 too:
    # band 1 begins at 128 and first holds 9.0 at 2 * 104 - 1 = 207; band 2 begins at 4000 and first holds it at 2 * 3000 - 1
    assert (plane['H'][..., 1, :] == 9.0).all() and (plane['k'][..., 1, :] == [40, 207, 5999]).all()


# ---------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("nprod", [1, 4])
def test_bit_identical_across_splits_reset_batches_and_concurrent_kernels(nprod):
    """2 NT + 17 windows at NT = 2^15, a stack of 2, 3 x 5 series: even calls, a run with stretches of single windows on either
    side of the first segment boundary and a call that ends on the segment's last window, and a random split; each run follows a
    Reset (the second one after 5000 windows of another series' partial segment, which must leave no trace), the third runs in
    batches of 4 series instead of 15, and all give the same A and the same plane bit for bit; so does a fresh context run while
    X-engine contractions and xengBeamformRun are in flight."""
    npair, ndm, nwin, nt, nstack, nlevel, nwhite = 3, 5, 8192, NT, 2, 5, 64
    kedge = period_bands(nt, 7, 2)
    total = 2 * nt + 17
    rng = np.random.default_rng(7 + nprod)
    x = float_case(rng, total, npair, ndm, nprod)
    ones = [8192] * 3 + [8192 - 20] + [1] * 20 + [1] * 20 + [8192 - 20]      # ... the 20th single window is the segment's last
    ones += _sizes(None, total - sum(ones), nwin, nwin)
    splits = [_sizes(None, total, nwin, nwin), ones, _sizes(rng, total, nwin), _sizes(None, total, 5000, 5000)]
    ends = [np.cumsum(s) for s in splits]
    assert any(nt in e for e in ends) and nt in ends[1] and nt + 1 in ends[1]
    assert any(((e - np.array(s) < nt) & (e > nt + 1)).any() for s, e in zip(splits, ends))   # and inside a call
    pl = PL(npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kedge)
    assert _batch() == (15, 15)
    outs = []
    for i, sizes in enumerate(splits):
        if i == 1:
            assert pl.stream(100 + x[:5000][::-1], [5000]) == []
        ffi.call("xengPlongSetBatch", 4 if i == 2 else 0)
        assert _batch() == ((4, 15) if i == 2 else (15, 15))
        ffi.call("xengPlongReset")
        assert _info() == (0, 0, 0)
        plane, = pl.stream(x, sizes)
        A, nseg = pl.spectrum()
        assert nseg == nstack and _info() == (total, 0, 1)
        outs.append((plane.tobytes(), A.tobytes()))
    check_records(pl, plane, A)
    with pytest.raises(ffi.XengError):
        ffi.call("xengPlongSetBatch", 16)
    pl.close()
    # a fresh context beside other work: contractions on their own stream, the beamformer on this one
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    pl = PL(npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kedge)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        planes, n = [], 0
        for nc in splits[0]:
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            done = pl.enqueue(x[n:n + nc])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengPlongSync")
            p = pl.result(done)
            if p is not None:
                planes.append(p)
            n += nc
        ffi.call("xengXgpuSync")
        (plane,), (A, _) = planes, pl.spectrum()
        outs.append((plane.tobytes(), A.tobytes()))
    finally:
        xg.close()
    pl.close()
    ffi.call("xengBeamformDestroy")
    for o in outs[1:]:
        assert o[0] == outs[0][0] and o[1] == outs[0][1]
    assert (np.frombuffer(outs[0][0], RECORD)['k'].reshape(npair, ndm, nlevel, 7)[:, :, 0] >= 2).all()      # (every band holds bins at level 1)


# ---------------------------------------------------------------- 4. planted sources
PLANT = dict(nt=NT, npair=2, ndm=3, kedge=[2, 600, 1300, 1600, 2000, NT // 2], strong=(27, 26), weak=(23, 12), where=(1, 2), threshold=6.0)


def planted_case():
    """NT = 2^15, integer noise 0..49, and in series (1, 2) two trains of one-window pulses: one of 26 every 27 windows -- a fundamental
    of NT / 27 = 1213.63 bins, 13 lines below Nyquist of a whitened power near 150 each -- and a weaker one of 12 every 23 windows,
    NT / 23 = 1424.70 bins, 11 lines near 40.  27 / 23 is no ratio of integers up to 16.  The bands put them into [600, 1300) and
    [1300, 1600)."""
    c = PLANT
    rng = np.random.default_rng(77)
    x = rng.integers(0, 50, (c['nt'], c['npair'], c['ndm'], 1)).astype(np.float32)
    for period, amp in (c['strong'], c['weak']):
        x[5::period, c['where'][0], c['where'][1], 0] += amp
    return x


def check_planted(plane, one_band_plane):
    """The sifted candidates of a banded plane are the two trains and nothing else, the stronger first; one record per level, the
    same A searched as one band, finds the stronger only."""
    c = PLANT
    nt, dms = c['nt'], np.arange(c['ndm']) * 0.5
    cands = period_sift(period_candidates_long(plane, c['threshold'], dms, nt, 1, 1e-3, c['kedge']), nt)
    assert {(x['pair'], x['idm']) for x in cands} == {c['where']}, cands
    assert len(cands) == 2, [(x['k'], x['h'], x['band'], x['log10_pfa']) for x in cands]
    s, w = cands
    assert abs(s['k'] / s['h'] - nt / 27) <= 0.5 and s['band'] == 1 and s['harmonics'] and -s['log10_pfa'] > 100
    assert abs(w['k'] / w['h'] - nt / 23) <= 0.5 and w['band'] == 2 and w['log10_pfa'] > s['log10_pfa'] and -w['log10_pfa'] >= c['threshold']
    assert abs(s['period'] - 27e-3) < 1e-5 and abs(w['period'] - 23e-3) < 1e-5 and s['dm'] == w['dm'] == 1.0
    one = period_sift(period_candidates_long(one_band_plane, c['threshold'], dms, nt, 1, 1e-3, [2, nt // 2]), nt)
    assert one and all(abs(x['k'] / x['h'] - nt / 23) > 0.5 for x in one)      # (the case one record per level misses)
    return cands


def test_two_planted_pulse_trains_in_different_bands_are_the_only_sifted_candidates():
    c = PLANT
    x = planted_case()
    (A32, _), = stacks(series(x, np.float32).reshape(c['nt'], -1), c['nt'], 1, 64, None, np.float32)
    A32 = A32.reshape(c['npair'], c['ndm'], -1)
    ref = check_planted(plane_of(harmonic_records(A32, 5, c['kedge'])), plane_of(harmonic_records(A32, 5, [2, c['nt'] // 2])))
    pl = PL(c['npair'], c['ndm'], 8192, 1, c['nt'], 1, 5, 64, c['kedge'])
    plane, = pl.stream(x, [8192] * 4)
    A, _ = pl.spectrum()
    check_records(pl, plane, A)
    pl.close()
    got = check_planted(plane, plane_of(harmonic_records(A, 5, [2, c['nt'] // 2])))
    assert [(g['k'], g['h'], g['band']) for g in got] == [(r['k'], r['h'], r['band']) for r in ref]


# ---------------------------------------------------------------- 5. the ABI
def test_completing_call_tickets_and_argument_checks():
    """NT = 2^15, a stack of 2, calls of 8192 windows: `completed` is 1 on the call that brings window 2 NT and 0 on every other,
    whose output (NULL or not) is untouched.  The completing call with out_dev NULL is INVALID_ARGUMENT and enqueues nothing: the
    counts stand, and the same call with an output then gives the plane of an undisturbed run.  Tickets count from 1; unknown
    tickets and null pointers are errors; every INVALID_ARGUMENT of Initialize leaves a live context alone; Run refuses nwin_call
    outside 1..nwin and misaligned or null pointers with the count unchanged; GetSpectrum a range outside the series; after
    Destroy every call that needs a context is INVALID_STATE.  The backend's plong_* calls."""
    npair, ndm, nt, nstack, nlevel, kedge = 2, 5, NT, 2, 2, [2, 300, NT // 2]
    rng = np.random.default_rng(3)
    x = float_case(rng, 2 * nt, npair, ndm, 1)
    pl = PL(npair, ndm, 8192, 1, nt, nstack, nlevel, 64, kedge)
    with pytest.raises(ffi.XengError) as ei:
        pl.spectrum()
    assert ei.value.status == INVALID_STATE                     # (no segment is complete yet)
    t, done = ctypes.c_ulonglong(), ctypes.c_int(-1)
    for k in range(7):
        assert pl.enqueue(x[8192 * k:8192 * k + 8192], out=k % 2 == 0) == 0
        ffi.call("xengPlongMark", ctypes.byref(t))
        assert t.value == k + 1
        ffi.call("xengPlongTicketDone", t.value, ctypes.byref(done))
        assert done.value in (0, 1)
        ffi.call("xengPlongWait", t.value)
        ffi.call("xengPlongTicketDone", t.value, ctypes.byref(done))
        assert done.value == 1 and pl.result(0) is None
    assert _info() == (7 * 8192, 1, 0) and pl.spectrum()[1] == 1
    with pytest.raises(ffi.XengError) as ei:
        pl.enqueue(x[7 * 8192:], out=False)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (7 * 8192, 1, 0)
    ffi.call("xengPlongSync")
    assert pl.result(0) is None
    plane = pl.run(x[7 * 8192:])
    assert plane is not None and _info() == (2 * nt, 0, 1)
    A, nseg = pl.spectrum()
    assert nseg == 2
    check_records(pl, plane, A)
    for bad in (0, 8):
        with pytest.raises(ffi.XengError):
            ffi.call("xengPlongTicketDone", bad, ctypes.byref(done))
        with pytest.raises(ffi.XengError):
            ffi.call("xengPlongWait", bad)
    from caltech_bifrost_dsp_amd.backend import HipBackend
    be = HipBackend()
    tk = be.plong_mark()
    assert tk == 8
    be.plong_wait(tk)
    be.plong_wait(tk)                   # already complete: answered by the query
    assert be.plong_ticket_done(tk) and be.plong_info() == (2 * nt, 0, 1) and be.plong_guards_intact()
    A2, nseg = be.plong_spectrum(0, npair * ndm, nt)
    assert nseg == 2 and A2.tobytes() == A.tobytes()
    assert be.plong_set_mask(np.ones(nt // 2, np.uint8)) == 0 and be.plong_set_mask(None) == 0
    be.plong_reset()
    assert be.plong_info() == (0, 0, 0)
    again, = pl.stream(x, [8192] * 8)
    assert again.tobytes() == plane.tobytes()
    # arguments, with the context
    edges = (ctypes.c_int * 3)(*kedge)
    good = [0, npair, ndm, 8192, 1, nt, nstack, nlevel, 64, 2, edges]
    for i, v in ((1, 0), (3, nt + 1), (4, 2), (5, 1 << 14), (5, 1 << 21), (6, 0), (7, 6), (8, 4), (8, 1 << 14), (9, 0), (9, 33), (10, None),
                 (10, (ctypes.c_int * 3)(2, 2, 9)), (10, (ctypes.c_int * 3)(1 << 10, 2000, 3000)), (10, (ctypes.c_int * 3)(2, 300, nt // 2 + 1))):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPlongInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, (i, v)
    assert _info() == (2 * nt, 0, 1)            # (the context is still there)
    comp = ctypes.c_int(-1)
    for args in ((pl.din.ptr, 0, pl.dout.ptr), (pl.din.ptr, 8193, pl.dout.ptr), (pl.din.ptr + 4, 1, pl.dout.ptr), (pl.din.ptr, 1, pl.dout.ptr + 8),
                 (None, 1, pl.dout.ptr)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPlongRun", *args, ctypes.byref(comp))
        assert ei.value.status == INVALID_ARGUMENT and _info() == (2 * nt, 0, 1)
    f, s, n = np.zeros(nt, np.float32), ctypes.c_int(), ctypes.c_longlong()
    for s0, ns in ((-1, 1), (0, 0), (0, 11), (10, 1), (9, 2)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPlongGetSpectrum", s0, ns, _fp(f), ctypes.byref(s))
        assert ei.value.status == INVALID_ARGUMENT
    din, dout = pl.din.ptr, pl.dout.ptr
    pl.close()
    for name, args in (("xengPlongRun", (din, 1, dout, ctypes.byref(s))), ("xengPlongReset", ()), ("xengPlongSetMask", (None,)), ("xengPlongSetBatch", (1,)),
                       ("xengPlongGetInfo", (ctypes.byref(n), ctypes.byref(s), ctypes.byref(n))), ("xengPlongGetSpectrum", (0, 1, _fp(f), ctypes.byref(s))),
                       ("xengPlongMark", (ctypes.byref(t),)), ("xengPlongWait", (1,)), ("xengPlongTicketDone", (1, ctypes.byref(s))),
                       ("xengPlongSync", ()), ("xengPlongCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name


# ---------------------------------------------------------------- 6. the chain on device rings
def chain_case():
    """Dual-pol power beams [nwindows][2 pairs][2 x 8 fine channels][4] of values 0..49 with a pulse of 8 per channel in XX of pair
    1 every 27 windows, dispersed at trial 5 of 8; the header UpchanSumBeams writes.  Spans of 2048 windows; the dedisperser's
    latency S makes the search skip span 0."""
    from tests.test_dedisp_cpu import header_table, power_header
    nchan, npair, N, W, nwin, nt, d0 = 2, 2, 8, 4, 2048, NT, 5
    nfine = nchan * N
    dms = [float(d) for d in np.linspace(0.0, 0.14, 8)]
    hdr = power_header(nchan, npair, N, W, seq0=4096)
    table, tsamp = header_table(hdr, nfine, dms)
    S = int(table.max())
    nspan = -(-S // nwin) + nt // nwin + 1
    rng = np.random.default_rng(99)
    x = rng.integers(0, 50, (nspan * nwin, npair, nfine, 4)).astype(np.float32)
    for t in range(2, nspan * nwin - S, 27):
        x[t + table[d0], 1, np.arange(nfine), 0] += 8
    return dict(nchan=nchan, npair=npair, N=N, W=W, nwin=nwin, nt=nt, nspan=nspan, d0=d0, nfine=nfine, dms=dms, hdr=hdr, S=S, tsamp=tsamp, x=x)


def test_chain_source_dedisperse_period_search_long_on_device_rings():
    """Source -> BeamDedisperse -> BeamPeriodSearchLong: on_candidates receives one sifted candidate, the planted pair, the planted
    DM's trial and the planted period of 27 windows, with its harmonics absorbed; the one plane of the output ring equals a
    direct run of xengPlongRun on the spans BeamDedisperse wrote, bit for bit, and its sequence begins at the first span past the
    dedisperser's partial sums; the header carries the bands."""
    c = chain_case()
    npair, nwin, nt, ndm, nlevel = c['npair'], c['nwin'], c['nt'], len(c['dms']), 4
    kedge = [2, 600, 1300, 2000, nt // 2]
    r0, r1, r2 = Ring("ub-output", space="cuda"), Ring("dd-output", space="cuda"), Ring("pl-output", space="cuda_host")
    got = []
    dd = BeamDedisperse(LOG, r0, r1, npair=npair, nchan=c['nchan'], nupchan=c['N'], nwin=nwin, dms=c['dms'], gpu=0)
    pr = BeamPeriodSearchLong(LOG, r1, r2, npair=npair, ndm=ndm, nwin=nwin, nt=nt, nstack=1, nlevel=nlevel, nwhite=64, kedge=kedge, threshold=6.0,
                              on_candidates=got.extend, gpu=0)
    mid, sink = Sink(r1, nwin * npair * ndm * 4), Sink(r2, npair * ndm * nlevel * 4 * 8)
    run_blocks([dd, pr], Source(r0, [(c['hdr'], c['x'], nwin * npair * c['nfine'] * 16)]), [mid, sink])
    (dh, _, dspans), = mid.sequences
    (hd, tag, planes), = sink.sequences
    acc_len = c['W'] * c['N']
    skipped = -(-c['S'] // nwin)
    assert dh['dedisp_latency'] == c['S'] and skipped == 1 and len(dspans) == c['nspan'] and len(planes) == 1
    assert tag == hd['seq0'] == 4096 + skipped * nwin * acc_len
    assert (hd['nt'], hd['nstack'], hd['nlevel'], hd['nwhite'], hd['kmin'], hd['nband'], hd['kedge'], hd['dedisp_latency']) == (
        nt, 1, nlevel, 64, 2, 4, kedge, c['S'])
    best = [g for g in got if g['pair'] == 1]
    assert best and {g['pair'] for g in got} == {1}, got
    top = min(best, key=lambda g: g['log10_pfa'])
    assert abs(top['k'] / top['h'] - nt / 27) <= 0.5 and top['band'] == 1 and top['harmonics'] and top['sigma'] > 6
    assert abs(top['period'] - 27 * c['tsamp']) < 1e-3 * top['period'] and abs(top['idm'] - c['d0']) <= 1
    assert pr.stats['ncand'] == len(got) and pr.stats['nstartup'] == skipped and pr.stats['nwindow'] == (c['nspan'] - skipped) * nwin
    assert pr.stats['nstack_done'] == 1 and pr.stats['ndropped'] == 0
    direct = PL(npair, ndm, nwin, 1, nt, 1, nlevel, 64, kedge)
    out = direct.stream(np.concatenate([sp.view(np.float32).reshape(nwin, npair, ndm, 1) for sp in dspans[skipped:]]), [nwin] * (c['nspan'] - skipped))
    direct.close()
    assert len(out) == 1 and out[0].tobytes() == planes[0].tobytes()
    assert (as_records_long(planes[0], npair, ndm, nlevel, 4)['k'][:, :, 0] >= 2).all()
