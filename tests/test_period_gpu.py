"""BeamPeriodSearch on the MI355X: xengPeriod* against the restatement (tests/period_ref.py).  The stacked spectrum A against the
float64 restatement at every segment length, both products, masks, stacks of 1 and 3 and a dead series; the records word for
word against the float32 harmonic-sum restatement run on the device's own A (levels, kmin, a NaN series, an integer-valued stack
with planted equal maxima); bit identity across splits of a run over calls, after Reset against a fresh context and beside an
X-engine contraction and xengBeamformRun; a planted pulse train; the ABI (a completing call without an output, `completed`,
tickets, calls without a context); and Source -> BeamDedisperse -> BeamPeriodSearch on device rings.  The output sits between two
poisoned guard bands that are checked after every call, the state's guards at every close.  No wall-clock assertions.

The bar of the float tests.  A numpy float32 evaluation of the same contract (tests/period_ref.py with dtype float32; numpy.fft.rfft
stays in single precision on float32 input) differs from the float64 restatement, at NT = 2^14, 64 series of chi^2 powers with
mean / sigma = 55, by at most 2.9e-6 of max(1, S) (B = NT/2; 3.1e-7 at B = 8, 6.1e-7 at B = 64; rms 9.0e-7).  TOL is five times
that, 1.45e-5, and a stack of nseg segments is held to TOL * max(1, A_ref) * nseg.  Measured on the MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamDedisperse, BeamPeriodSearch, period_candidates  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.period_search import RECORD, as_records  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.period_ref import harmonic_records, series, stacks  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
TOL = 1.45e-5
# worst |A - A_ref| / (max(1, A_ref) * nseg) over test_spectrum_within_tol_of_the_float64_restatement on the MI355X
MEASURED = "not measured"


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    n, s, k = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong()
    ffi.call("xengPeriodGetInfo", ctypes.byref(n), ctypes.byref(s), ctypes.byref(k))
    return n.value, s.value, k.value


class PR:
    """The xengPeriod context (one per process), an input buffer and an output plane between two poisoned guard bands."""

    def __init__(self, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin):
        self.npair, self.ndm, self.nwin, self.nprod, self.nt, self.nstack, self.nlevel = npair, ndm, nwin, nprod, nt, nstack, nlevel
        self.nwhite, self.kmin = nwhite, kmin
        ffi.call("xengPeriodInitialize", 0, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin)
        self.din = ffi.DeviceBuffer(nwin * npair * ndm * nprod * 4)
        self.nbytes = npair * ndm * nlevel * 8
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nbytes)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def enqueue(self, x, out=True):
        """One call; returns `completed`."""
        nc = x.shape[0]
        assert x.shape == (nc, self.npair, self.ndm, self.nprod)
        self.din.upload(np.ascontiguousarray(x, np.float32))
        done = ctypes.c_int(-1)
        ffi.call("xengPeriodRun", self.din.ptr, nc, self.dout.ptr + GUARD if out else None, ctypes.byref(done))
        assert done.value in (0, 1)
        return done.value

    def result(self, completed):
        """After a sync: the plane of a completing call (the poison is put back behind it), or None after having checked that a
        call which completed nothing left the poison in the output too; every byte before and after it must still be poison."""
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.nbytes:] == POISON).all(), "bytes past the output's records were written"
        if not completed:
            assert (raw[GUARD:GUARD + self.nbytes] == POISON).all(), "a call that completed no stack wrote its output"
            return None
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + self.nbytes].copy().view(RECORD).reshape(self.npair, self.ndm, self.nlevel)

    def run(self, x):
        done = self.enqueue(x)
        ffi.call("xengPeriodSync")
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

    def spectrum(self):
        A, nseg = np.empty((self.npair, self.ndm, self.nt // 2), np.float32), ctypes.c_int()
        ffi.call("xengPeriodGetSpectrum", _fp(A), ctypes.byref(nseg))
        return A, nseg.value

    def set_mask(self, keep):
        ffi.call("xengPeriodSetMask", None if keep is None else np.ascontiguousarray(keep, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengPeriodCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengPeriodDestroy")
        self.din.free()
        self.dout.free()


def plane_of(rec):
    out = np.zeros(rec['k'].shape, RECORD)
    out['H'], out['k'] = rec['H'], rec['k']
    return out


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


def check_records(pr, plane, A):
    """The plane of a completed stack equals, bit for bit, the float32 harmonic-sum restatement run on the device's own A."""
    exp = plane_of(harmonic_records(A, pr.nlevel, pr.kmin))
    assert plane.tobytes() == exp.tobytes(), "records differ from the restatement on the device's A: %r" % (
        np.argwhere((plane['k'] != exp['k']) | (plane['H'].view(np.uint32) != exp['H'].view(np.uint32)))[:5],)


# ---------------------------------------------------------------- 1. the spectrum against float64
def edge_mask(n, B):
    keep = np.ones(n, np.uint8)
    keep[3 * B - 3:3 * B + 2] = 0               # a run that crosses the edge between blocks 2 and 3
    return keep


def block_mask(n, B):
    keep = np.ones(n, np.uint8)
    if B < n:
        keep[B:2 * B] = 0                       # the whole of block 1
    else:
        keep[n // 4:n // 2] = 0
    return keep


SPECTRUM_CASES = {
    # nt: (nprod, nstack, nwhite or None for nt/2, masks)
    1 << 8: (1, 3, 8, (edge_mask,)),
    1 << 9: (4, 1, 64, (block_mask,)),
    1 << 10: (1, 3, None, ()),
    1 << 11: (4, 3, 8, (edge_mask, block_mask)),
    1 << 12: (1, 1, 64, (edge_mask,)),
    1 << 13: (4, 1, None, (block_mask,)),
    1 << 14: (1, 3, 64, (edge_mask, block_mask)),
}


@pytest.mark.parametrize("nt", sorted(SPECTRUM_CASES))
def test_spectrum_within_tol_of_the_float64_restatement(nt):
    """2 pairs x 5 trials (the series fill nothing evenly), chi^2 powers with mean / sigma = 55, one dead series; every segment
    length once -- both parities of log2(NT/2) -- and between them both products, stacks of 1 and 3, B = 8, 64 and NT/2, a mask
    that zaps a run across a block edge and one that zaps a whole block.  After every completed segment A is read back and held
    to TOL * max(1, A_ref) * nseg against the float64 restatement; bin 0 reads +0, zapped bins and the dead series exactly nseg.
    A completed stack's plane equals the float32 harmonic restatement of the device's A."""
    nprod, nstack, nwhite, masks = SPECTRUM_CASES[nt]
    nwhite = nwhite or nt // 2
    npair, ndm, nlevel, kmin = 2, 5, 3, 2
    nwin = nt // 2 + 5
    nsegs = nstack + 1
    rng = np.random.default_rng(nt)
    x = float_case(rng, nsegs * nt, npair, ndm, nprod)
    x[:, 1, 2, :] = 0.0
    keep = np.ones(nt // 2, np.uint8)
    for m in masks:
        keep &= m(nt // 2, nwhite)
    ref = stacks(series(x, np.float64).reshape(x.shape[0], -1), nt, nstack, nwhite, keep, np.float64)
    pr = PR(npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin)
    if masks:
        pr.set_mask(keep)
    worst, n, seg = 0.0, 0, 0
    for nc in _sizes(rng, x.shape[0], nwin):
        plane = pr.run(x[n:n + nc])
        n += nc
        if n // nt == seg:
            continue
        A_ref, nseg_ref = ref[seg]
        seg += 1
        A, nseg = pr.spectrum()
        assert nseg == nseg_ref and _info() == (n, seg % nstack, seg // nstack)
        A_ref = A_ref.reshape(A.shape)
        err = np.abs(A - A_ref) / (np.maximum(1.0, A_ref) * nseg)
        worst = max(worst, float(err.max()))
        assert (err <= TOL).all(), "nt=%d segment %d: worst |A - A_ref| / (max(1, A_ref) nseg) = %.3g, TOL %.3g" % (nt, seg, err.max(), TOL)
        assert (A[..., 0] == 0).all() and not np.signbit(A[..., 0]).any()
        assert (A[..., keep == 0] == nseg).all() and (A[1, 2, 1:] == nseg).all()
        assert (plane is not None) == (nseg == nstack)
        if plane is not None:
            check_records(pr, plane, A)
    assert seg == nsegs
    pr.close()
    print("period spectrum nt=%d nprod=%d nstack=%d B=%d: worst |A - A_ref| / (max(1, A_ref) nseg) = %.3g (TOL %.3g)" % (nt, nprod, nstack, nwhite, worst, TOL))


# ---------------------------------------------------------------- 2. the records word for word
@pytest.mark.parametrize("nlevel,kmin", [(1, 1), (3, 31), (5, 1), (5, 31)])
def test_records_equal_the_restatement_on_the_devices_spectrum(nlevel, kmin):
    """NT = 1024, stacks of 2: nlevel 1, 3 and 5, kmin 1 and its maximum NT/32 - 1.  Series (0, 1) holds a NaN in the stack's first
    segment and (1, 3) an Inf in its second: both read {+0, -1} at every level (A is NaN from that segment on), and every other
    series -- A and records -- is bit for bit what it is in a run without the defects."""
    npair, ndm, nt, nstack, nwhite = 2, 5, 1024, 2, 64
    rng = np.random.default_rng(100 * nlevel + kmin)
    clean = float_case(rng, nstack * nt, npair, ndm, 1)
    x = clean.copy()
    x[300, 0, 1, 0] = np.nan
    x[nt + 17, 1, 3, 0] = np.inf
    pr = PR(npair, ndm, 100, 1, nt, nstack, nlevel, kmin=kmin, nwhite=nwhite)
    sizes = _sizes(rng, nstack * nt, 100, 100)
    good, = pr.stream(clean, sizes)
    A_good, nseg = pr.spectrum()
    assert nseg == nstack
    check_records(pr, good, A_good)
    assert (good['k'] >= kmin << np.arange(nlevel)).all() and (good['k'] < nt // 2).all() and (good['H'] > 0).all()
    bad, = pr.stream(x, sizes)
    A_bad, _ = pr.spectrum()
    check_records(pr, bad, A_bad)
    pr.close()
    others = np.ones((npair, ndm), bool)
    others[0, 1] = others[1, 3] = False
    assert good[others].tobytes() == bad[others].tobytes() and A_good[others].tobytes() == A_bad[others].tobytes()
    none = np.array([(0.0, -1)] * nlevel, RECORD).tobytes()
    for s in ((0, 1), (1, 3)):
        assert bad[s].tobytes() == none and np.isnan(A_bad[s][1:]).all() and A_bad[s][0] == 0


def test_integer_valued_stack_with_planted_equal_maxima():
    """NT = 512, a stack of 3, B = 8, every bin zapped but 40, 41, 104 and 105; each series is a constant plus two tones of equal
    amplitude at bins 40 and 104.  A zapped bin reads 1.0 per segment, and in the blocks of 40 and of 104 the tone's bin holds
    all the power that counts (its neighbour's is rounding noise, 1e-13 of it), so S = P / (P / 2) = 2.0: A is 3.0 everywhere,
    6.0 at 40 and 104, a tiny number at 41 and 105 -- every harmonic sum is exact, equal maxima abound at every level, and the
    smallest k must win: level 0 reads {6.0, 40}.  All five levels equal the restatement of the device's A bit for bit."""
    npair, ndm, nt, nstack, nlevel, kmin = 2, 5, 512, 3, 5, 1
    n = np.arange(nstack * nt)
    amp = np.arange(1, npair * ndm + 1).reshape(npair, ndm) * 8.0
    tone = np.cos(2 * np.pi * 40 * n / nt) + np.cos(2 * np.pi * 104 * n / nt)
    x = (100.0 + amp[None] * tone[:, None, None]).astype(np.float32)[..., None]
    keep = np.zeros(nt // 2, np.uint8)
    keep[[40, 41, 104, 105]] = 1
    pr = PR(npair, ndm, 77, 1, nt, nstack, nlevel, 8, kmin)
    pr.set_mask(keep)
    plane, = pr.stream(x, _sizes(None, nstack * nt, 77, 77))
    A, nseg = pr.spectrum()
    pr.close()
    assert nseg == 3 and (A[..., keep == 0][..., 1:] == 3.0).all() and (A[..., 0] == 0).all()
    assert (A[..., [40, 104]] == 6.0).all() and (A[..., [41, 105]] < 1e-6).all()
    check_records(pr, plane, A)
    assert (plane['H'][..., 0] == 6.0).all() and (plane['k'][..., 0] == 40).all()
    assert (plane['H'][..., 1] == 9.0).all() and (plane['k'][..., 1] == 40).all()      # A[(40+1)/2] + A[40] = 3 + 6, first reached at k = 40


# ---------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("nprod", [1, 4])
def test_bit_identical_across_splits_reset_and_concurrent_kernels(nprod):
    """3 NT + 17 windows at NT = 256, a stack of 3: calls of 30, 10, 1 and 7 windows and a random split put segment boundaries
    at the first, an inner and the last window of a call; each run follows a Reset (the second one after 50 windows of another
    series' partial segment, which must leave no trace) and gives the same A and the same plane bit for bit; so does a fresh
    context run while X-engine contractions and xengBeamformRun are in flight."""
    npair, ndm, nwin, nt, nstack, nlevel, nwhite, kmin = 3, 37, 30, 256, 3, 5, 16, 1
    total = 3 * nt + 17
    rng = np.random.default_rng(7 + nprod)
    x = float_case(rng, total, npair, ndm, nprod)
    splits = [[30] * (total // 30) + [total % 30], [10] * (total // 10) + [total % 10], [1] * total, [7] * (total // 7) + [total % 7],
              _sizes(rng, total, nwin)]
    ends = [np.cumsum(s) for s in splits]
    assert any(nt in e for e in ends) and any((nt + 1) in e for e in ends)            # a boundary at a call's last and before its first window
    assert any(((e - np.array(s) < nt) & (e > nt + 1)).any() for s, e in zip(splits, ends))   # and inside a call
    pr = PR(npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin)
    outs = []
    for i, sizes in enumerate(splits):
        if i == 1:
            assert pr.stream(100 + x[:50][::-1], [30, 20]) == []
        ffi.call("xengPeriodReset")
        assert _info() == (0, 0, 0)
        plane, = pr.stream(x, sizes)
        A, nseg = pr.spectrum()
        assert nseg == nstack and _info() == (total, 0, 1)
        outs.append((plane.tobytes(), A.tobytes()))
    check_records(pr, plane, A)
    pr.close()
    # a fresh context beside other work: contractions on their own stream, the beamformer on this one
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    pr = PR(npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        planes, n = [], 0
        for nc in splits[0]:
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            done = pr.enqueue(x[n:n + nc])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengPeriodSync")
            p = pr.result(done)
            if p is not None:
                planes.append(p)
            n += nc
        ffi.call("xengXgpuSync")
        (plane,), (A, _) = planes, pr.spectrum()
        outs.append((plane.tobytes(), A.tobytes()))
    finally:
        xg.close()
    pr.close()
    ffi.call("xengBeamformDestroy")
    for o in outs[1:]:
        assert o[0] == outs[0][0] and o[1] == outs[0][1]
    assert (np.frombuffer(outs[0][0], RECORD)['k'] >= 1).all()


# ---------------------------------------------------------------- 4. a planted source
def planted_case(threshold):
    """NT = 1024, integer noise 0..49, and in series (1, 2) a one-window pulse every 64 windows whose amplitude is the first
    multiple of 10 at which the float32 restatement alone scores the 16-harmonic sum at twice the threshold or more."""
    nt, npair, ndm, p0, d0 = 1024, 2, 5, 1, 2
    rng = np.random.default_rng(77)
    noise = rng.integers(0, 50, (nt, npair, ndm, 1)).astype(np.float32)
    for amp in range(10, 400, 10):
        x = noise.copy()
        x[5::64, p0, d0, 0] += amp
        (A, _), = stacks(series(x, np.float32).reshape(nt, -1), nt, 1, 64, None, np.float32)
        cands = period_candidates(plane_of(harmonic_records(A.reshape(npair, ndm, -1), 5, 2)), threshold, np.arange(ndm) * 0.5, nt, 1, 1e-3)
        top = [c for c in cands if c['h'] == 16]
        if top and -top[0]['log10_pfa'] >= 2 * threshold:
            return x, (p0, d0), cands
    raise AssertionError("no amplitude clears the threshold")


def test_planted_pulse_train_is_the_only_candidate():
    """The level-16 record of the planted series is k = 16 * NT / 64 = 256 exactly -- the 16 harmonics at 16, 32 ... 256 -- and
    period_candidates returns that series and no other, as it does on the restatement's plane."""
    threshold = 6.0
    x, (p0, d0), ref_cands = planted_case(threshold)
    assert {(c['pair'], c['idm']) for c in ref_cands} == {(p0, d0)}
    npair, ndm, nt = x.shape[1], x.shape[2], x.shape[0]
    pr = PR(npair, ndm, 128, 1, nt, 1, 5, 64, 2)
    plane, = pr.stream(x, [128] * (nt // 128))
    A, _ = pr.spectrum()
    check_records(pr, plane, A)
    pr.close()
    assert plane['k'][p0, d0, 4] == 256
    cands = period_candidates(plane, threshold, np.arange(ndm) * 0.5, nt, 1, 1e-3)
    assert cands and {(c['pair'], c['idm']) for c in cands} == {(p0, d0)}
    top, = [c for c in cands if c['h'] == 16]
    assert top['k'] == 256 and abs(top['period'] - 64e-3) < 1e-12 and top['dm'] == 1.0 and -top['log10_pfa'] >= 2 * threshold - 0.1
    assert [(c['h'], c['k']) for c in cands] == [(c['h'], c['k']) for c in ref_cands]


# ---------------------------------------------------------------- 5. the ABI
def test_completing_call_without_an_output_and_the_completed_flag():
    """NT = 256, a stack of 2, calls of 100 windows: `completed` is 1 on the call that brings window 512 and 0 on every other,
    whose output (NULL or not) is untouched.  The completing call with out_dev NULL is INVALID_ARGUMENT and enqueues nothing: the
    counts stand, and the same call with an output then gives the plane of an undisturbed run."""
    npair, ndm, nt, nstack, nlevel = 2, 5, 256, 2, 2
    rng = np.random.default_rng(3)
    x = float_case(rng, 600, npair, ndm, 1)
    pr = PR(npair, ndm, 100, 1, nt, nstack, nlevel, 16, 1)
    with pytest.raises(ffi.XengError) as ei:
        pr.spectrum()
    assert ei.value.status == INVALID_STATE                     # (no segment is complete yet)
    for k in range(5):
        assert pr.enqueue(x[100 * k:100 * k + 100], out=k % 2 == 0) == 0
        ffi.call("xengPeriodSync")
        assert pr.result(0) is None
    assert _info() == (500, 1, 0) and pr.spectrum()[1] == 1
    with pytest.raises(ffi.XengError) as ei:
        pr.enqueue(x[500:600], out=False)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (500, 1, 0)
    ffi.call("xengPeriodSync")
    assert pr.result(0) is None
    plane = pr.run(x[500:600])
    assert plane is not None and _info() == (600, 0, 1)
    A, nseg = pr.spectrum()
    assert nseg == 2
    check_records(pr, plane, A)
    ffi.call("xengPeriodReset")
    again, = pr.stream(x, [100] * 6)
    assert again.tobytes() == plane.tobytes()
    pr.close()


def test_completion_tickets_and_their_query():
    """xengPeriodMark / Wait / TicketDone as the other engines': tickets count from 1 after Initialize; a ticket whose kernels have
    completed reads done = 1, every ticket does after Sync; unknown tickets (0, last + 1) and null pointers are errors; the
    backend's wait through both branches, and its other period_* calls."""
    npair, ndm, nt = 2, 40, 256
    rng = np.random.default_rng(11)
    x = rng.integers(0, 50, (nt, npair, ndm, 1)).astype(np.float32)
    ffi.call("xengPeriodInitialize", 0, npair, ndm, nt, 1, nt, 1, 2, 16, 1)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    outs = [ffi.DeviceBuffer(npair * ndm * 2 * 8) for _ in range(6)]
    tickets, done, comp = [], ctypes.c_int(-1), ctypes.c_int(-1)
    for o in outs:
        ffi.call("xengPeriodRun", din.ptr, nt, o.ptr, ctypes.byref(comp))
        assert comp.value == 1
        t = ctypes.c_ulonglong()
        ffi.call("xengPeriodMark", ctypes.byref(t))
        tickets.append(t.value)
    assert tickets == list(range(1, 7))
    ffi.call("xengPeriodTicketDone", tickets[-1], ctypes.byref(done))      # returns at once, whatever the answer
    assert done.value in (0, 1)
    ffi.call("xengPeriodWait", tickets[2])
    for t in tickets[:3]:                                                   # stream order: everything before it too
        ffi.call("xengPeriodTicketDone", t, ctypes.byref(done))
        assert done.value == 1
    ffi.call("xengPeriodSync")
    ffi.call("xengPeriodTicketDone", tickets[-1], ctypes.byref(done))
    assert done.value == 1
    planes = [o.download(np.uint8).tobytes() for o in outs]
    assert all(p == planes[0] for p in planes) and (np.frombuffer(planes[0], RECORD)['k'] >= 1).all()
    for bad in (0, tickets[-1] + 1):
        with pytest.raises(ffi.XengError):
            ffi.call("xengPeriodTicketDone", bad, ctypes.byref(done))
        with pytest.raises(ffi.XengError):
            ffi.call("xengPeriodWait", bad)
    with pytest.raises(ffi.XengError):
        ffi.call("xengPeriodTicketDone", tickets[0], None)
    with pytest.raises(ffi.XengError):
        ffi.call("xengPeriodMark", None)
    from caltech_bifrost_dsp_amd.backend import HipBackend
    be = HipBackend()
    tk = be.period_mark()
    assert tk == tickets[-1] + 1
    be.period_wait(tk)
    be.period_wait(tk)                  # already complete: answered by the query
    assert be.period_ticket_done(tk) and be.period_info() == (6 * nt, 0, 6) and be.period_guards_intact()
    A, nseg = be.period_spectrum(npair, ndm, nt)
    assert nseg == 1 and planes[0] == plane_of(harmonic_records(A, 2, 1)).tobytes()
    assert be.period_set_mask(np.ones(nt // 2, np.uint8)) == 0 and be.period_set_mask(None) == 0
    be.period_reset()
    assert be.period_info() == (0, 0, 0)
    ffi.call("xengPeriodDestroy")


def test_argument_checks_with_and_without_a_context():
    """Every INVALID_ARGUMENT of Initialize leaves a live context alone; Run with a context refuses nwin_call outside 1..nwin and
    misaligned or null pointers with nothing launched and the count unchanged; after Destroy every call that needs a context is
    INVALID_STATE."""
    pr = PR(2, 16, 64, 1, 256, 1, 2, 16, 1)
    good = (0, 2, 16, 64, 1, 256, 1, 2, 16, 1)
    for i, v in ((1, 0), (2, 0), (3, 0), (3, 257), (4, 2), (5, 128), (5, 384), (5, 1 << 15), (6, 0), (7, 0), (7, 6), (8, 4), (8, 24), (8, 256), (9, 0), (9, 8)):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeriodInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info() == (0, 0, 0)                 # (the context is still there)
    comp = ctypes.c_int(-1)
    for args in ((pr.din.ptr, 0, pr.dout.ptr), (pr.din.ptr, 65, pr.dout.ptr), (pr.din.ptr + 4, 1, pr.dout.ptr), (pr.din.ptr, 1, pr.dout.ptr + 8),
                 (None, 1, pr.dout.ptr)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeriodRun", *args, ctypes.byref(comp))
        assert ei.value.status == INVALID_ARGUMENT and _info() == (0, 0, 0)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengPeriodRun", pr.din.ptr, 1, pr.dout.ptr, None)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (0, 0, 0)
    din, dout = pr.din.ptr, pr.dout.ptr
    f, s, n, t = np.zeros(2 * 16 * 128, np.float32), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_ulonglong()
    ffi.call("xengPeriodSync")
    assert pr.result(0) is None
    pr.close()
    for name, args in (("xengPeriodRun", (din, 1, dout, ctypes.byref(s))), ("xengPeriodReset", ()), ("xengPeriodSetMask", (None,)),
                       ("xengPeriodGetInfo", (ctypes.byref(n), ctypes.byref(s), ctypes.byref(n))), ("xengPeriodGetSpectrum", (_fp(f), ctypes.byref(s))),
                       ("xengPeriodMark", (ctypes.byref(t),)), ("xengPeriodWait", (1,)), ("xengPeriodTicketDone", (1, ctypes.byref(s))),
                       ("xengPeriodSync", ()), ("xengPeriodCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name


# ---------------------------------------------------------------- 6. the chain on device rings
def chain_case():
    """Dual-pol power beams [nwindows][2 pairs][4 x 8 fine channels][4] of values 0..49 with a pulse of 8 per channel in XX of pair
    1 every 4 windows, dispersed at trial 5 of 8; the header UpchanSumBeams writes.  A period of 4 windows at NT = 256 is bin 64,
    the only harmonic below Nyquist, so that one level names the period; the dedisperser's latency S = 10 windows makes the
    search skip span 0 of 16 windows."""
    from tests.test_dedisp_cpu import header_table, power_header
    nchan, npair, N, W, nwin, nt, d0 = 4, 2, 8, 4, 16, 256, 5
    nfine = nchan * N
    dms = [float(d) for d in np.linspace(0.0, 0.14, 8)]
    hdr = power_header(nchan, npair, N, W, seq0=4096)
    table, tsamp = header_table(hdr, nfine, dms)
    S = int(table.max())
    nspan = -(-S // nwin) + nt // nwin + 1
    rng = np.random.default_rng(99)
    x = rng.integers(0, 50, (nspan * nwin, npair, nfine, 4)).astype(np.float32)
    for t in range(2, nspan * nwin - S, 4):
        x[t + table[d0], 1, np.arange(nfine), 0] += 8
    return dict(nchan=nchan, npair=npair, N=N, W=W, nwin=nwin, nt=nt, nspan=nspan, d0=d0, nfine=nfine, dms=dms, hdr=hdr, S=S, tsamp=tsamp, x=x)


def test_chain_source_dedisperse_period_search_on_device_rings():
    """Source -> BeamDedisperse -> BeamPeriodSearch: on_candidates receives exactly one candidate, the planted pair, the planted
    DM's trial (its neighbours grouped in) and the planted period of 4 windows; the one plane of the output ring equals a direct
    run of xengPeriodRun on the spans BeamDedisperse wrote, bit for bit, and its sequence begins at the first span past the
    dedisperser's partial sums."""
    c = chain_case()
    npair, nwin, nt, ndm = c['npair'], c['nwin'], c['nt'], len(c['dms'])
    r0, r1, r2 = Ring("ub-output", space="cuda"), Ring("dd-output", space="cuda"), Ring("pr-output", space="cuda_host")
    got = []
    dd = BeamDedisperse(LOG, r0, r1, npair=npair, nchan=c['nchan'], nupchan=c['N'], nwin=nwin, dms=c['dms'], gpu=0)
    pr = BeamPeriodSearch(LOG, r1, r2, npair=npair, ndm=ndm, nwin=nwin, nt=nt, nstack=1, nlevel=1, nwhite=nt // 2, kmin=2, threshold=6.0,
                          on_candidates=got.extend, gpu=0)
    mid, sink = Sink(r1, nwin * npair * ndm * 4), Sink(r2, npair * ndm * 8)
    run_blocks([dd, pr], Source(r0, [(c['hdr'], c['x'], nwin * npair * c['nfine'] * 16)]), [mid, sink])
    (dh, _, dspans), = mid.sequences
    (hd, tag, planes), = sink.sequences
    acc_len = c['W'] * c['N']
    skipped = -(-c['S'] // nwin)
    assert dh['dedisp_latency'] == c['S'] and skipped == 1 and len(dspans) == c['nspan'] and len(planes) == 1
    assert tag == hd['seq0'] == 4096 + skipped * nwin * acc_len
    assert (hd['nt'], hd['nstack'], hd['nlevel'], hd['nwhite'], hd['kmin'], hd['dedisp_latency']) == (nt, 1, 1, nt // 2, 2, c['S'])
    assert len(got) == 1, got
    cand, = got
    assert (cand['pair'], cand['idm'], cand['dm'], cand['h'], cand['k']) == (1, c['d0'], c['dms'][c['d0']], 1, 64) and cand['ntrial'] >= 1
    assert abs(cand['period'] - 4 * c['tsamp']) < 1e-12 * cand['period'] and cand['sigma'] > 6
    assert pr.stats['ncand'] == 1 and pr.stats['nstartup'] == skipped and pr.stats['nwindow'] == (c['nspan'] - skipped) * nwin
    assert pr.stats['nstack_done'] == 1 and pr.stats['ndropped'] == 0
    direct = PR(npair, ndm, nwin, 1, nt, 1, 1, nt // 2, 2)
    out = direct.stream(np.concatenate([sp.view(np.float32).reshape(nwin, npair, ndm, 1) for sp in dspans[skipped:]]), [nwin] * (c['nspan'] - skipped))
    direct.close()
    assert len(out) == 1 and out[0].tobytes() == planes[0].tobytes()
    assert (as_records(planes[0], npair, ndm, 1)['k'] >= 2).all()
