"""BeamCoherentDedisperse on the MI355X: xengCdedisp* against the restatement (tests/cdedisp_ref.py).  The filter against the float64
restatement at every transform length the emulated run covers; a pure delay; an impulse dispersed in float64; bit identity across
call sizes, after Reset against a fresh context and beside an X-engine contraction and xengBeamformRun; a NaN sample; calls that
complete no block; the ABI; Source -> BeamCoherentDedisperse -> UpchanSumBeams on device rings, and on through BeamFold.  The output
sits between two poisoned guard bands that are checked after every call, the state's guards at every close.  No wall-clock
assertions.

The bar of the float tests is not a constant: it is five times the worst gap between the complex64 and the float64 evaluation of
the restatement ON THE TEST'S OWN INPUTS (tests/cdedisp_ref.py float_gap; numpy's FFT stays in single precision on complex64
input), per row and block as max |y - y_ref| / rms(y_ref), so a quiet row is not allowed a loud row's error.  Measured here with
numpy 2.2 on Gaussian rows of scales 0.5 to 50 and unit-modulus tables: gaps of 1.7e-7 (NFFT 256), 1.6e-7 (512), 1.7e-7 (4096) and
2.0e-7 (8192), so bars of 8e-7 to 1.0e-6; the kernel's own source on host threads (tests/test_cdedisp_emul_cpu.py, no fused
multiply-adds) stands at 4.4e-7, 5.5e-7, 6.2e-7 and 7.1e-7.  Measured on the MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamCoherentDedisperse, BeamFold, UpchanSumBeams, cdedisp_plan, chirp_table  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.dedisp import KDM  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.cdedisp_ref import disperse, filter_blocks, float_gap, gaussian_rows, nblocks_after, row_error, select, unit_tables  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.upchan_beams_ref import upchan_sum_beams  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
CHAN_BW = 23925.78125
NCHAN, NBEAM, PAIR0, NPAIR, NTIME = 3, 6, 1, 2, 100     # the common shape: a selection offset, a row stride, calls unrelated to L
NB = 2 * NPAIR
# worst row error / bar over test_filter_within_the_bar_of_the_float64_restatement on the MI355X, per (NFFT, M).  (The kernel's
# source on host threads, on that test's own inputs: 0.57, 0.64, 0.52, 0.69 and 0.69 of the bar; 0.72, 0.62, 0.55, 0.66 and 0.71
# when the host compiler contracts to fused multiply-adds.)
MEASURED = "not measured"


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    s, m, n, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengCdedispGetInfo", ctypes.byref(s), ctypes.byref(m), ctypes.byref(n), ctypes.byref(b))
    return s.value, m.value, n.value, b.value


def _freqs(f0=50e6, nchan=NCHAN):
    return f0 + CHAN_BW * np.arange(nchan)


class CD:
    """The xengCdedisp context (one per process), an input buffer and the output of one call between two poisoned guard bands."""

    def __init__(self, nfft, overlap, ntime=NTIME, nchan=NCHAN, nbeam=NBEAM, pair0=PAIR0, npair=NPAIR):
        self.nfft, self.overlap, self.ntime, self.nchan, self.nbeam, self.pair0, self.npair = nfft, overlap, ntime, nchan, nbeam, pair0, npair
        self.step = nfft - overlap
        ffi.call("xengCdedispInitialize", 0, nchan, nbeam, ntime, pair0, npair, nfft, overlap)
        self.max_blocks = -(-ntime // self.step)
        assert _info() == (self.step, self.max_blocks, 0, 0)
        self.din = ffi.DeviceBuffer(nchan * nbeam * ntime * 8)
        self.unit = nchan * 2 * npair * self.step * 8
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.max_blocks * self.unit)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def set_chirp(self, table):
        table = np.ascontiguousarray(table, np.complex64)
        assert table.shape == (self.npair, self.nchan, self.nfft)
        ffi.call("xengCdedispSetChirp", _fp(table.view(np.float32)))

    def enqueue(self, x, out=True):
        """One call; returns nblocks."""
        assert x.shape == (self.nchan, self.nbeam, self.ntime)
        self.din.upload(np.ascontiguousarray(x, np.complex64))
        nb = ctypes.c_int(-1)
        ffi.call("xengCdedispRun", self.din.ptr, self.dout.ptr + GUARD if out else None, ctypes.byref(nb))
        assert 0 <= nb.value <= self.max_blocks
        return nb.value

    def result(self, nb):
        """After a sync: the nb units the call wrote (the poison is put back behind them); every byte before them and past them --
        the whole output of a call that completed nothing -- must still be poison."""
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + nb * self.unit:] == POISON).all(), "bytes past the completed blocks were written"
        if nb:
            ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + nb * self.unit].copy().view(np.complex64).reshape(nb, self.nchan, 2 * self.npair, self.step)

    def run(self, x):
        nb = self.enqueue(x)
        ffi.call("xengCdedispSync")
        return self.result(nb)

    def stream(self, x):
        """Consecutive calls over the samples of x [nchan][nbeam][k * ntime]; the blocks they completed, [nblk][nchan][2 npair][L]."""
        assert x.shape[-1] % self.ntime == 0
        out, total, done = [], _info()[2], _info()[3]
        for k in range(x.shape[-1] // self.ntime):
            y = self.run(x[..., k * self.ntime:(k + 1) * self.ntime])
            total += self.ntime
            assert done + len(y) == nblocks_after(total, self.nfft, self.overlap)
            done += len(y)
            out.append(y)
        assert _info()[2:] == (total, done)
        return np.concatenate(out)

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengCdedispCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengCdedispDestroy")
        self.din.free()
        self.dout.free()


def _length(nfft, overlap, nblk, ntime=NTIME):
    """Samples, a whole number of calls, that complete at least nblk blocks."""
    return -(-(nfft + (nblk - 1) * (nfft - overlap)) // ntime) * ntime


# ---------------------------------------------------------------- 1. the filter against float64
@pytest.mark.parametrize("nfft,overlap", [(256, 64), (512, 0), (512, 256), (4096, 1216), (8192, 2432)])
def test_filter_within_the_bar_of_the_float64_restatement(nfft, overlap):
    """3 channels x 6 beams of Gaussian rows of scales 0.5 to 50, pairs 1 and 2 selected, a dispersive table of another DM per
    pair (sweeps of 0.15 and 0.33 NFFT at the lowest channel: within M where there is one, wrapped where there is none -- the
    restatement wraps alike), one selected row of zeros, three blocks and a few calls more: every row and block within five times
    the complex64 restatement's own gap, the zero row exactly zero, and nothing of the unselected beams anywhere."""
    n = _length(nfft, overlap, 3)
    rng = np.random.default_rng(nfft + overlap)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    x[1, 2 * PAIR0 + 2] = 0
    dms = [0.4 * nfft / 256, 0.9 * nfft / 256]
    table = chirp_table(_freqs(), CHAN_BW, dms, nfft)
    rows = select(x, PAIR0, NPAIR)
    gap = float_gap(rows, table, nfft, overlap)
    cd = CD(nfft, overlap)
    cd.set_chirp(table)
    got = cd.stream(x)
    cd.close()
    ref = filter_blocks(rows, table, nfft, overlap)
    assert len(got) == len(ref) >= 3
    err = row_error(got, ref)
    print("NFFT %d M %d: complex64 gap %.2e, bar %.2e, worst row %.2e (%.2f of the bar)" % (nfft, overlap, gap, 5 * gap, err.max(), err.max() / (5 * gap)))
    assert 1e-7 < gap < 1e-6
    assert (err <= 5 * gap).all(), (err.max(), 5 * gap)
    assert (got[:, 1, 2] == 0).all()


# ---------------------------------------------------------------- 2. a pure delay
@pytest.mark.parametrize("nfft,overlap", [(256, 64), (8192, 2432)])
def test_pure_delay_shifts_the_stream_without_a_seam(nfft, overlap):
    """T = exp(-2 pi i k d / NFFT) / NFFT delays by d samples: output sample i is input sample i + M/2 - d, for d = M/2, 0 and -M/2,
    to the bar, across the block seams.  A wrong discard region or a wrong overlap shows as wrapped samples.  After Initialize the
    table is 1/NFFT: the d = 0 case without a SetChirp."""
    n = _length(nfft, overlap, 3)
    rng = np.random.default_rng(17)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    rows = select(x, PAIR0, NPAIR)
    k = np.arange(nfft)
    cd = CD(nfft, overlap)
    for d in (None, overlap // 2, 0, -overlap // 2):
        ffi.call("xengCdedispReset")
        table = np.broadcast_to(np.exp(-2j * np.pi * k * (d or 0) / nfft) / nfft, (NPAIR, NCHAN, nfft)).astype(np.complex64)
        if d is not None:
            cd.set_chirp(table)
        got = cd.stream(x)
        nblk = len(got)
        flat = got.transpose(1, 2, 0, 3).reshape(NCHAN, NB, nblk * cd.step)
        lo = overlap // 2 - (d or 0)
        exp = rows[:, :, lo:lo + nblk * cd.step]
        bar = 5 * float_gap(rows, table, nfft, overlap)
        err = np.max(np.abs(flat.astype(np.complex128) - exp), axis=-1) / np.sqrt(np.mean(np.abs(exp.astype(np.complex128)) ** 2, axis=-1))
        print("NFFT %d d %r: bar %.2e, worst row %.2e" % (nfft, d, bar, err.max()))
        assert (err <= bar).all(), (d, err.max(), bar)
    cd.close()


# ---------------------------------------------------------------- 3. a dispersed impulse
def test_dispersed_impulse_comes_back_in_one_sample():
    """40 MHz, DM 10 (a sweep of 742 samples), NFFT 4096, M 1216: an impulse dispersed in float64, rounded to complex64, comes back
    in the sample it was sent in, mid-block and two samples from either edge of block 1's output; its share of the row's output
    energy is the float64 restatement's on the same input (0.99996 to 0.99998) less the bar."""
    nfft, overlap, f_c, dm = 4096, 1216, 40e6, 10.0
    step = nfft - overlap
    n = _length(nfft, overlap, 3)
    table = chirp_table(_freqs(f_c), CHAN_BW, [0.0, dm], nfft)
    cd = CD(nfft, overlap)
    cd.set_chirp(table)
    for i_out in (step + step // 2, step + 2, 2 * step - 3):
        imp = np.zeros(n, np.complex128)
        imp[i_out + overlap // 2] = 100.0
        x = np.zeros((NCHAN, NBEAM, n), np.complex64)
        x[0, 2 * PAIR0 + 3] = disperse(imp, f_c, CHAN_BW, dm, KDM)
        rows = select(x, PAIR0, NPAIR)
        ffi.call("xengCdedispReset")
        got = cd.stream(x)
        ref = filter_blocks(rows, table, nfft, overlap)
        bar = 5 * float_gap(rows[:1, 2:], table[1:, :1], nfft, overlap)
        p, q = np.abs(got[:, 0, 3].astype(np.complex128).reshape(-1)) ** 2, np.abs(ref[:, 0, 3].reshape(-1)) ** 2
        print("impulse at %d: share %.6f, float64 %.6f, bar %.2e" % (i_out, p.max() / p.sum(), q.max() / q.sum(), bar))
        assert int(np.argmax(p)) == int(np.argmax(q)) == i_out
        assert q.max() / q.sum() > 0.9999 and p.max() / p.sum() >= q.max() / q.sum() - bar
        rest = np.ones((NCHAN, NB), bool)
        rest[0, 3] = False
        assert (got[:, rest] == 0).all()
    cd.close()


# ---------------------------------------------------------------- 4., 5. bit identity
def test_bit_identical_across_call_sizes():
    """One stream through contexts of ntime 96, 100 and 250 (L = 192: the last completes one or two blocks in a call; blocks
    complete on the last sample of a call and inside calls): the same blocks bit for bit."""
    nfft, overlap, n = 256, 64, 6000
    rng = np.random.default_rng(23)
    x = gaussian_rows(rng, NCHAN, NBEAM, 96 * 63)
    table = unit_tables(rng, NPAIR, NCHAN, nfft)
    nblk = nblocks_after(n, nfft, overlap)
    outs = []
    for ntime in (96, 100, 250):
        m = n if n % ntime == 0 else 96 * 63
        cd = CD(nfft, overlap, ntime=ntime)
        cd.set_chirp(table)
        got = cd.stream(x[..., :m])
        cd.close()
        assert len(got) >= nblk and (cd.max_blocks == 2) == (ntime == 250)
        outs.append(got[:nblk].tobytes())
    assert outs[1] == outs[0] and outs[2] == outs[0]
    ends = [np.arange(1, 6048 // t + 1) * t for t in (96, 100, 250)]
    done = nfft + (nfft - overlap) * np.arange(nblk)            # samples at which the blocks complete
    assert any(np.isin(done, e).any() for e in ends) and not all(np.isin(done, e).all() for e in ends)


def test_bit_identical_after_reset_in_a_fresh_context_and_beside_other_kernels():
    """The same stream: from Initialize; after a Reset that follows 500 samples of another stream (a partial block, which must
    leave no trace); and in a fresh context while X-engine contractions run on their streams and xengBeamformRun on this one."""
    nfft, overlap = 512, 256
    n = _length(nfft, overlap, 4)
    rng = np.random.default_rng(29)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    table = unit_tables(rng, NPAIR, NCHAN, nfft)
    cd = CD(nfft, overlap)
    cd.set_chirp(table)
    outs = [cd.stream(x).tobytes()]
    ffi.call("xengCdedispReset")
    assert _info()[2:] == (0, 0)
    assert len(cd.stream(7 + x[..., 300:800][..., ::-1])) == 0 and _info()[2:] == (500, 0)
    ffi.call("xengCdedispReset")
    outs.append(cd.stream(x).tobytes())
    cd.close()
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    cd = CD(nfft, overlap)
    cd.set_chirp(table)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(n // NTIME):
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            nb = cd.enqueue(x[..., k * NTIME:(k + 1) * NTIME])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengCdedispSync")
            got.append(cd.result(nb))
        ffi.call("xengXgpuSync")
        outs.append(np.concatenate(got).tobytes())
    finally:
        xg.close()
    cd.close()
    ffi.call("xengBeamformDestroy")
    assert len(outs[0]) == nblocks_after(n, nfft, overlap) * cd.unit and outs[1] == outs[0] and outs[2] == outs[0]


# ---------------------------------------------------------------- 6. a non-finite sample
def test_one_nan_takes_the_two_blocks_of_its_row_that_hold_it():
    """NFFT 256, M 64: sample 400 lies in [384, 448), which blocks 1 and 2 share.  A NaN there makes exactly those two blocks of its
    row NaN, every sample of them, and every other word is bit-identical to the clean run."""
    nfft, overlap = 256, 64
    n = _length(nfft, overlap, 4)
    rng = np.random.default_rng(31)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    table = unit_tables(rng, NPAIR, NCHAN, nfft)
    cd = CD(nfft, overlap)
    cd.set_chirp(table)
    clean = cd.stream(x)
    bad = x.copy()
    bad[2, 2 * PAIR0 + 1, 400] = np.nan
    ffi.call("xengCdedispReset")
    got = cd.stream(bad)
    cd.close()
    hit = np.zeros(got.shape[:3], bool)
    hit[1:3, 2, 1] = True
    assert np.isnan(got[hit].real).all() and np.isnan(got[hit].imag).all()
    assert got[~hit].tobytes() == clean[~hit].tobytes() and not np.isnan(clean.view(np.float32)).any()


# ---------------------------------------------------------------- 7., 8. the ABI
def test_nblocks_info_null_output_and_set_chirp_mid_stream():
    """NFFT 256, M 64, calls of 100: nblocks is 0, 0, 1, 0, 1 ... as the sample count says, and a call that completes nothing leaves
    its output (NULL or not) untouched.  A completing call with out_dev NULL is INVALID_ARGUMENT, enqueues nothing and counts
    nothing: the same call with an output then completes the block.  SetChirp between two calls holds from the next block: blocks 0
    and 1 are the first table's, block 2 on the second's, on one stream.  A table with a non-finite word is refused and changes
    nothing."""
    nfft, overlap = 256, 64
    n = _length(nfft, overlap, 5)
    rng = np.random.default_rng(37)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    rows = select(x, PAIR0, NPAIR)
    t0, t1 = unit_tables(rng, NPAIR, NCHAN, nfft), unit_tables(rng, NPAIR, NCHAN, nfft)
    cd = CD(nfft, overlap)
    cd.set_chirp(t0)
    got, flags = [], []
    for k in range(n // NTIME):
        call = x[..., k * NTIME:(k + 1) * NTIME]
        want = nblocks_after((k + 1) * NTIME, nfft, overlap) - nblocks_after(k * NTIME, nfft, overlap)
        if k == 5:                              # (448 of 500 samples: blocks 0 and 1 are out, block 2 needs sample 639)
            assert _info()[3] == 2
            bad = t1.copy()
            bad[1, 2, 77] = np.inf
            with pytest.raises(ffi.XengError) as ei:
                cd.set_chirp(bad)
            assert ei.value.status == INVALID_ARGUMENT
            cd.set_chirp(t1)
        if want:
            cd.din.upload(np.ascontiguousarray(call))
            nb = ctypes.c_int(-1)
            with pytest.raises(ffi.XengError) as ei:
                ffi.call("xengCdedispRun", cd.din.ptr, None, ctypes.byref(nb))
            assert ei.value.status == INVALID_ARGUMENT and _info()[2] == k * NTIME
            y = cd.run(call)
        else:
            nb = cd.enqueue(call, out=(k % 2 == 0))
            ffi.call("xengCdedispSync")
            y = cd.result(nb)
        assert len(y) == want
        flags.append(want)
        got.append(y)
    got = np.concatenate(got)
    cd.close()
    assert flags[:5] == [0, 0, 1, 0, 1] and len(got) == 5
    bar = 5 * max(float_gap(rows, t0, nfft, overlap), float_gap(rows, t1, nfft, overlap))
    assert (row_error(got[:2], filter_blocks(rows, t0, nfft, overlap, count=2)) <= bar).all()
    assert (row_error(got[2:], filter_blocks(rows, t1, nfft, overlap, first=2)) <= bar).all()
    assert (row_error(got[2:], filter_blocks(rows, t0, nfft, overlap, first=2)) > 0.1).all()


def test_completion_tickets_and_argument_checks_with_and_without_a_context():
    """Tickets count from 1 after Initialize and every one is done after Sync; unknown tickets are errors.  Every INVALID_ARGUMENT
    of Initialize leaves a live context alone; Run refuses misaligned and null pointers with nothing launched and the count
    unchanged; after Destroy every call that needs a context is INVALID_STATE."""
    cd = CD(256, 64)
    x = np.zeros((NCHAN, NBEAM, NTIME), np.complex64)
    t, d, nb = ctypes.c_ulonglong(), ctypes.c_int(-1), ctypes.c_int(-1)
    ffi.call("xengCdedispMark", ctypes.byref(t))
    assert t.value == 1
    cd.enqueue(x)
    ffi.call("xengCdedispMark", ctypes.byref(t))
    assert t.value == 2
    ffi.call("xengCdedispWait", 2)
    ffi.call("xengCdedispSync")
    for k in (1, 2):
        ffi.call("xengCdedispTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, 3):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdedispWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, NBEAM, NTIME, 0, 1, 256, 64), (0, NCHAN, NBEAM, NTIME, 3, 1, 256, 64), (0, NCHAN, NBEAM, NTIME, 0, 1, 384, 64),
                 (0, NCHAN, NBEAM, NTIME, 0, 1, 256, 63), (0, NCHAN, NBEAM, NTIME, 0, 1, 256, 130), (0, NCHAN, NBEAM, NTIME, 0, 1, 1 << 14, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdedispInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info() == (192, 1, NTIME, 0)
    for args in ((None, cd.dout.ptr + GUARD, ctypes.byref(nb)), (cd.din.ptr, cd.dout.ptr + GUARD, None), (cd.din.ptr + 8, cd.dout.ptr + GUARD, ctypes.byref(nb)),
                 (cd.din.ptr, cd.dout.ptr + GUARD + 8, ctypes.byref(nb))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdedispRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengCdedispSync")
    assert _info() == (192, 1, NTIME, 0) and len(cd.result(0)) == 0
    cd.close()
    s, n = ctypes.c_int(), ctypes.c_longlong()
    f = np.zeros(4, np.float32)
    for name, args in (("xengCdedispRun", (cd.din.ptr or 4096, 4096, ctypes.byref(nb))), ("xengCdedispReset", ()), ("xengCdedispSetChirp", (_fp(f),)),
                       ("xengCdedispGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), ctypes.byref(n))), ("xengCdedispMark", (ctypes.byref(t),)),
                       ("xengCdedispWait", (1,)), ("xengCdedispTicketDone", (1, ctypes.byref(d))), ("xengCdedispSync", ()),
                       ("xengCdedispCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCdedispDestroy")


# ---------------------------------------------------------------- 9., 10. the blocks on device rings
def _voltage_header(nchan, nbeam, seq0, sfreq):
    hdr = source_header(nchan, nbeam, 1, seq0=seq0, sfreq=sfreq, chan_bw=CHAN_BW)
    hdr.update(nbeam=nbeam, nstand=nbeam, npol=1, nbit=32, complex=True)
    return hdr


def _ring_bytes(v, g):
    return np.concatenate([np.ascontiguousarray(v[..., k * g:(k + 1) * g]).reshape(-1) for k in range(v.shape[-1] // g)])


@pytest.mark.parametrize("g", [NTIME, 1000])
def test_blocks_dedisperse_then_upchannelise_on_device_rings(g):
    """Source -> BeamCoherentDedisperse (planned: multiple_of 8) -> UpchanSumBeams (nupchan 8) on device rings, 60 MHz, DMs 2 and 4
    (sweeps of 44 and 88 samples at the lowest channel): the plan is (512, 136); every span of the dedisperser is one block of the
    float64 restatement to the bar, its header says pairs, DMs and plan, and seq0 = the input's + M/2; the upchanneliser accepts
    it and writes, per span, the float64 restatement of ITS contract applied to the float64 blocks (rtol 1e-4 of the span's
    largest power: two fp32 stages).  Gulps of 100 samples complete no block or one, which the kernel writes into its span; gulps
    of 1000 two or three, written side by side into a device buffer and moved span by span on the copy stream."""
    nup, seq0, sfreq, dms = 8, 5000, 60e6, [2.0, 4.0]
    nfft, overlap = cdedisp_plan(_freqs(sfreq), CHAN_BW, 4.0, nup)
    assert (nfft, overlap) == (512, 136)
    step = nfft - overlap
    n = _length(nfft, overlap, 4, g)
    rng = np.random.default_rng(41)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    hdr = _voltage_header(NCHAN, NBEAM, seq0, sfreq)
    r0, r1, r2 = Ring("bf-output", space="cuda"), Ring("cd-output", space="cuda"), Ring("ub-output", space="cuda")
    cd = BeamCoherentDedisperse(LOG, r0, r1, NCHAN, NBEAM, g, dms, pair0=PAIR0, npair=NPAIR, multiple_of=nup, gpu=0)
    ub = UpchanSumBeams(LOG, r1, r2, nchan=NCHAN, nbeam=NB, ntime_gulp=step, nupchan=nup, nframe_sum=step // nup, gpu=0)
    mid, sink = Sink(r1, NCHAN * NB * step * 8), Sink(r2, NPAIR * NCHAN * nup * 16)
    run_blocks([cd, ub], Source(r0, [(hdr, _ring_bytes(x, g), NCHAN * NBEAM * g * 8)]), [mid, sink])
    (ch, ctag, cspans), = mid.sequences
    (uh, utag, uspans), = sink.sequences
    nblk = nblocks_after(n, nfft, overlap)
    assert len(cspans) == len(uspans) == nblk >= 4 and ctag == ch['seq0'] == utag == uh['seq0'] == seq0 + overlap // 2
    assert (ch['nbeam'], ch['nstand'], ch['pair0'], ch['cdedisp_dm'], ch['cdedisp_nfft'], ch['cdedisp_overlap']) == (NB, NB, PAIR0, dms, nfft, overlap)
    assert uh['cdedisp_dm'] == dms and uh['nupchan'] == nup and uh['pair0'] == 0 and not {'acc_len', 'ntime_sum', 'nupchan'} & set(ch)
    table = chirp_table(_freqs(sfreq), CHAN_BW, dms, nfft)
    rows = select(x, PAIR0, NPAIR)
    ref = filter_blocks(rows, table, nfft, overlap)
    got = np.array([s.view(np.complex64).reshape(NCHAN, NB, step) for s in cspans])
    bar = 5 * float_gap(rows, table, nfft, overlap)
    assert (row_error(got, ref) <= bar).all()
    for j, s in enumerate(uspans):
        exp = upchan_sum_beams(ref[j], nup, step // nup, 0, step)
        assert np.allclose(s.view(np.float32).reshape(exp.shape), exp, rtol=0, atol=1e-4 * np.abs(exp).max())
    assert cd.stats['nblock'] == nblk and cd.stats['ndropped'] == 0


def _fold_chain(first_ring_data, hdr, gulp_bytes, dedisperse, nchan, step, nup, nbin, pulsar, nspan, dm):
    """Source -> [BeamCoherentDedisperse ->] UpchanSumBeams -> BeamFold on device rings; (the dedisperser's sequences or None, the
    fold's)."""
    r0, r1, r2 = Ring("bf-output", space="cuda"), Ring("ub-output", space="cuda"), Ring("fold-output", space="cuda_host")
    blocks, sinks, rin = [], [], r0
    if dedisperse:
        rc = Ring("cd-output", space="cuda")
        blocks.append(BeamCoherentDedisperse(LOG, r0, rc, nchan, 2, NTIME, [dm], nfft=256, overlap=256 - step, gpu=0))
        sinks.append(Sink(rc, nchan * 2 * step * 8))
        rin = rc
    nwin = step // nup
    blocks.append(UpchanSumBeams(LOG, rin, r1, nchan=nchan, nbeam=2, ntime_gulp=step, nupchan=nup, nframe_sum=1, gpu=0))
    blocks.append(BeamFold(LOG, r1, r2, npair=1, nchan=nchan, nupchan=nup, nwin=nwin, nbin=nbin, pulsars=[pulsar], nsub=nspan, gpu=0))
    sinks.append(Sink(r2, nbin * 4))
    run_blocks(blocks, Source(r0, [(hdr, first_ring_data, gulp_bytes)]), sinks)
    return (sinks[0].sequences if dedisperse else None), sinks[-1].sequences


def test_full_chain_folds_a_dispersed_pulse_train_into_one_bin():
    """Two coarse channels at 40 MHz, one pair, a train of one-sample pulses every 96 samples in unit noise, dispersed in float64 at
    DM 0.55 inside each channel (a sweep of 41 samples, five windows of 8) and delayed between the channels as the cold plasma
    does.  Source -> BeamCoherentDedisperse (NFFT 256, M 64) -> UpchanSumBeams (nupchan 8, every frame a window) -> BeamFold (12
    bins of one window, one sub-integration of 20 spans).  The float64 chain is the float64 restatement of the dedisperser, rounded
    to complex64 and sent through the same two blocks with the dedisperser's header.  The folded profile's peak bin is the float64
    chain's, bin 5, where the train was put; its peak-to-mean is within four bars of it (a power is quadratic in the voltages, and
    a ratio takes two)."""
    nchan, nup, nbin, dm, sfreq, nfft, overlap, nspan, period = 2, 8, 12, 0.55, 40e6, 256, 64, 20, 96
    step = nfft - overlap
    n = _length(nfft, overlap, nspan)
    assert nblocks_after(n, nfft, overlap) == nspan
    rng = np.random.default_rng(43)
    freqs = _freqs(sfreq, nchan)
    f_ref = (sfreq - CHAN_BW / 2) + CHAN_BW / nup * (nchan * nup - 1)          # the highest fine channel: fold_rotations' reference
    x = np.zeros((nchan, 2, n), np.complex64)
    for c in range(nchan):
        lag = int(np.rint(KDM * dm * ((freqs[c] * 1e-6) ** -2 - (f_ref * 1e-6) ** -2) * CHAN_BW))
        train = np.zeros(n, np.complex128)
        train[(44 + lag) % period::period] = 30.0                               # (44: the middle of bin 5 at the reference frequency)
        for b in range(2):
            noise = rng.standard_normal(n) + 1j * rng.standard_normal(n)
            x[c, b] = disperse(train, freqs[c], CHAN_BW, dm, KDM) + noise
    hdr = _voltage_header(nchan, 2, 0, sfreq)
    pulsar = dict(f0=CHAN_BW / period, dm=dm)
    gulp = nchan * 2 * NTIME * 8
    cseqs, fseqs = _fold_chain(_ring_bytes(x, NTIME), hdr, gulp, True, nchan, step, nup, nbin, pulsar, nspan, dm)
    (ch, _, cspans), = cseqs
    (_, _, (prof,)), = fseqs
    assert len(cspans) == nspan and ch['cdedisp_dm'] == [dm] and ch['seq0'] == overlap // 2
    table = chirp_table(freqs, CHAN_BW, [dm], nfft)
    ref = filter_blocks(x, table, nfft, overlap).astype(np.complex64)
    _, ((_, _, (prof64,)),) = _fold_chain(ref.reshape(-1), ch, nchan * 2 * step * 8, False, nchan, step, nup, nbin, pulsar, nspan, dm)
    p, q = (a.view(np.float32).astype(np.float64) for a in (prof, prof64))
    bar = 5 * float_gap(x, table, nfft, overlap)
    ptm = lambda a: a.max() / a.mean()
    print("peak bins %d / %d, peak-to-mean %.6f (float64 chain %.6f), bar %.2e" % (p.argmax(), q.argmax(), ptm(p), ptm(q), bar))
    assert p.argmax() == q.argmax() == 5 and abs(ptm(p) - ptm(q)) <= 4 * bar * ptm(q)
    assert ptm(q) > 6                           # (12 bins: a profile with everything in one bin reads 12)
