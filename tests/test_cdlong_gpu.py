"""BeamCoherentDedisperseLong on the MI355X: xengCdlong* against the restatement (tests/cdedisp_ref.py, whose contract it shares, and
the four-step complex64 route of tests/cdlong_ref.py).  The filter against the float64 restatement from 2^14 to 2^20 points; a pure
delay; an impulse dispersed in float64 under cdedisp_plan_long's plan; bit identity across call sizes, after Reset and in a fresh
context; a NaN sample; calls that complete no block; SetChirp mid-stream; the ABI; the input pinned byte for byte; Source ->
BeamCoherentDedisperseLong -> UpchanSumBeams on device rings against the C-ABI call.  The output sits between two poisoned guard
bands that are checked after every call, the state's guards at every close.  No wall-clock assertions.

The bar is not a constant: per row and block, max |y - y_ref| / rms(y_ref) against the float64 restatement at most five times a
complex64 gap ON THE TEST'S OWN INPUTS, the larger of the direct complex64 evaluation's (float_gap) and the four-step complex64
evaluation's (four_step_gap: the route carries two more roundings per element than a direct FFT).  Measured here with numpy 2.2 on
the inputs of test_filter_within_the_bar_of_the_float64_restatement, as direct gap / four-step gap, and the kernels' own source on
host threads (tests/test_cdlong_emul_cpu.py's driver, no fused multiply-adds) on Gaussian rows and unit-modulus tables of those
sizes: (2^16, 20000) 1.75e-7 / 3.08e-7, kernel 9.3e-7 (0.60 of the bar); (2^17, 40000) 2.09e-7 / 3.29e-7, kernel 8.3e-7 (0.50);
(2^20, 2^18) 2.37e-7 / 3.47e-7, kernel 1.14e-6 (0.66).  Measured on the MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamCoherentDedisperseLong, UpchanSumBeams, cdedisp_plan_long, chirp_table  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.dedisp import KDM  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import input_pins  # noqa: E402
from tests.cdedisp_ref import disperse, filter_blocks, gaussian_rows, nblocks_after, row_error, select, unit_tables  # noqa: E402
from tests.cdlong_ref import gaps  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.upchan_beams_ref import upchan_sum_beams  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
CHAN_BW = 23925.78125
NCHAN, NBEAM, PAIR0, NPAIR, NTIME = 2, 6, 1, 2, 4000     # the common shape: a selection offset, a row stride, calls unrelated to L
NB = 2 * NPAIR
NFFT, M = 1 << 14, 4560                                  # the common plan: N1 = N2 = 128, M/2 = 2280 no multiple of the column tile
L = NFFT - M
# worst row error / bar over test_filter_within_the_bar_of_the_float64_restatement on the MI355X, per (NFFT, M)
MEASURED = {(1 << 14, 4560): 0.54, (1 << 15, 0): 0.56, (1 << 15, 1 << 14): 0.55, (1 << 17, 40000): 0.59, (1 << 20, 1 << 18): 0.58}
# (worst rows 7.7e-7, 8.4e-7, 8.1e-7, 8.9e-7 and 9.4e-7 against bars of 1.44e-6 to 1.62e-6: direct gaps 1.9e-7 to 2.2e-7, four-step gaps
# 2.9e-7 to 3.2e-7.  The pure delay: worst row 7.7e-7 at 2^14 and 1.0e-6 at 2^17 against bars of 1.3e-6 to 1.5e-6.  The impulse:
# shares 0.999998 mid-block and 0.999996 at either edge, the float64 restatement's to six places.)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    s, m, n, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengCdlongGetInfo", ctypes.byref(s), ctypes.byref(m), ctypes.byref(n), ctypes.byref(b))
    return s.value, m.value, n.value, b.value


def _freqs(f0=50e6, nchan=NCHAN):
    return f0 + CHAN_BW * np.arange(nchan)


class CL:
    """The xengCdlong context (one per process), an input buffer and the output of one call between two poisoned guard bands."""

    def __init__(self, nfft=NFFT, overlap=M, ntime=NTIME, nchan=NCHAN, nbeam=NBEAM, pair0=PAIR0, npair=NPAIR):
        self.nfft, self.overlap, self.ntime, self.nchan, self.nbeam, self.pair0, self.npair = nfft, overlap, ntime, nchan, nbeam, pair0, npair
        self.step = nfft - overlap
        ffi.call("xengCdlongInitialize", 0, nchan, nbeam, ntime, pair0, npair, nfft, overlap)
        self.max_blocks = -(-ntime // self.step)
        assert _info() == (self.step, self.max_blocks, 0, 0)
        self.din = ffi.DeviceBuffer(nchan * nbeam * ntime * 8)
        self.unit = nchan * 2 * npair * self.step * 8
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.max_blocks * self.unit)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def set_chirp(self, table):
        """the whole table [npair][nchan][nfft], uploaded pair by pair"""
        table = np.ascontiguousarray(table, np.complex64)
        assert table.shape == (self.npair, self.nchan, self.nfft)
        for p in range(self.npair):
            ffi.call("xengCdlongSetChirp", p, _fp(table[p].view(np.float32)))

    def enqueue(self, x, out=True):
        """One call; returns nblocks."""
        assert x.shape == (self.nchan, self.nbeam, self.ntime)
        self.din.upload(np.ascontiguousarray(x, np.complex64))
        nb = ctypes.c_int(-1)
        ffi.call("xengCdlongRun", self.din.ptr, self.dout.ptr + GUARD if out else None, ctypes.byref(nb))
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
        ffi.call("xengCdlongSync")
        return self.result(nb)

    def stream(self, x):
        """Consecutive calls over the samples of x [nchan][nbeam][k * ntime]; the blocks they completed, [nblk][nchan][2 npair][L]."""
        assert x.shape[-1] % self.ntime == 0
        out, total, done = [np.empty((0, self.nchan, 2 * self.npair, self.step), np.complex64)], _info()[2], _info()[3]
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
        ffi.call("xengCdlongCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengCdlongDestroy")
        self.din.free()
        self.dout.free()


def _length(nfft, overlap, nblk, ntime=NTIME):
    """Samples, a whole number of calls, that complete at least nblk blocks."""
    return -(-(nfft + (nblk - 1) * (nfft - overlap)) // ntime) * ntime


# ---------------------------------------------------------------- 1. the filter against float64
def _filter_case(nfft, overlap, nchan, npair, nblk, ntime):
    nbeam, pair0 = 2 * npair + 2, 1
    n = _length(nfft, overlap, nblk, ntime)
    rng = np.random.default_rng(nfft + overlap)
    x = gaussian_rows(rng, nchan, nbeam, n)
    zc, zb = nchan - 1, 2 * npair - 2
    x[zc, 2 * pair0 + zb] = 0
    dms = [0.4 * nfft / 256, 0.9 * nfft / 256][:npair]
    table = chirp_table(_freqs(nchan=nchan), CHAN_BW, dms, nfft)
    rows = select(x, pair0, npair)
    ref = filter_blocks(rows, table, nfft, overlap)
    direct, four = gaps(rows, table, nfft, overlap, ref)
    gap = max(direct, four)
    cl = CL(nfft, overlap, ntime, nchan, nbeam, pair0, npair)
    cl.set_chirp(table)
    got = cl.stream(x)
    cl.close()
    assert len(got) == len(ref) >= nblk
    err = row_error(got, ref)
    print("NFFT %d M %d: direct gap %.2e, four-step gap %.2e, bar %.2e, worst row %.2e (%.2f of the bar)"
          % (nfft, overlap, direct, four, 5 * gap, err.max(), err.max() / (5 * gap)))
    assert 1e-7 < gap < 1e-6
    assert (err <= 5 * gap).all(), (err.max(), 5 * gap)
    assert (got[:, zc, zb] == 0).all()


@pytest.mark.parametrize("nfft,overlap,nchan,npair,nblk,ntime", [(1 << 14, 4560, 2, 2, 3, 4000), (1 << 15, 0, 2, 2, 3, 8000), (1 << 15, 1 << 14, 2, 2, 3, 8000),
                                                                (1 << 17, 40000, 2, 1, 3, 40000), (1 << 20, 1 << 18, 1, 1, 2, 200000)])
def test_filter_within_the_bar_of_the_float64_restatement(nfft, overlap, nchan, npair, nblk, ntime):
    """Gaussian rows of scales 0.5 to 50, pairs from 1 on selected of one pair more, a dispersive table of another DM per pair
    (sweeps of 0.15 and 0.33 NFFT at the lowest channel: within M where there is one, wrapped where there is none -- the restatement
    wraps alike), one selected row of zeros, three blocks (two at 2^20) and a few calls more: every row and block within five times
    the larger complex64 gap, the zero row exactly zero.  (2^14, 4560): N1 = N2 = 128; 2^15: 128 x 256, the extreme overlaps; 2^17:
    256 x 512, pass B two rows per work-group; 2^20: 512 x 2048, 64 KiB tiles, one channel and one pair."""
    _filter_case(nfft, overlap, nchan, npair, nblk, ntime)


def test_input_is_byte_identical_after_every_call():
    """in_dev is `const` in include/xeng.h: the (2^14, 4560) case again with every upload of the input pinned and compared byte for
    byte before the next upload, before the free and at the end (tests/input_pins.py)."""
    with input_pins.recording(ffi.DeviceBuffer) as rec:
        _filter_case(1 << 14, 4560, 2, 2, 3, 4000)
    assert rec.nchecked >= 3, (rec.nchecked, rec.names[:4])


# ---------------------------------------------------------------- 2. a pure delay
@pytest.mark.parametrize("nfft,overlap,ntime", [(1 << 14, 4560, 4000), (1 << 17, 40000, 40000)])
def test_pure_delay_shifts_the_stream_without_a_seam(nfft, overlap, ntime):
    """T = exp(-2 pi i k d / NFFT) / NFFT delays by d samples: output sample i is input sample i + M/2 - d, for d = M/2, 0 and -M/2,
    to the bar, across the block seams.  A wrong discard region or a wrong overlap shows as wrapped samples.  After Initialize the
    table is 1/NFFT: the d = 0 case without a SetChirp.  One channel, one pair."""
    nchan, nbeam, pair0, npair = 1, 4, 1, 1
    n = _length(nfft, overlap, 3, ntime)
    rng = np.random.default_rng(17)
    x = gaussian_rows(rng, nchan, nbeam, n)
    rows = select(x, pair0, npair)
    k = np.arange(nfft)
    cl = CL(nfft, overlap, ntime, nchan, nbeam, pair0, npair)
    for d in (None, overlap // 2, 0, -overlap // 2):
        ffi.call("xengCdlongReset")
        table = np.broadcast_to(np.exp(-2j * np.pi * ((k * (d or 0)) % nfft) / nfft) / nfft, (npair, nchan, nfft)).astype(np.complex64)
        if d is not None:
            cl.set_chirp(table)
        got = cl.stream(x)
        nblk = len(got)
        flat = got.transpose(1, 2, 0, 3).reshape(nchan, 2 * npair, nblk * cl.step)
        lo = overlap // 2 - (d or 0)
        exp = rows[:, :, lo:lo + nblk * cl.step]
        bar = 5 * max(gaps(rows, table, nfft, overlap))
        err = np.max(np.abs(flat.astype(np.complex128) - exp), axis=-1) / np.sqrt(np.mean(np.abs(exp.astype(np.complex128)) ** 2, axis=-1))
        print("NFFT %d d %r: bar %.2e, worst row %.2e" % (nfft, d, bar, err.max()))
        assert nblk >= 3 and (err <= bar).all(), (d, err.max(), bar)
    cl.close()


# ---------------------------------------------------------------- 3. a dispersed impulse
def test_dispersed_impulse_comes_back_in_one_sample():
    """20 MHz, DM 10 (a sweep of 5937 samples), cdedisp_plan_long's plan (2^15, 8908): an impulse dispersed in float64, rounded to
    complex64, comes back in the sample it was sent in, mid-block and two samples from either edge of block 1's output; its share of
    the row's output energy is within 1e-4 of the float64 restatement's own share on the same input."""
    f_c, dm = 20e6, 10.0
    nfft, overlap = cdedisp_plan_long(_freqs(f_c), CHAN_BW, dm)
    assert (nfft, overlap) == (1 << 15, 8908)          # (1.5 sweeps are 8906.2: the next even number)
    step, ntime = nfft - overlap, 8000
    n = _length(nfft, overlap, 3, ntime)
    table = chirp_table(_freqs(f_c), CHAN_BW, [0.0, dm], nfft)
    cl = CL(nfft, overlap, ntime)
    cl.set_chirp(table)
    for i_out in (step + step // 2, step + 2, 2 * step - 3):
        imp = np.zeros(n, np.complex128)
        imp[i_out + overlap // 2] = 100.0
        x = np.zeros((NCHAN, NBEAM, n), np.complex64)
        x[0, 2 * PAIR0 + 3] = disperse(imp, f_c, CHAN_BW, dm, KDM)
        rows = select(x, PAIR0, NPAIR)
        ffi.call("xengCdlongReset")
        got = cl.stream(x)
        ref = filter_blocks(rows, table, nfft, overlap)
        p, q = np.abs(got[:, 0, 3].astype(np.complex128).reshape(-1)) ** 2, np.abs(ref[:, 0, 3].reshape(-1)) ** 2
        print("impulse at %d: share %.6f, float64 %.6f" % (i_out, p.max() / p.sum(), q.max() / q.sum()))
        assert int(np.argmax(p)) == int(np.argmax(q)) == i_out
        assert abs(p.max() / p.sum() - q.max() / q.sum()) <= 1e-4
        rest = np.ones((NCHAN, NB), bool)
        rest[0, 3] = False
        assert (got[:, rest] == 0).all()
    cl.close()


# ---------------------------------------------------------------- 4., 5. bit identity
def test_bit_identical_across_call_sizes():
    """One stream through contexts of ntime 480, 1000 and L + 7 = 11831 (one whole block plus 7 samples; blocks complete inside
    calls and, with 11831, early in a call whose rest already belongs to the next block): the same blocks bit for bit."""
    rng = np.random.default_rng(23)
    n = 4 * (L + 7)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    table = unit_tables(rng, NPAIR, NCHAN, NFFT)
    nblk = 3
    outs = []
    for ntime in (480, 1000, L + 7):
        m = _length(NFFT, M, nblk, ntime)
        assert m <= n
        cl = CL(ntime=ntime)
        cl.set_chirp(table)
        got = cl.stream(x[..., :m])
        cl.close()
        assert len(got) >= nblk
        outs.append(got[:nblk].tobytes())
    assert outs[1] == outs[0] and outs[2] == outs[0]


def test_bit_identical_after_reset_and_in_a_fresh_context():
    """The same stream: from Initialize; after a Reset that follows 20000 samples of another stream (one block and a partial one,
    which must leave no trace -- the overlap copy has run); and in a fresh context."""
    n = _length(NFFT, M, 3)
    rng = np.random.default_rng(29)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    table = unit_tables(rng, NPAIR, NCHAN, NFFT)
    cl = CL()
    cl.set_chirp(table)
    outs = [cl.stream(x).tobytes()]
    ffi.call("xengCdlongReset")
    assert _info()[2:] == (0, 0)
    assert len(cl.stream(7 + x[..., 3000:23000][..., ::-1])) == 1 and _info()[2:] == (20000, 1)
    ffi.call("xengCdlongReset")
    outs.append(cl.stream(x).tobytes())
    cl.close()
    cl = CL()
    cl.set_chirp(table)
    outs.append(cl.stream(x).tobytes())
    cl.close()
    assert len(outs[0]) == nblocks_after(n, NFFT, M) * cl.unit and outs[1] == outs[0] and outs[2] == outs[0]


# ---------------------------------------------------------------- 6. a non-finite sample
def test_one_nan_takes_the_two_blocks_of_its_row_that_hold_it():
    """NFFT 2^14, M 4560: sample 25000 lies in [23648, 28208), which blocks 1 and 2 share.  A NaN there makes exactly those two
    blocks of its row NaN, every sample of them, and every other word is bit-identical to the clean run."""
    n = _length(NFFT, M, 4)
    rng = np.random.default_rng(31)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    table = unit_tables(rng, NPAIR, NCHAN, NFFT)
    cl = CL()
    cl.set_chirp(table)
    clean = cl.stream(x)
    bad = x.copy()
    bad[1, 2 * PAIR0 + 1, 25000] = np.nan
    ffi.call("xengCdlongReset")
    got = cl.stream(bad)
    cl.close()
    hit = np.zeros(got.shape[:3], bool)
    hit[1:3, 1, 1] = True
    assert len(got) == 4 and np.isnan(got[hit].real).all() and np.isnan(got[hit].imag).all()
    assert got[~hit].tobytes() == clean[~hit].tobytes() and not np.isnan(clean.view(np.float32)).any()


# ---------------------------------------------------------------- 7., 8. the ABI
def test_nblocks_info_null_output_and_set_chirp_mid_stream():
    """NFFT 2^14, M 4560, calls of 4000: nblocks is 0, 0, 0, 0, 1, 0, 0, 1 ... as the sample count says, and a call that completes
    nothing leaves its output (NULL or not) untouched.  A completing call with out_dev NULL is INVALID_ARGUMENT, enqueues nothing
    and counts nothing: the same call with an output then completes the block.  SetChirp of both pairs between two calls holds from
    the next block: blocks 0 and 1 are the first table's, blocks 2 and 3 the second's, on one stream.  A table with a non-finite
    word and a pair outside the context's are refused and change nothing."""
    n = _length(NFFT, M, 4)
    rng = np.random.default_rng(37)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    rows = select(x, PAIR0, NPAIR)
    t0, t1 = unit_tables(rng, NPAIR, NCHAN, NFFT), unit_tables(rng, NPAIR, NCHAN, NFFT)
    cl = CL()
    cl.set_chirp(t0)
    got, flags = [], []
    for k in range(n // NTIME):
        call = x[..., k * NTIME:(k + 1) * NTIME]
        want = nblocks_after((k + 1) * NTIME, NFFT, M) - nblocks_after(k * NTIME, NFFT, M)
        if k == 8:                              # (32000 samples: blocks 0 and 1 are out, block 2 needs sample 40031)
            assert _info() == (L, 1, 32000, 2)
            bad = t1.copy()
            bad[1, 1, 77] = np.inf
            for pair, tab in ((1, bad[1]), (NPAIR, t1[0])):
                with pytest.raises(ffi.XengError) as ei:
                    ffi.call("xengCdlongSetChirp", pair, _fp(tab.view(np.float32)))
                assert ei.value.status == INVALID_ARGUMENT
            cl.set_chirp(t1)
        if want:
            cl.din.upload(np.ascontiguousarray(call))
            nb = ctypes.c_int(-1)
            with pytest.raises(ffi.XengError) as ei:
                ffi.call("xengCdlongRun", cl.din.ptr, None, ctypes.byref(nb))
            assert ei.value.status == INVALID_ARGUMENT and _info()[2] == k * NTIME
            y = cl.run(call)
        else:
            nb = cl.enqueue(call, out=(k % 2 == 0))
            ffi.call("xengCdlongSync")
            y = cl.result(nb)
        assert len(y) == want
        flags.append(want)
        got.append(y)
    got = np.concatenate(got)
    cl.close()
    assert flags[:8] == [0, 0, 0, 0, 1, 0, 0, 1] and len(got) == 4
    bar = 5 * max(gaps(rows, t0, NFFT, M) + gaps(rows, t1, NFFT, M))
    assert (row_error(got[:2], filter_blocks(rows, t0, NFFT, M, count=2)) <= bar).all()
    assert (row_error(got[2:], filter_blocks(rows, t1, NFFT, M, first=2)) <= bar).all()
    assert (row_error(got[2:], filter_blocks(rows, t0, NFFT, M, first=2)) > 0.1).all()


def test_completion_tickets_and_argument_checks_with_and_without_a_context():
    """Tickets count from 1 after Initialize and every one is done after Sync; unknown tickets are errors.  Every INVALID_ARGUMENT
    of Initialize leaves a live context alone; Run refuses misaligned and null pointers with nothing launched and the count
    unchanged; after Destroy every call that needs a context is INVALID_STATE."""
    cl = CL()
    x = np.zeros((NCHAN, NBEAM, NTIME), np.complex64)
    t, d, nb = ctypes.c_ulonglong(), ctypes.c_int(-1), ctypes.c_int(-1)
    ffi.call("xengCdlongMark", ctypes.byref(t))
    assert t.value == 1
    cl.enqueue(x)
    ffi.call("xengCdlongMark", ctypes.byref(t))
    assert t.value == 2
    ffi.call("xengCdlongWait", 2)
    ffi.call("xengCdlongSync")
    for k in (1, 2):
        ffi.call("xengCdlongTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, 3):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdlongWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, NBEAM, NTIME, 0, 1, NFFT, M), (0, NCHAN, NBEAM, NTIME, 3, 1, NFFT, M), (0, NCHAN, NBEAM, NTIME, 0, 1, 3 << 13, M),
                 (0, NCHAN, NBEAM, NTIME, 0, 1, NFFT, M + 1), (0, NCHAN, NBEAM, NTIME, 0, 1, NFFT, NFFT // 2 + 2), (0, NCHAN, NBEAM, NTIME, 0, 1, 1 << 13, 0),
                 (0, NCHAN, NBEAM, NTIME, 0, 1, 1 << 21, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdlongInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info() == (L, 1, NTIME, 0)
    for args in ((None, cl.dout.ptr + GUARD, ctypes.byref(nb)), (cl.din.ptr, cl.dout.ptr + GUARD, None), (cl.din.ptr + 8, cl.dout.ptr + GUARD, ctypes.byref(nb)),
                 (cl.din.ptr, cl.dout.ptr + GUARD + 8, ctypes.byref(nb))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdlongRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengCdlongSync")
    assert _info() == (L, 1, NTIME, 0) and len(cl.result(0)) == 0
    cl.close()
    s, n = ctypes.c_int(), ctypes.c_longlong()
    f = np.zeros(4, np.float32)
    for name, args in (("xengCdlongRun", (cl.din.ptr or 4096, 4096, ctypes.byref(nb))), ("xengCdlongReset", ()), ("xengCdlongSetChirp", (0, _fp(f))),
                       ("xengCdlongGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), ctypes.byref(n))), ("xengCdlongMark", (ctypes.byref(t),)),
                       ("xengCdlongWait", (1,)), ("xengCdlongTicketDone", (1, ctypes.byref(d))), ("xengCdlongSync", ()),
                       ("xengCdlongCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCdlongDestroy")


# ---------------------------------------------------------------- 9. the blocks on device rings
def _voltage_header(nchan, nbeam, seq0, sfreq):
    hdr = source_header(nchan, nbeam, 1, seq0=seq0, sfreq=sfreq, chan_bw=CHAN_BW)
    hdr.update(nbeam=nbeam, nstand=nbeam, npol=1, nbit=32, complex=True)
    return hdr


def _ring_bytes(v, g):
    return np.concatenate([np.ascontiguousarray(v[..., k * g:(k + 1) * g]).reshape(-1) for k in range(v.shape[-1] // g)])


def test_blocks_dedisperse_then_upchannelise_on_device_rings():
    """Source -> BeamCoherentDedisperseLong (planned: multiple_of 8) -> UpchanSumBeams (nupchan 8) on device rings, 25 MHz, DMs 4
    and 10 (sweeps of 1216 and 3040 samples at the lowest channel): the plan is (2^14, 4560); every span of the dedisperser is, bit
    for bit, the block xengCdlongRun writes for the same samples through the C ABI (which the tests above hold to the bar); its
    header says pairs, DMs and plan, and seq0 = the input's + M/2; the upchanneliser accepts it and writes, per span, the float64
    restatement of ITS contract applied to the float64 blocks (rtol 1e-4 of the span's largest power: two fp32 stages)."""
    nup, seq0, sfreq, dms, g = 8, 5000, 25e6, [4.0, 10.0], NTIME
    nfft, overlap = cdedisp_plan_long(_freqs(sfreq), CHAN_BW, 10.0, nup)
    assert (nfft, overlap) == (NFFT, M)
    n = _length(nfft, overlap, 3, g)
    rng = np.random.default_rng(41)
    x = gaussian_rows(rng, NCHAN, NBEAM, n)
    hdr = _voltage_header(NCHAN, NBEAM, seq0, sfreq)
    r0, r1, r2 = Ring("bf-output", space="cuda"), Ring("cd-output", space="cuda"), Ring("ub-output", space="cuda")
    cd = BeamCoherentDedisperseLong(LOG, r0, r1, NCHAN, NBEAM, g, dms, pair0=PAIR0, npair=NPAIR, multiple_of=nup, gpu=0)
    ub = UpchanSumBeams(LOG, r1, r2, nchan=NCHAN, nbeam=NB, ntime_gulp=L, nupchan=nup, nframe_sum=L // nup, gpu=0)
    mid, sink = Sink(r1, NCHAN * NB * L * 8), Sink(r2, NPAIR * NCHAN * nup * 16)
    run_blocks([cd, ub], Source(r0, [(hdr, _ring_bytes(x, g), NCHAN * NBEAM * g * 8)]), [mid, sink])
    ffi.call("xengCdlongDestroy")
    (ch, ctag, cspans), = mid.sequences
    (uh, utag, uspans), = sink.sequences
    nblk = nblocks_after(n, nfft, overlap)
    assert len(cspans) == len(uspans) == nblk >= 3 and ctag == ch['seq0'] == utag == uh['seq0'] == seq0 + overlap // 2
    assert (ch['nbeam'], ch['nstand'], ch['pair0'], ch['cdedisp_dm'], ch['cdedisp_nfft'], ch['cdedisp_overlap']) == (NB, NB, PAIR0, dms, nfft, overlap)
    assert uh['cdedisp_dm'] == dms and uh['nupchan'] == nup and uh['pair0'] == 0 and not {'acc_len', 'ntime_sum', 'nupchan'} & set(ch)
    table = chirp_table(_freqs(sfreq), CHAN_BW, dms, nfft)
    cl = CL()
    cl.set_chirp(table)
    abi = cl.stream(x)
    cl.close()
    got = np.array([s.view(np.complex64).reshape(NCHAN, NB, L) for s in cspans])
    assert got.tobytes() == abi.tobytes()
    ref = filter_blocks(select(x, PAIR0, NPAIR), table, nfft, overlap)
    for j, s in enumerate(uspans):
        exp = upchan_sum_beams(ref[j], nup, L // nup, 0, L)
        assert np.allclose(s.view(np.float32).reshape(exp.shape), exp, rtol=0, atol=1e-4 * np.abs(exp).max())
    assert cd.stats['nblock'] == nblk and cd.stats['ndropped'] == 0
