"""BeamDetrend on the MI355X: xengDetrend* against the restatement (tests/detrend_ref.py), byte for byte and with no tolerance: the
output of every call and M, A and the valid bytes of every decided block.  Integer data against float64 arithmetic
(blocks/detrend.py detrend_reference) in three splits; float data at the smallest and the largest block, at a block that is no power
of two and with a ring that wraps; the fall-backs (a NaN, infinities, a constant series, heavy ties); bit identity across splits and
after a Reset against a fresh context; the ABI's refusals; and xengDedispRun -> xengDetrendRun -> xengPulseRun on the device.  The
output sits between poisoned guard bands that are checked after every call, the input is read back after every call and must be
what was uploaded, the state's guards are checked at every close.  No wall-clock assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import detrend_reference  # noqa: E402
from tests import detrend_cases, detrend_ref  # noqa: E402
from tests.dedisp_ref import dedisperse  # noqa: E402
from tests.pulse_ref import pulse_search  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
K_MAD = detrend_cases.K_MAD
_pf, _pu8 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)
RECORD = np.dtype([('snr', '<f4'), ('n', '<i4'), ('iw', '<i4'), ('B', '<f4')])


def _info():
    n, k = ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengDetrendGetInfo", ctypes.byref(n), ctypes.byref(k))
    return n.value, k.value


class DT:
    """The xengDetrend context (one per process), an input buffer, the output between poisoned guard bands, and the restatement
    beside it: every call goes to both and is compared byte for byte, and so are the knots of every block decided."""

    def __init__(self, npair, ndm, nwin, nprod, nblk, normalise):
        self.npair, self.ndm, self.nwin, self.nprod, self.nblk = npair, ndm, nwin, nprod, nblk
        self.nser = npair * ndm
        # the buffers come first, the context second: tests/test_accel_gpu.py says why
        self.din = ffi.DeviceBuffer(nwin * self.nser * nprod * 4)
        self.dout = ffi.DeviceBuffer(2 * GUARD + nwin * self.nser * 4)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        ffi.call("xengDetrendInitialize", 0, npair, ndm, nwin, nprod, nblk, normalise, K_MAD)
        self.ref = detrend_ref.DetrendRef(self.nser, nblk, normalise, K_MAD, nprod)
        self.knots = []

    def reset(self):
        ffi.call("xengDetrendReset")
        self.ref.reset()
        assert _info() == (0, 0)

    def get_knots(self):
        M, A = (np.empty(self.nser, np.float32) for _ in range(2))
        v = np.empty(self.nser, np.uint8)
        ffi.call("xengDetrendGetKnots", M.ctypes.data_as(_pf), A.ctypes.data_as(_pf), v.ctypes.data_as(_pu8))
        return M, A, v

    def run(self, x):
        nc = x.shape[0]
        sent = np.ascontiguousarray(x, np.float32).reshape(nc, self.nser, self.nprod)
        self.din.upload(sent)
        done = ctypes.c_int(-1)
        ffi.call("xengDetrendRun", self.din.ptr, nc, self.dout.ptr + GUARD, ctypes.byref(done))
        ffi.call("xengDetrendSync")
        assert self.din.download(np.uint8, sent.nbytes).tobytes() == sent.tobytes(), "the input was written"
        raw = self.dout.download(np.uint8)
        per = self.nser * 4
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + nc * per:] == POISON).all(), "bytes past the call's windows were written"
        out = raw[GUARD:GUARD + nc * per].copy().view(np.float32).reshape(nc, self.nser)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        before = self.ref.nblocks
        exp = self.ref.run(sent)
        assert done.value == int(self.ref.nblocks > before)
        if done.value:
            got = self.get_knots()
            for name, a, b in zip(("M", "A", "valid"), got, self.ref.newest):
                assert a.tobytes() == b.tobytes(), "%s of block %d differs at series %r" % (name, before, np.flatnonzero(a.view(np.uint8) != b.view(np.uint8))[:5] // a.itemsize)
            self.knots.append(got)
        bad = np.argwhere(out.view(np.uint32) != exp.view(np.uint32))
        assert bad.size == 0, "out differs at (window, series) %r: %r / %r" % (bad[:5].tolist(), out[tuple(bad[0])], exp[tuple(bad[0])])
        return out

    def stream(self, x, sizes):
        outs, n = [], 0
        for nc in sizes:
            outs.append(self.run(x[n:n + nc]))
            n += nc
        assert n == x.shape[0] and _info() == (self.ref.n, self.ref.nblocks)
        return np.concatenate(outs)

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengDetrendCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengDetrendDestroy")
        self.din.free()
        self.dout.free()


@pytest.mark.parametrize("nprod", [1, 4])
def test_integer_data_equal_float64_arithmetic_in_every_split(nprod):
    """3 x 37 = 111 series (no multiple of 32 or 64), nblk 64, not normalised, 640 windows in calls of 64, of 1 and of 1..30: every
    word equals the float64 statement (every median, difference and product is exact in both), and so do M and A of every block."""
    npair, ndm, nblk, total = 3, 37, 64, 640
    D = 96
    x = detrend_cases.integer_scene(7 + nprod, total, npair, ndm, nprod)
    z = detrend_ref.series(x, nprod)
    y64, M64, A64, v64 = detrend_reference(z, nblk, normalise=False)
    first = None
    for sizes in (detrend_cases.whole(total, 64), [1] * total, detrend_cases.random_sizes(11, total, 30)):
        dt = DT(npair, ndm, 64, nprod, nblk, 0)
        try:
            out = dt.stream(x, sizes)
            assert np.array_equal(out[D:].astype(np.float64), y64[:total - D]) and not out[:D].any() and out[D:].any()
            assert len(dt.knots) == 10 and v64.all()
            for k, (M, A, v) in enumerate(dt.knots):
                assert np.array_equal(M.astype(np.float64), M64[k]) and np.array_equal(A.astype(np.float64), A64[k]) and v.all()
            first = first if first is not None else out.tobytes()
            assert out.tobytes() == first
        finally:
            dt.close()


@pytest.mark.parametrize("normalise", [0, 1])
@pytest.mark.parametrize("npair,ndm,nblk,nwin,total", [(1, 7, 4, 4, 60), (2, 35, 30, 15, 240), (3, 37, 1024, 512, 3 * 1024 + 40), (1, 5, 8192, 4096, 2 * 8192 + 4200)],
                         ids=["nblk4", "nblk30", "nblk1024", "nblk8192"])
def test_float_data_equal_the_restatement_byte_for_byte(npair, ndm, nblk, nwin, total, normalise):
    """The smallest block (a ring of 10 slots wraps six times, the knot slots are taken fifteen times); nblk 30 in spans of 15 (u is
    no dyadic fraction, 70 series: ragged tiles); nblk 1024; nblk 8192 with 5 series (32 KiB of keys).  nprod 4 where normalised.
    The scenes carry the constant series, the series of two values, the NaN of block 2 and the infinities."""
    nprod = 4 if normalise else 1
    x = detrend_cases.float_scene(100 + nblk, total, npair, ndm, nprod, nblk)
    sizes = detrend_cases.whole(total, nwin) if nblk > 30 else detrend_cases.random_sizes(nblk, total, nwin)
    dt = DT(npair, ndm, nwin, nprod, nblk, normalise)
    try:
        out = dt.stream(x, sizes)
        D = 3 * nblk // 2
        assert not out[:D].any() and out[D:, 0].all() and len(dt.knots) == total // nblk
    finally:
        dt.close()


def test_fall_backs_a_nan_a_constant_series_and_heavy_ties():
    """nblk 16, normalised, 7 series x 96 windows.  Series 3 has a NaN in block 2: knot 2 is not valid, its neighbours stand in, and
    the NaN's own window reads +0.  Series 1 is constant: A = 0, no knot is ever valid, the output is all +0.  Series 2 has two
    values, -0 and +0 among them.  All equal the restatement (DT.run compares)."""
    nblk, total = 16, 96
    x = detrend_cases.float_scene(9, total, 1, 7, 1, nblk)
    dt = DT(1, 7, 8, 1, nblk, 1)
    try:
        out = dt.stream(x, detrend_cases.whole(total, 8))
        valid = np.stack([k[2] for k in dt.knots])
        assert valid[:, 0].all() and not valid[:, 1].any() and valid[:, 3].tolist() == [1, 1, 0, 1, 1, 1] and not valid[1, 4] and not valid[3, 4]
        assert not out[:, 1].any() and all(k[1][1] == 0 for k in dt.knots)
        at = 2 * nblk + nblk // 3 + 24
        assert out[at, 3] == 0 and out[at - 1, 3] != 0 and out[at + 1, 3] != 0 and np.isfinite(out).all()
    finally:
        dt.close()


def test_splits_merge_to_the_same_bytes_and_a_reset_is_a_fresh_context():
    """nblk 30, 70 series, 150 windows: one call per block, 30 x 1 per block and random sizes give the same bytes; after a prefix and a
    Reset the run equals a fresh context's; the guards are intact (DT.close), the input is unchanged after every call (DT.run)."""
    npair, ndm, nblk, total = 2, 35, 30, 150
    x = detrend_cases.float_scene(31, total, npair, ndm, 4, nblk)
    runs = []
    for sizes in (detrend_cases.whole(total, 30), [1] * total, detrend_cases.random_sizes(3, total, 30)):
        dt = DT(npair, ndm, 30, 4, nblk, 1)
        try:
            runs.append(dt.stream(x, sizes).tobytes())
        finally:
            dt.close()
    assert runs[0] == runs[1] == runs[2]
    dt = DT(npair, ndm, 30, 4, nblk, 1)
    try:
        dt.stream(detrend_cases.float_scene(32, 47, npair, ndm, 4, nblk), detrend_cases.whole(47, 30))
        dt.reset()
        assert dt.stream(x, detrend_cases.random_sizes(4, total, 30)).tobytes() == runs[0]
    finally:
        dt.close()


def test_refusals_touch_no_device():
    L = ffi.lib()
    good = dict(npair=2, ndm=8, nwin=4, nprod=1, nblk=8, normalise=1, k_mad=1.0)

    def init(**kw):
        a = dict(good, **kw)
        return L.xengDetrendInitialize(0, a['npair'], a['ndm'], a['nwin'], a['nprod'], a['nblk'], a['normalise'], ctypes.c_float(a['k_mad']))

    L.xengDetrendDestroy()
    for kw in (dict(nblk=7), dict(nblk=2), dict(nblk=8194), dict(nwin=9), dict(nwin=0), dict(k_mad=float('nan')), dict(k_mad=0.0), dict(k_mad=-1.0),
               dict(k_mad=float('inf')), dict(nprod=2), dict(normalise=2), dict(npair=0), dict(npair=4097, ndm=4096),
               dict(npair=4096, ndm=4096, nblk=40, nwin=4)):        # (64 windows of 2^24 series: exactly 2^32 bytes, not below the cap)
        assert init(**kw) == INVALID_ARGUMENT, kw
    assert b"history" in L.xengGetLastError()
    n = ctypes.c_longlong()
    done = ctypes.c_int(-7)
    assert L.xengDetrendGetInfo(ctypes.byref(n), ctypes.byref(n)) == INVALID_STATE              # (no refusal above left a context)
    assert L.xengDetrendRun(16, 1, 16, ctypes.byref(done)) == INVALID_STATE
    assert init() == 0
    try:
        buf = ffi.DeviceBuffer(4096)
        M = np.empty(16, np.float32)
        v = np.empty(16, np.uint8)
        assert L.xengDetrendGetKnots(M.ctypes.data_as(_pf), M.ctypes.data_as(_pf), v.ctypes.data_as(_pu8)) == INVALID_STATE
        for args in ((None, 1, buf.ptr, ctypes.byref(done)), (buf.ptr, 1, None, ctypes.byref(done)), (buf.ptr, 1, buf.ptr, None),
                     (buf.ptr + 4, 1, buf.ptr, ctypes.byref(done)), (buf.ptr, 1, buf.ptr + 8, ctypes.byref(done)), (buf.ptr, 0, buf.ptr, ctypes.byref(done)),
                     (buf.ptr, 5, buf.ptr, ctypes.byref(done))):
            assert L.xengDetrendRun(*args) == INVALID_ARGUMENT
        assert _info() == (0, 0) and done.value == -7
        buf.free()
    finally:
        ffi.call("xengDetrendDestroy")


def test_dedisperse_detrend_and_search_on_the_device():
    """2 pairs x 8 trials x 64 channels, integer power beams with a step in the level and a planted pulse: xengDedispRun writes a
    device buffer, xengDetrendRun reads that buffer and writes another, xengPulseRun reads that one.  The dedispersed planes equal
    the integer sums, the detrended ones the restatement byte for byte, and the pulse records the float32 restatement of the search
    on them: n, iw and B exactly, snr to 2^-22 (its scale g is a square root and a division, each correctly rounded in both)."""
    npair, ndm, nfine, nwin, nblk, nwidth, nstat = 2, 8, 64, 16, 32, 4, 32
    total = 16 * nwin
    rng = np.random.default_rng(5)
    delays = (np.arange(ndm)[:, None] * np.arange(nfine)[None, ::-1] // 16).astype(np.int32)
    S = int(delays.max())
    x = rng.integers(0, 20, (total, npair, nfine, 4)).astype(np.float32)
    x[100:, :, :, 0] += 7
    for q in range(nfine):
        x[120 + delays[5, q], 1, q, 0] += 40
    y = dedisperse(x, delays, nprod=1, dtype=np.float64).astype(np.float32)
    ref = detrend_ref.DetrendRef(npair * ndm, nblk, 1, K_MAD, 1)
    din = ffi.DeviceBuffer(nwin * npair * nfine * 16)
    dy = ffi.DeviceBuffer(nwin * npair * ndm * 4)
    dz = ffi.DeviceBuffer(nwin * npair * ndm * 4)
    drec = ffi.DeviceBuffer(npair * ndm * 16)
    ffi.call("xengDedispInitialize", 0, npair, nfine, nwin, ndm, S, 1)
    ffi.call("xengDedispSetDelays", np.ascontiguousarray(delays).ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    ffi.call("xengDetrendInitialize", 0, npair, ndm, nwin, 1, nblk, 1, K_MAD)
    ffi.call("xengPulseInitialize", 0, npair, ndm, nwin, 1, nwidth, nstat)
    try:
        zs, recs = [], []
        done = ctypes.c_int()
        for j in range(total // nwin):
            din.upload(np.ascontiguousarray(x[j * nwin:(j + 1) * nwin]))
            ffi.call("xengDedispRun", din.ptr, nwin, dy.ptr)
            ffi.call("xengDetrendRun", dy.ptr, nwin, dz.ptr, ctypes.byref(done))
            ffi.call("xengPulseRun", dz.ptr, nwin, drec.ptr)
            ffi.call("xengPulseSync")
            assert dy.download(np.float32).tobytes() == y[j * nwin:(j + 1) * nwin].tobytes()
            z = ref.run(y[j * nwin:(j + 1) * nwin])
            assert dz.download(np.float32).tobytes() == z.tobytes(), j
            zs.append(z)
            recs.append(drec.download(np.uint8).view(RECORD).copy())
        exp = pulse_search(np.concatenate(zs), nstat, nwidth, np.float32, [nwin] * (total // nwin))['records']
        scored = 0
        for got, e in zip(recs, exp):
            assert np.array_equal(got['n'], e['n'].reshape(-1)) and np.array_equal(got['iw'], e['iw'].reshape(-1))
            assert got['B'].tobytes() == e['B'].reshape(-1).astype(np.float32).tobytes()
            assert (np.abs(got['snr'] - e['snr'].reshape(-1)) <= np.abs(e['snr'].reshape(-1)) * 2.0 ** -22).all()
            scored += int((got['n'] >= 0).sum())
        assert scored > 0
        best = max((r['snr'][ndm + 5], j) for j, r in enumerate(recs))
        assert best[0] > 6 and best[1] == (120 + S + 48) // nwin                # the pulse, D = 48 windows late, in its own trial
    finally:
        for name in ("Pulse", "Detrend", "Dedisp"):
            ffi.call("xeng%sDestroy" % name)
        for b in (din, dy, dz, drec):
            b.free()
