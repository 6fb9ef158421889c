"""UpchanImageSearch on the MI355X: xengImsearch* against the restatement (tests/imsearch_ref.py).  Every run is 64 integrations with
S = 12 and nstat = 16, so the U ring wraps four times and the Z ring more often.  Word for word on integer data (npix 37, 70 and
300: ragged rows, rows that are not 16-byte aligned, more than one tile; ndm 1, 5 and 7: fewer than four waves' worth and not a
multiple of 4; nwidth 1, 3 and 5; 5, 9 and 19 groups: one, two and three chunks of loads); the sub-list invariant; Reset and SetDelays against a
fresh context; SetWeights mid-run; float data against the float64 restatement; NaN and constant words; beside an X-engine
contraction and xengBeamformRun; refusals and tickets; and the block on device rings behind a source and behind UpchanImage.  Every
call's plane sits between two poisoned guard bands of its own, all checked after the run; the state's guards at every close.  No
wall-clock assertions."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from tests.imsearch_ref import RECORD, imsearch, integer_case, planted_case, ramp_delays, records  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
NONE_BYTES = np.array([(0.0, -1, -1)], RECORD).tobytes()
NINT, NSTAT, S = 64, 16, 12
W5 = np.array([1, 1, 0, 2, 1], np.float32)
W9 = np.array([1, 2, 1, 0, 1, 1, 3, 1, 1], np.float32)
W19 = np.array([1, 2, 1, 0, 1, 1, 3, 1, 1, 1, 1, 0, 2, 1, 1, 1, 1, 2, 1], np.float32)     # 17 in use: three chunks of loads


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    n, s = ctypes.c_longlong(), ctypes.c_int()
    ffi.call("xengImsearchGetInfo", ctypes.byref(n), ctypes.byref(s))
    return n.value, s.value


class IS:
    """The xengImsearch context (one per process), the images of a run on the device and one output plane per call, each between
    two poisoned guard bands."""

    def __init__(self, npix, ngroup, ndm, nwidth, nstat=NSTAT, max_delay=S, delays=None, weights=None):
        self.npix, self.ngroup, self.ndm, self.nwidth, self.nstat = npix, ngroup, ndm, nwidth, nstat
        ffi.call("xengImsearchInitialize", 0, npix, ngroup, ndm, max_delay, nwidth, nstat)
        self.image_bytes = ngroup * 4 * npix * 4
        self.stride = GUARD + (npix * 8 + 15) // 16 * 16
        self.din = self.dout = None
        if weights is not None:
            self.set_weights(weights)
        if delays is not None:
            self.set_delays(delays)

    def set_delays(self, delays):
        d = np.ascontiguousarray(delays, np.int32)
        assert d.shape == (self.ndm, self.ngroup)
        ffi.call("xengImsearchSetDelays", d.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def set_weights(self, w):
        w = np.ascontiguousarray(w, np.float32)
        assert w.shape == (self.ngroup,)
        ffi.call("xengImsearchSetWeights", _fp(w))

    def enqueue(self, x, each=None):
        """One Run per integration of x [n][ngroup][4][npix]; each(k) is called before integration k is enqueued."""
        n = x.shape[0]
        assert x.shape == (n, self.ngroup, 4, self.npix)
        self.din = ffi.DeviceBuffer(n * self.image_bytes).upload(np.ascontiguousarray(x, np.float32))
        self.dout = ffi.DeviceBuffer(n * self.stride + GUARD)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        for k in range(n):
            if each is not None:
                each(k)
            ffi.call("xengImsearchRun", self.din.ptr + k * self.image_bytes, self.dout.ptr + k * self.stride + GUARD)
        self.n = n

    def result(self):
        """After a sync: the planes [n][npix]; every byte between and around them must still be poison."""
        raw = self.dout.download(np.uint8)
        nb = self.npix * 8
        planes = np.empty((self.n, self.npix), RECORD)
        for k in range(self.n):
            a = k * self.stride
            assert (raw[a:a + GUARD] == POISON).all(), "bytes before the plane of call %d were written" % k
            planes[k] = raw[a + GUARD:a + GUARD + nb].copy().view(RECORD)
            assert (raw[a + GUARD + nb:a + self.stride] == POISON).all(), "bytes past the plane of call %d were written" % k
        assert (raw[self.n * self.stride:] == POISON).all()
        return planes

    def run(self, x, each=None):
        self.enqueue(x, each)
        ffi.call("xengImsearchSync")
        return self.result()

    def baseline(self):
        out = [np.empty((self.ngroup, self.npix), np.float32) for _ in range(3)]
        ffi.call("xengImsearchGetBaseline", *[_fp(a) for a in out])
        return out

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengImsearchCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengImsearchDestroy")


def ref_planes(ref):
    return np.stack([records(ref, n) for n in range(ref['snr'].shape[0])])


# ---------------------------------------------------------------- 1. word for word on integer data
INT_CASES = {
    # npix, ngroup, ndm, nwidth
    "37 pixels, 5 trials, 3 widths": (37, 5, 5, 3),
    "70 pixels, 7 trials, 3 widths, 9 groups": (70, 9, 7, 3),
    "300 pixels, 1 trial, 1 width": (300, 5, 1, 1),
    "300 pixels, 7 trials, 3 widths": (300, 5, 7, 3),
    "37 pixels, 1 trial, 3 widths": (37, 5, 1, 3),
    "72 pixels (aligned rows), 5 trials, 1 width": (72, 5, 5, 1),
    "37 pixels, 5 trials, 5 widths, 19 groups": (37, 19, 5, 5),
}


@functools.lru_cache(maxsize=None)
def int_case(name):
    npix, ngroup, ndm, nwidth = INT_CASES[name]
    x, delays = integer_case(npix, ngroup, ndm, NINT, seed=sorted(INT_CASES).index(name))
    w = {5: W5, 9: W9, 19: W19}[ngroup]
    assert delays.max() == S and delays.min() == 0
    return x, delays, w, imsearch(x, delays, w, NSTAT, nwidth, np.float32)


@pytest.mark.parametrize("case", sorted(INT_CASES))
def test_integer_data_match_the_restatement_word_for_word(case):
    """Every call's plane equals the float32 restatement's word for word; GetBaseline is refused before the first block is complete
    and equals the restatement's c, m, v of the last complete block after 16, 17, 32 and 64 integrations."""
    npix, ngroup, ndm, nwidth = INT_CASES[case]
    x, delays, w, ref = int_case(case)
    ctx = IS(npix, ngroup, ndm, nwidth, delays=delays, weights=w)
    assert _info() == (0, S)
    got = []
    for a, b in ((0, 15), (15, 16), (16, 17), (17, 32), (32, 64)):
        got.append(ctx.run(x[a:b]))
        assert _info() == (b, S)
        if b < NSTAT:
            with pytest.raises(ffi.XengError) as ei:
                ctx.baseline()
            assert ei.value.status == INVALID_STATE
        else:
            for g, f in zip(ctx.baseline(), "cmv"):
                assert g.tobytes() == ref[f][b // NSTAT - 1].astype(np.float32).tobytes(), (case, b, f)
    ctx.close()
    got = np.concatenate(got)
    exp = ref_planes(ref)
    for n in range(NINT):
        assert got[n].tobytes() == exp[n].tobytes(), (case, n)
    assert (got[:NSTAT + S]['idm'] == -1).all() and (got[NSTAT + S + (1 << (nwidth - 1)):]['idm'] >= 0).all()


def test_planted_pulse_is_recovered():
    """The planted dispersed box pulse of tests/test_imsearch_cpu.py: word for word, and the best record of its plane."""
    x, delays, w, (n, pix, idm, iw) = planted_case()
    ctx = IS(70, 5, 4, 3, delays=delays, weights=w)
    got = ctx.run(x)
    ctx.close()
    assert got.tobytes() == ref_planes(imsearch(x, delays, w, NSTAT, 3, np.float32)).tobytes()
    assert (got[n]['idm'][pix], got[n]['iw'][pix]) == (idm, iw) and got[n]['snr'].argmax() == pix and got[n]['snr'][pix] > 15


# ---------------------------------------------------------------- float data, shared
@functools.lru_cache(maxsize=None)
def float_case(npix=300, ngroup=5, ndm=7):
    """XX and YY each N(1000, 15) per word, NaN in words 2 and 3."""
    rng = np.random.default_rng(5)
    x = np.full((NINT, ngroup, 4, npix), np.nan, np.float32)
    x[:, :, :2] = rng.normal(1000.0, 15.0, (NINT, ngroup, 2, npix)).astype(np.float32)
    return x, ramp_delays(ndm, ngroup, S)


@functools.lru_cache(maxsize=None)
def float_run():
    """The stand-alone run of float_case: 300 pixels, 7 trials, 3 widths."""
    x, delays = float_case()
    ctx = IS(300, 5, 7, 3, delays=delays, weights=W5)
    got = ctx.run(x)
    ctx.close()
    return got


# ---------------------------------------------------------------- 2. the sub-list invariant
def test_a_sub_list_of_pixels_gives_those_pixels_records_bit_for_bit():
    """37 scattered pixels of the 300, run as a list of their own (ragged rows, another place in the tile, another pitch): their
    records are those of the full run bit for bit."""
    x, delays = float_case()
    full = float_run()
    pick = np.sort(np.random.default_rng(8).choice(300, 37, replace=False))
    assert pick[-1] >= 256 and (np.diff(pick) > 1).any()
    ctx = IS(37, 5, 7, 3, delays=delays, weights=W5)
    sub = ctx.run(np.ascontiguousarray(x[..., pick]))
    ctx.close()
    assert sub.tobytes() == np.ascontiguousarray(full[:, pick]).tobytes()
    assert (sub[NSTAT + S + 4:]['idm'] >= 0).all()


# ---------------------------------------------------------------- 3. Reset and SetDelays
def test_reset_and_set_delays_against_a_fresh_context():
    """After 23 integrations of other data (the state, both rings and the counters somewhere else) a Reset, and after 9 more a
    SetDelays of the same table, each followed by the run: bit-identical to the fresh context's."""
    x, delays = float_case()
    fresh = float_run()
    other = np.ascontiguousarray(x[::-1] * np.float32(0.5))
    ctx = IS(300, 5, 7, 3, delays=delays, weights=W5)
    ctx.run(other[:23])
    ffi.call("xengImsearchReset")
    assert _info() == (0, S)
    a = ctx.run(x)
    ctx.run(other[:9])
    ctx.set_delays(delays)
    assert _info() == (0, S)
    b = ctx.run(x)
    ctx.set_delays(delays // 2)                     # (another S: the slots of the U ring move)
    assert _info() == (0, S // 2)
    c = ctx.run(x)
    ctx.close()
    assert a.tobytes() == fresh.tobytes() and b.tobytes() == fresh.tobytes()
    ctx = IS(300, 5, 7, 3, delays=delays // 2, weights=W5)
    c0 = ctx.run(x)
    ctx.close()
    assert c.tobytes() == c0.tobytes() and c.tobytes() != fresh.tobytes()


# ---------------------------------------------------------------- 4. SetWeights mid-run
def test_set_weights_mid_run():
    """Weights set again after 40 integrations (another set of groups left out): the planes equal the restatement's word for word,
    and no boxcar that reaches before integration 40 is scored -- width 1 alone at 40, at most 2 at 41 and 42."""
    x, delays = integer_case(70, 9, 5, NINT, seed=3)
    w1 = np.array([1, 1, 0, 1, 2, 1, 1, 0, 1], np.float32)
    ctx = IS(70, 9, 5, 3, delays=delays, weights=W9)
    got = ctx.run(x, each=lambda k: ctx.set_weights(w1) if k == 40 else None)
    assert _info() == (NINT, S)
    ctx.close()
    ref = imsearch(x, delays, [(0, W9), (40, w1)], NSTAT, 3, np.float32)
    assert got.tobytes() == ref_planes(ref).tobytes()
    assert (got[40]['idm'] >= 0).all() and got[40]['iw'].max() == 0 and got[41]['iw'].max() <= 1 and got[42]['iw'].max() <= 1
    assert got[39]['iw'].max() == 2 and got[43:]['iw'].max() == 2


# ---------------------------------------------------------------- 5. float data
def test_float_data_within_the_bar_of_the_float64_restatement():
    """XX, YY ~ N(1000, 15), 300 pixels, 7 trials, 3 widths.  The bar is five times the float32-to-float64 gap of the restatement on
    these inputs, relative to max(1, |snr|).  Measured: gap 1.3e-5, bar 6.5e-5, the GPU's worst record 1.23e-5 = 0.19 of the bar; 0.07 % of
    the 10 800 records have a thin margin.  Every record is scored exactly where the float64
    restatement scores; its snr is within the bar of the float64 score at its own (idm, iw); (idm, iw) equal the float64
    restatement's wherever its margin between best and runner-up is at least twice the bar, and at most 2 % of the records have a
    thinner margin (there the record's key must still score within twice the bar of the best)."""
    x, delays = float_case()
    got = float_run()
    r64 = imsearch(x, delays, W5, NSTAT, 3, np.float64)
    r32 = imsearch(x, delays, W5, NSTAT, 3, np.float32)
    both = r64['scored'] & r32['scored']
    assert both.any() and np.array_equal(r64['scored'], r32['scored'])
    gap = float((np.abs(r32['score'][both].astype(np.float64) - r64['score'][both]) / np.maximum(1.0, np.abs(r64['score'][both]))).max())
    bar = 5 * gap
    assert 0 < gap < 1e-4
    nint, ndm, nwidth, npix = r64['score'].shape
    flat = np.where(r64['scored'], r64['score'], -np.inf).reshape(nint, ndm * nwidth, npix)
    anyref = r64['scored'].any(axis=(1, 2))
    assert np.array_equal(got['idm'] >= 0, anyref)
    assert got[~anyref].tobytes() == NONE_BYTES * int((~anyref).sum())
    srt = np.sort(flat, axis=1)
    top, second = srt[:, -1], srt[:, -2]
    n_i, p_i = np.nonzero(anyref)
    gi, gw = got['idm'][n_i, p_i].astype(int), got['iw'][n_i, p_i].astype(int)
    assert (gi < ndm).all() and (gw < nwidth).all() and r64['scored'][n_i, gi, gw, p_i].all()
    at = r64['score'][n_i, gi, gw, p_i]
    t, s2 = top[n_i, p_i], second[n_i, p_i]
    scale = np.maximum(1.0, np.abs(t))
    err = np.abs(got['snr'][n_i, p_i].astype(np.float64) - at) / np.maximum(1.0, np.abs(at))
    wide = (t - s2) >= 2 * bar * scale
    print("imsearch float: float32 gap %.3g, bar %.3g, GPU worst %.3g = %.2f of the bar; %.2f %% of %d records with a thin margin"
          % (gap, bar, err.max(), err.max() / bar, 100.0 * (~wide).mean(), wide.size))
    assert (err <= bar).all()
    assert (gi[wide] == r64['idm'][n_i, p_i][wide]).all() and (gw[wide] == r64['iw'][n_i, p_i][wide]).all()
    assert (~wide).mean() <= 0.02
    assert (t - at <= 2 * bar * scale).all()


# ---------------------------------------------------------------- 6. flags
def test_nan_and_constant_words():
    """96 integrations of the float data, 70 pixels.  NaN filling the weight-0 group changes no byte.  A pixel constant in one used
    group (v = 0) reads {0, -1, -1} throughout.  A NaN in one used word (integration 36, group 1, pixel 41) un-scores exactly the
    records of that pixel whose sums reach it or the blocks it spoils -- the float32 restatement's records, with stretches without a
    record and scored ones after -- and changes no byte of any other pixel."""
    rng = np.random.default_rng(12)
    npix, ngroup, ndm = 70, 5, 5
    x = np.full((96, ngroup, 4, npix), np.nan, np.float32)
    x[:, :, :2] = rng.normal(1000.0, 15.0, (96, ngroup, 2, npix)).astype(np.float32)
    delays = ramp_delays(ndm, ngroup, S)
    ctx = IS(npix, ngroup, ndm, 3, delays=delays, weights=W5)
    clean = ctx.run(x)
    y = x.copy()
    y[:, 2] = np.nan
    ffi.call("xengImsearchReset")
    assert ctx.run(y).tobytes() == clean.tobytes()
    y = x.copy()
    y[:, 3, :2, 17] = 321.0
    y[36, 1, 1, 41] = np.nan
    ffi.call("xengImsearchReset")
    bad = ctx.run(y)
    ctx.close()
    others = np.ones(npix, bool)
    others[[17, 41]] = False
    assert np.ascontiguousarray(bad[:, others]).tobytes() == np.ascontiguousarray(clean[:, others]).tobytes()
    assert np.ascontiguousarray(bad[:, 17]).tobytes() == NONE_BYTES * 96
    ref = ref_planes(imsearch(y, delays, W5, NSTAT, 3, np.float32))
    assert np.ascontiguousarray(bad[:, 41]).tobytes() == np.ascontiguousarray(ref[:, 41]).tobytes()
    # group 1 has the back-delays 12, 10, 8, 5, 3: trial d meets the NaN at 36 + b and has no u of block 3 (block 2 is not valid) at
    # [48 + b, 64 + b), so no trial has a z at [60, 67); before 39 and after 75 + 3 (the widest boxcar) nothing reaches any of it
    assert list(S - delays[:, 1]) == [12, 10, 8, 5, 3]
    gone = bad[:, 41]['idm'] < 0
    assert gone[:NSTAT + S].all() and not gone[NSTAT + S:60].any() and gone[60:67].all() and not gone[67:].any()
    assert bad[:39, 41].tobytes() == clean[:39, 41].tobytes() and bad[79:, 41].tobytes() == clean[79:, 41].tobytes()
    assert bad[39, 41].tobytes() != clean[39, 41].tobytes() or clean[39, 41]['idm'] != 4
    assert (clean[NSTAT + S:]['idm'] >= 0).all()


# ---------------------------------------------------------------- 7. beside other kernels
def test_bit_identical_beside_a_contraction_and_the_beamformer():
    """The float run enqueued while X-engine contractions (their own stream) and xengBeamformRun (this stream) are in flight:
    bit-identical to the stand-alone run."""
    from tests.gpu_util import Xgpu, synth_voltages
    x, delays = float_case()
    alone = float_run()
    rng = np.random.default_rng(3)
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    ctx = IS(300, 5, 7, 3, delays=delays, weights=W5)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)

        def beside(k):
            if k % 8 == 0:
                for g in range(4):
                    ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)

        got = ctx.run(x, each=beside)
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    ctx.close()
    ffi.call("xengBeamformDestroy")
    assert got.tobytes() == alone.tobytes()


# ---------------------------------------------------------------- 8. refusals and tickets
def test_argument_and_state_refusals():
    """Every INVALID_ARGUMENT of Initialize (refused before the live context is touched), of the setters and of Run (nothing
    launched, the count unchanged); Run before SetDelays and every call without a context: INVALID_STATE."""
    ctx = IS(40, 3, 2, 3, max_delay=4)
    for args in ((0, 0, 3, 2, 4, 3, 16), (0, 40, 0, 2, 4, 3, 16), (0, 40, 3, 0, 4, 3, 16), (0, 40, 3, 2, -1, 3, 16), (0, (1 << 24) + 1, 3, 2, 4, 3, 16),
                 (0, 40, 3, 1025, 4, 3, 16), (0, 40, 3, 2, 4, 0, 16), (0, 40, 3, 2, 4, 7, 64), (0, 40, 3, 2, 4, 3, 1), (0, 40, 3, 2, 4, 3, (1 << 20) + 1),
                 (0, 40, 3, 2, 4, 4, 7), (0, 1 << 24, 24, 2, 4, 3, 16)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImsearchInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info() == (0, -1)                   # (the context is still there, without a table)
    din, dout = ffi.DeviceBuffer(3 * 4 * 40 * 4), ffi.DeviceBuffer(40 * 8)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengImsearchRun", din.ptr, dout.ptr)
    assert ei.value.status == INVALID_STATE
    good = np.array([[4, 2, 0], [2, 1, 0]], np.int32)
    for bad in (np.array([[5, 2, 0], [2, 1, 0]], np.int32), np.array([[4, 2, 0], [2, -1, 0]], np.int32)):
        with pytest.raises(ffi.XengError) as ei:
            ctx.set_delays(bad)
        assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengImsearchSetDelays", None)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (0, -1)
    ctx.set_delays(good)
    for bad in ([1, np.nan, 1], [1, np.inf, 1], [1, -1, 1], [0, 0, 0]):
        with pytest.raises(ffi.XengError) as ei:
            ctx.set_weights(np.array(bad, np.float32))
        assert ei.value.status == INVALID_ARGUMENT, bad
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengImsearchSetWeights", None)
    assert ei.value.status == INVALID_ARGUMENT
    for args in ((din.ptr + 4, dout.ptr), (din.ptr, dout.ptr + 8), (None, dout.ptr), (din.ptr, None)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImsearchRun", *args)
        assert ei.value.status == INVALID_ARGUMENT and _info() == (0, 4)
    for bad in ((None, 1, 1), (1, None, 1), (1, 1, None)):
        f = np.zeros(120, np.float32)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImsearchGetBaseline", *[None if b is None else _fp(f) for b in bad])
        assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengImsearchCheckGuards", None)
    assert ei.value.status == INVALID_ARGUMENT
    ctx.close()
    for name, args in (("xengImsearchRun", (din.ptr, dout.ptr)), ("xengImsearchReset", ()), ("xengImsearchSync", ()),
                       ("xengImsearchSetDelays", (good.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name


def test_completion_tickets_and_their_query():
    """xengImsearchMark / Wait / TicketDone as the other engines of the beamformer's stream: tickets count from 1 after Initialize; a
    ticket whose kernels have completed reads done = 1 (and its plane is there), every ticket does after Sync; unknown tickets (0,
    last + 1) and null pointers are errors; the backend's wait through both branches."""
    x, delays, w, ref = int_case("37 pixels, 5 trials, 3 widths")
    exp = ref_planes(ref)
    ctx = IS(37, 5, 5, 3, delays=delays, weights=w)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    outs = [ffi.DeviceBuffer(37 * 8) for _ in range(NINT)]
    tickets, done = [], ctypes.c_int(-1)
    for k in range(NINT):
        ffi.call("xengImsearchRun", din.ptr + k * ctx.image_bytes, outs[k].ptr)
        t = ctypes.c_ulonglong()
        ffi.call("xengImsearchMark", ctypes.byref(t))
        tickets.append(t.value)
    assert tickets == list(range(1, NINT + 1))
    ffi.call("xengImsearchTicketDone", tickets[-1], ctypes.byref(done))     # returns at once, whatever the answer
    assert done.value in (0, 1)
    ffi.call("xengImsearchWait", tickets[40])
    for t in tickets[38:41]:                                                # stream order: everything before it too
        ffi.call("xengImsearchTicketDone", t, ctypes.byref(done))
        assert done.value == 1
    assert outs[40].download(np.uint8).tobytes() == exp[40].tobytes()
    ffi.call("xengImsearchSync")
    ffi.call("xengImsearchTicketDone", tickets[-1], ctypes.byref(done))
    assert done.value == 1 and outs[-1].download(np.uint8).tobytes() == exp[-1].tobytes()
    for bad in (0, tickets[-1] + 1):
        with pytest.raises(ffi.XengError):
            ffi.call("xengImsearchTicketDone", bad, ctypes.byref(done))
        with pytest.raises(ffi.XengError):
            ffi.call("xengImsearchWait", bad)
    with pytest.raises(ffi.XengError):
        ffi.call("xengImsearchTicketDone", tickets[0], None)
    with pytest.raises(ffi.XengError):
        ffi.call("xengImsearchMark", None)
    from caltech_bifrost_dsp_amd.backend import HipBackend
    be = HipBackend()
    be.imsearch_reset()
    assert be.imsearch_info() == (0, S)
    tk = be.imsearch_mark()
    assert tk == tickets[-1] + 1
    be.imsearch_wait(tk)
    be.imsearch_wait(tk)                # already complete: answered by the query
    assert be.imsearch_ticket_done(tk) and be.imsearch_guards_intact()
    ctx.close()


# ---------------------------------------------------------------- 9. the block on device rings
def test_chain_source_to_image_search_on_device_rings_finds_the_planted_pulse():
    """Source -> UpchanImageSearch on a device ring, the planes to a pinned-host ring: 70 pixels, 5 groups at 40 ... 60 MHz, 64
    integrations of 1 s, four trials (S = 12), the pulse of tests/test_imsearch_cpu.py planted along trial 2 with the top of the band
    at integration 33.  The brightest candidate's pixel, dm, width and sample are the planted ones; the planes equal the float32
    restatement's word for word."""
    from caltech_bifrost_dsp_amd.blocks import UpchanImageSearch
    from caltech_bifrost_dsp_amd.ring import Ring
    from tests.imsearch_ref import plant
    from tests.pipeline_util import LOG, Sink, Source, run_blocks
    from tests.test_imsearch_cpu import ACC_LEN, DMS, NGROUP, _noise, _sky, image_header, table
    npix, seq0 = 70, 4096
    x = plant(_noise(np.random.default_rng(1), NINT, npix), table()[2], 33, 2, 33)
    got = []
    r0, r1 = Ring("im-output", space="cuda"), Ring("is-output", space="cuda_host")
    blk = UpchanImageSearch(LOG, r0, r1, lmn=_sky(npix), dms=DMS, nwidth=3, nstat=NSTAT, threshold=8.0, radius=0.015, weights=W5, max_delay=S,
                            on_candidates=got.extend, gpu=0)
    sink = Sink(r1, npix * 8)
    run_blocks([blk], Source(r0, [(image_header(npix=npix, seq0=seq0), x, NGROUP * 4 * npix * 4)]), [sink])
    ok = ctypes.c_int()
    ffi.call("xengImsearchCheckGuards", ctypes.byref(ok))
    ffi.call("xengImsearchDestroy")
    assert ok.value == 1
    (hd, tag, planes), = sink.sequences
    assert tag == seq0 and len(planes) == NINT and blk.stats['nsearched'] == NINT
    assert (hd['ndm'], hd['nwidth'], hd['widths'], hd['nstat'], hd['imsearch_latency'], hd['tint'], hd['threshold']) == (4, 3, [1, 2, 4], NSTAT, S, 1.0, 8.0)
    ref = ref_planes(imsearch(x, table(), W5, NSTAT, 3, np.float32))
    for k, o in enumerate(planes):
        assert o.tobytes() == ref[k].tobytes(), k
    best = max(got, key=lambda c: c['snr'])
    assert (best['pixel'], best['idm'], best['dm'], best['width'], best['window']) == (33, 2, DMS[2], 2, 33 + S + 1)
    assert best['sample'] == seq0 + 33 * ACC_LEN and best['snr'] > 15 and blk.stats['ncand'] == len(got)


# ---------------------------------------------------------------- 10. behind the imager
def test_chain_upchan_image_to_image_search_at_16_stands():
    """Source (visibilities of 16 stands, 8 fine channels) -> UpchanImage (37 pixels, groups of two channels) -> UpchanImageSearch on
    device rings, 24 integrations: the search takes npix, the groups, their frequencies and the integration length from the imager's
    header (integrations of 4 ms, groups 24 kHz apart at 50 MHz: DM 2.5 lags 3 integrations over the band), each plane is npix
    records, and the planes equal a direct run of xengImsearchRun on the images the imager wrote, bit for bit."""
    from caltech_bifrost_dsp_amd.blocks import UpchanImage, UpchanImageSearch, group_frequencies, image_dm_delays
    from caltech_bifrost_dsp_amd.ring import Ring
    from tests.image_ref import random_array
    from tests.pipeline_util import LOG, Sink, Source, run_blocks
    from tests.test_image_cpu import _sky, vis_header
    nstand, nfine, nfavg, npix, nint, nstat, dms = 16, 8, 2, 37, 24, 4, [0.0, 2.5]
    ngroup, n = nfine // nfavg, 2 * nstand
    rng = np.random.default_rng(21)
    pos, lmn = random_array(rng, nstand, 300.0, 2.0), _sky(rng, npix)
    A = (rng.normal(0, 10, (nint, nfine, n, n)) + 1j * rng.normal(0, 10, (nint, nfine, n, n)))
    V = (A + np.conj(A.transpose(0, 1, 3, 2))).astype(np.complex64)
    hdr = vis_header(nstand=nstand, nfine=nfine, seq0=960)
    r0, r1, r2 = Ring("uc-output", space="cuda"), Ring("image-output", space="cuda"), Ring("is-output", space="cuda_host")
    im = UpchanImage(LOG, r0, r1, pos, lmn, nfavg=nfavg, gpu=0)
    blk = UpchanImageSearch(LOG, r1, r2, lmn=lmn, dms=dms, nwidth=2, max_delay=8, nstat=nstat, threshold=3.0, gpu=0)
    mid, sink = Sink(r1, ngroup * 4 * npix * 4), Sink(r2, npix * 8)
    run_blocks([im, blk], Source(r0, [(hdr, V.reshape(-1), nfine * n * n * 8)]), [mid, sink])
    ffi.call("xengImsearchDestroy")
    ffi.call("xengImageDestroy")
    (ih, _, images), = mid.sequences
    (hd, tag, planes), = sink.sequences
    assert len(images) == len(planes) == nint and tag == hd['seq0'] == 960 and all(p.nbytes == npix * 8 for p in planes)
    tint = hdr['acc_len'] * hdr['nchan'] / hdr['bw_hz']
    tab = image_dm_delays(group_frequencies(ih, ngroup), dms, tint)
    assert tab.max() == tab[1, 0] == 3 and (tab[0] == 0).all()
    assert (hd['npix'], hd['nfavg'], hd['ndm'], hd['dms'], hd['imsearch_latency'], hd['nstat']) == (npix, nfavg, 2, dms, 3, nstat)
    assert hd['tint'] == tint and hd['image_sfreq'] == ih['image_sfreq']
    ctx = IS(npix, ngroup, 2, 2, nstat=nstat, max_delay=8, delays=tab)
    direct = ctx.run(np.stack([i.view(np.float32).reshape(ngroup, 4, npix) for i in images]))
    ctx.close()
    for k, o in enumerate(planes):
        assert o.tobytes() == direct[k].tobytes(), k
    assert (direct[:nstat + 3]['idm'] == -1).all() and (direct[nstat + 3:]['idm'] >= 0).all() and blk.stats['nsearched'] == nint
