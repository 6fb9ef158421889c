"""BeamPulseSearch on the MI355X: xengPulse* against the restatement (tests/pulse_ref.py).  Word for word on integer data (both
products, series that do not fill a work-group, no tail and a tail longer than any call, calls of 1, 7 and 30 windows that put
block boundaries at their first, an inner and their last window); bit identity across splits of a run over calls, after Reset
against a fresh context and beside an X-engine contraction and xengBeamformRun; float data against the float64 restatement at
tol = 1e-4 * max(1, |snr|), and the baseline's c, m, v and every record's B bit for bit against the float32 restatement; series
without a baseline; tickets and the checks that need a context; the live shape with a planted pulse; and Source ->
BeamDedisperse -> BeamPulseSearch on device rings.  The output sits between two poisoned guard bands that are checked after
every call, the state's guards at every close.  No wall-clock assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamDedisperse, BeamPulseSearch  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.pulse_search import RECORD, as_records  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks  # noqa: E402
from tests.pulse_cases import FIXED_SIZES, INT_CASES, _sizes, float_case, integer_case  # noqa: E402,F401
from tests.pulse_ref import merge_records, pulse_search, series  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
NONE_BYTES = np.array([(0.0, -1, -1, 0.0)], RECORD).tobytes()


def tol(snr_ref):
    """The bar of the float tests: five times what a numpy float32 emulation of the contract's evaluation order (no fused
    multiply-adds; 512 series x 1024 windows, nstat = 256, widths 1..128, mean / sigma = 55) differs from float64 by, 2.0e-5 of
    max(1, |snr|).  The margin is for the fused q, for g = 1/sqrt(v) being the library's choice, and for contraction."""
    return 1e-4 * np.maximum(1.0, np.abs(snr_ref))


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    n, k = ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengPulseGetInfo", ctypes.byref(n), ctypes.byref(k))
    return n.value, k.value


class PS:
    """The xengPulse context (one per process), an input buffer and an output plane between two poisoned guard bands."""

    def __init__(self, npair, ndm, nwin, nprod, nwidth, nstat):
        self.npair, self.ndm, self.nwin, self.nprod, self.nwidth, self.nstat = npair, ndm, nwin, nprod, nwidth, nstat
        ffi.call("xengPulseInitialize", 0, npair, ndm, nwin, nprod, nwidth, nstat)
        self.din = ffi.DeviceBuffer(nwin * npair * ndm * nprod * 4)
        self.dout = ffi.DeviceBuffer(2 * GUARD + npair * ndm * 16)

    def enqueue(self, x):
        nc = x.shape[0]
        assert x.shape == (nc, self.npair, self.ndm, self.nprod)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        self.din.upload(np.ascontiguousarray(x, np.float32))
        ffi.call("xengPulseRun", self.din.ptr, nc, self.dout.ptr + GUARD)

    def result(self):
        """After a sync: the plane; every byte before and after it must still be poison."""
        raw = self.dout.download(np.uint8)
        n = self.npair * self.ndm * 16
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + n:] == POISON).all(), "bytes past the output's %d records were written" % (self.npair * self.ndm)
        return raw[GUARD:GUARD + n].copy().view(RECORD).reshape(self.npair, self.ndm)

    def run(self, x):
        self.enqueue(x)
        ffi.call("xengPulseSync")
        return self.result()

    def stream(self, x, sizes):
        """Consecutive calls of the given sizes over the windows of x; the planes, one per call."""
        outs, n = [], 0
        for nc in sizes:
            outs.append(self.run(x[n:n + nc]))
            n += nc
        assert n == x.shape[0]
        return outs

    def baseline(self):
        out = [np.empty((self.npair, self.ndm), np.float32) for _ in range(3)]
        ffi.call("xengPulseGetBaseline", *[_fp(a) for a in out])
        return out

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengPulseCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengPulseDestroy")


def planes_as_records(planes):
    return [dict(snr=p['snr'], n=p['n'], iw=p['iw'], B=p['B']) for p in planes]


def merged_bits(planes, sizes):
    """The host's merge of the calls' planes (strictly greater replaces, in call order), as raw words."""
    m = merge_records(planes_as_records(planes), sizes)
    out = np.zeros(m['n'].shape, RECORD)
    out['snr'], out['n'], out['iw'], out['B'] = m['snr'], m['n'], m['iw'], m['B']
    return out.tobytes()


# ---------------------------------------------------------------- 1. word for word on integer data
def winners_lead(ref, sizes):
    """On the float64 reference: in every call of every series, every scored candidate other than the winner either trails it
    by more than tol, or holds EXACTLY the winner's score.  Integer data make exact ties common -- equal sums at two windows, or
    B_4w = 2 B_w against rho_(iw+2) = rho_iw / 2 -- and in 30 windows of values 0..49 no seed avoids them; there the contract's
    order (smallest n, then smallest iw) decides, not rounding: equal B under the same g and a rho scaled by a power of two are
    equal in fp32 too.  Returns the number of (series, call) that fail."""
    bad, a = 0, 0
    snr = ref['snr'].reshape(ref['snr'].shape[0], ref['snr'].shape[1], -1)
    for nc in sizes:
        s = np.where(np.isnan(snr[a:a + nc]), -np.inf, snr[a:a + nc]).reshape(-1, snr.shape[2])
        top = s.max(axis=0)
        with np.errstate(invalid='ignore'):
            near = (s != top) & (top - s <= tol(top)) & np.isfinite(top)
        bad += int(near.any(axis=0).sum())
        a += nc
    return bad


@pytest.mark.parametrize("case", sorted(INT_CASES))
def test_integer_data_match_the_restatement_word_for_word(case):
    """Every stage of the contract is exact in fp32 on this data (sums below 2^24, nstat a power of two), so after every call
    GetBaseline's c, m, var equal the float32 restatement bit for bit (INVALID_STATE before the first block is complete), and
    each record's B does; (n_call, iw) equal it for every series and call, after winners_lead has held on the float64 reference
    for all of them."""
    npair, ndm, nprod, nwidth, nstat, total, _ = INT_CASES[case]
    x, sizes, r32, r64 = integer_case(case)
    assert winners_lead(r64, sizes) == 0
    ends = np.cumsum(sizes)
    starts = ends - np.array(sizes)
    if nstat == 16:
        assert any(a % nstat == 0 for a in starts) and any((e - 1) % nstat == 0 for e in ends) and any((e - 1) % nstat == nstat - 1 for e in ends)
        assert any(a < k * nstat < e - 1 for a, e in zip(starts, ends) for k in range(1, 8))
    ps = PS(npair, ndm, 30, nprod, nwidth, nstat)
    a = 0
    for k, nc in enumerate(sizes):
        got = ps.run(x[a:a + nc])
        a += nc
        assert _info() == (a, a // nstat)
        exp, exp64 = r32['records'][k], r64['records'][k]
        assert np.array_equal(got['n'], exp['n']) and np.array_equal(got['iw'], exp['iw']), (case, k)
        assert np.array_equal(exp['n'], exp64['n']) and np.array_equal(exp['iw'], exp64['iw'])
        assert np.array_equal(got['B'].view(np.uint32), exp['B'].view(np.uint32)), (case, k)
        assert (np.abs(got['snr'] - exp64['snr']) <= tol(exp64['snr'])).all(), (case, k)
        if a < nstat:
            with pytest.raises(ffi.XengError) as ei:
                ps.baseline()
            assert ei.value.status == INVALID_STATE
        else:
            blk = a // nstat - 1
            for g, f in zip(ps.baseline(), ('c', 'm', 'v')):
                assert np.array_equal(g.view(np.uint32), r32[f][blk].view(np.uint32)), (case, k, f)
    ps.close()


# ---------------------------------------------------------------- 2. bit identity
@pytest.mark.parametrize("nprod", [1, 4])
def test_bit_identical_across_splits_reset_and_concurrent_kernels(nprod):
    """540 windows of float data, nstat = 128, 8 widths: one call per 30 windows, 10 windows, 1 window and a random split give
    the same merged {snr, n, iw, B} bit for bit (each after a Reset, so the ring position and what the state holds differ too),
    and so does a fresh context run while X-engine contractions and xengBeamformRun are in flight."""
    npair, ndm, nwin, nwidth, nstat, total = 3, 37, 30, 8, 128, 540
    rng = np.random.default_rng(7 + nprod)
    x = float_case(rng, total, npair, ndm, nprod)
    ps = PS(npair, ndm, nwin, nprod, nwidth, nstat)
    first = merged_bits(ps.stream(x, [30] * 18), [30] * 18)
    outs = []
    for sizes in ([10] * 54, [1] * 540, _sizes(rng, total, nwin)):
        ffi.call("xengPulseReset")
        assert _info() == (0, 0)
        outs.append(merged_bits(ps.stream(x, sizes), sizes))
    ps.close()
    # a fresh context beside other work: contractions on their own stream, the beamformer on this one
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    ps = PS(npair, ndm, nwin, nprod, nwidth, nstat)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        parts = []
        for k in range(18):
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ps.enqueue(x[30 * k:30 * k + 30])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengPulseSync")
            parts.append(ps.result())
        ffi.call("xengXgpuSync")
        outs.append(merged_bits(parts, [30] * 18))
    finally:
        xg.close()
    ps.close()
    ffi.call("xengBeamformDestroy")
    for o in outs:
        assert o == first
    assert (np.frombuffer(first, RECORD)['n'] >= nstat).all()


# ---------------------------------------------------------------- 3. float data
def check_against_float64(planes, sizes, ref, what):
    """Every plane of a run against the float64 reference, all series: a series the reference scores nothing for in the call
    holds the empty record and the others a scored (n, iw), the record's snr within tol of the reference's score at that
    (n, iw), and that score within 2 tol of the reference's maximum of the call.  Returns the worst |snr - ref| / max(1, |ref|)."""
    nwidth = ref['snr'].shape[1]
    snr = ref['snr'].reshape(ref['snr'].shape[0], nwidth, -1)
    scored = ref['scored'].reshape(snr.shape)
    col = np.arange(snr.shape[2])
    worst, a = 0.0, 0
    for k, (p, nc) in enumerate(zip(planes, sizes)):
        p = p.reshape(-1)
        anyref = scored[a:a + nc].any(axis=(0, 1))
        assert np.array_equal(p['n'] >= 0, anyref), (what, k)
        empty = p[~anyref]
        assert empty.tobytes() == NONE_BYTES * empty.size, (what, k)
        n, iw, c = p['n'][anyref], p['iw'][anyref], col[anyref]
        assert (n < nc).all() and (iw >= 0).all() and (iw < nwidth).all() and scored[a + n, iw, c].all(), (what, k)
        at = snr[a + n, iw, c]
        top = np.where(scored[a:a + nc], snr[a:a + nc], -np.inf).max(axis=(0, 1))[anyref]
        err = np.abs(p['snr'][anyref].astype(np.float64) - at)
        if err.size:
            worst = max(worst, float((err / np.maximum(1.0, np.abs(at))).max()))
        assert (err <= tol(at)).all(), "%s, call %d: worst |snr - ref| / tol = %.3g" % (what, k, (err / tol(at)).max())
        assert (top - at <= 2 * tol(top)).all(), (what, k)
        a += nc
    return worst


@pytest.mark.parametrize("nprod,nstat,nwidth", [(1, 24, 5), (4, 24, 5), (1, 256, 8), (4, 256, 8)])
def test_float_data_within_tol_of_the_float64_restatement(nprod, nstat, nwidth):
    """3 x 37 series of chi^2 powers with gains in [0.5, 1.5], calls of 30 windows and a ragged last one: nstat = 24, not a power of
    two, with the 5 widths a block of 24 admits (2^(nwidth-1) <= nstat), and nstat = 256 with 8.  A near-tie may resolve either
    way and no series is excluded.  On the MI355X the worst |snr - ref| / max(1, |ref|) measured is recorded in DESIGN.md 4.17."""
    npair, ndm, nwin = 3, 37, 30
    total = 4 * nstat + 17
    rng = np.random.default_rng(27 + nprod + nstat)
    x = float_case(rng, total, npair, ndm, nprod)
    sizes = [nwin] * (total // nwin) + ([total % nwin] if total % nwin else [])
    ref = pulse_search(series(x, np.float64), nstat, nwidth, np.float64)
    ps = PS(npair, ndm, nwin, nprod, nwidth, nstat)
    planes = ps.stream(x, sizes)
    ps.close()
    worst = check_against_float64(planes, sizes, ref, "float nprod=%d nstat=%d" % (nprod, nstat))
    print("pulse float nprod=%d nstat=%d nwidth=%d: worst |snr - ref| / max(1, |ref|) = %.3g (tol 1e-4)" % (nprod, nstat, nwidth, worst))


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("nstat,nwidth", [(24, 5), (128, 8)])
def test_float_data_hold_the_baseline_and_the_boxcar_sums_bit_for_bit(nstat, nwidth, nprod):
    """The contract's roundings on the device, on float data: 3 x 37 series of float_case, calls of 30 windows and a ragged last
    one.  After every call that completes a block GetBaseline's c, m and v equal the float32 restatement (delta = fl(z - c),
    a = fl(a + delta), q = fmaf(delta, delta, q), m = fl(a r), v = fmaf(-m, m, fl(q r)), the fused steps correctly rounded) as
    uint32 words; and each record's B equals the restatement's B at the record's own (n, iw) -- y = fl(fl(z - c) - m), not
    contracted, and plain fp32 adds.  snr keeps tol() and a near-tie may resolve either way, as check_against_float64 has it."""
    npair, ndm, nwin = 3, 37, 30
    total = 4 * nstat + 17
    rng = np.random.default_rng(127 + nprod + nstat)
    x = float_case(rng, total, npair, ndm, nprod)
    sizes = [nwin] * (total // nwin) + ([total % nwin] if total % nwin else [])
    assert sizes[-1] < nwin
    r64 = pulse_search(series(x, np.float64), nstat, nwidth, np.float64)
    r32 = pulse_search(series(x, np.float32), nstat, nwidth, np.float32)
    B32 = r32['B'].reshape(total, nwidth, -1)
    ps = PS(npair, ndm, nwin, nprod, nwidth, nstat)
    planes, a, nblocks = [], 0, 0
    for nc in sizes:
        before = a // nstat
        planes.append(ps.run(x[a:a + nc]))
        if (a + nc) // nstat > before:
            blk = (a + nc) // nstat - 1
            for g, f in zip(ps.baseline(), ('c', 'm', 'v')):
                diff = g.view(np.uint32) != r32[f][blk].view(np.uint32)
                print("pulse float nprod=%d nstat=%d block %d: %d of %d words of %s differ" % (nprod, nstat, blk, diff.sum(), diff.size, f))
                assert not diff.any(), (f, blk, int(diff.sum()))
            nblocks += 1
        p = planes[-1].reshape(-1)
        has = p['n'] >= 0
        col = np.arange(p.size)[has]
        exp = B32[a + p['n'][has], p['iw'][has], col]
        diff = p['B'][has].view(np.uint32) != exp.view(np.uint32)
        print("pulse float nprod=%d nstat=%d call at %d: %d of %d B differ" % (nprod, nstat, a, diff.sum(), diff.size))
        assert not diff.any(), (a, int(diff.sum()))
        a += nc
    ps.close()
    assert nblocks == 4 and all((pl['n'] >= 0).all() for pl in planes[-2:])
    check_against_float64(planes, sizes, r64, "float bit for bit nprod=%d nstat=%d" % (nprod, nstat))


# ---------------------------------------------------------------- 4. series without a baseline
def test_series_without_a_baseline_score_nothing_and_recover():
    """A constant series (v = 0 in every block), a series with one NaN window and one with one +Inf window, among clean
    neighbours; nstat = 16, 4 widths, calls of 8 windows, so a call lies in one block.  The constant series never scores.  The NaN
    at window 36 (block 2): calls 4 (32..39: boxcars that do not touch 36 score) and 5 hold records, calls 6 and 7 (block 3, whose
    previous block is not valid) hold {0, -1, -1, 0}, call 8 (block 4) scores again.  The Inf is not a NaN: its own window scores
    +inf, then block 3 is without a baseline in the same way.  Every record equals the float32 restatement's (n, iw, B); the
    neighbours are bit for bit what they are in a run without the defects."""
    npair, ndm, nwin, nwidth, nstat, total = 2, 35, 8, 4, 16, 96
    rng = np.random.default_rng(41)
    clean = float_case(rng, total, npair, ndm, 1)
    x = clean.copy()
    x[:, 0, 3, 0] = 777.0
    x[36, 1, 5, 0] = np.nan
    x[36, 1, 30, 0] = np.inf
    sizes = [nwin] * (total // nwin)
    ps = PS(npair, ndm, nwin, 1, nwidth, nstat)
    good = ps.stream(clean, sizes)
    ffi.call("xengPulseReset")
    bad = ps.stream(x, sizes)
    ps.close()
    r32 = pulse_search(series(x, np.float32), nstat, nwidth, np.float32, sizes)
    others = np.ones((npair, ndm), bool)
    others[0, 3] = others[1, 5] = others[1, 30] = False
    for k in range(len(sizes)):
        assert good[k][others].tobytes() == bad[k][others].tobytes(), k
        assert bad[k][0, 3].tobytes() == NONE_BYTES, k
        for s in ((1, 5), (1, 30)):
            e = r32['records'][k]
            assert (bad[k][s]['n'], bad[k][s]['iw']) == (e['n'][s], e['iw'][s]), (k, s)
            assert bad[k][s]['B'].tobytes() == e['B'][s].tobytes() or (np.isnan(bad[k][s]['B']) and np.isnan(e['B'][s])), (k, s)
            empty = k < 2 or k in (6, 7)                            # no previous block, or a previous block that is not valid
            assert (bad[k][s].tobytes() == NONE_BYTES) == empty, (k, s)
            if k >= 8:
                assert good[k][s]['n'] >= 0 and bad[k][s]['n'] >= 0
        if k >= 2:
            assert (good[k]['n'] >= 0).all()
    assert bad[4][1, 5]['n'] >= 0 and np.isfinite(bad[4][1, 5]['snr']) and not (bad[4][1, 5]['n'] == 4 and bad[4][1, 5]['iw'] == 0)
    assert np.isposinf(bad[4][1, 30]['snr']) and (bad[4][1, 30]['n'], bad[4][1, 30]['iw']) == (4, 0) and np.isposinf(bad[4][1, 30]['B'])


# ---------------------------------------------------------------- 5. tickets and checks
def test_completion_tickets_and_their_query():
    """xengPulseMark / Wait / TicketDone as the six engines of tests/test_beamform_gpu.py: tickets count from 1 after Initialize;
    a ticket whose kernel has completed reads done = 1 (and its output is there), every ticket does after Sync; unknown tickets
    (0, last + 1) and null pointers are errors; the backend's wait through both branches."""
    npair, ndm, nwin, nwidth, nstat = 2, 40, 8, 3, 8
    rng = np.random.default_rng(11)
    x = rng.integers(0, 50, (2 * nwin, npair, ndm, 1)).astype(np.float32)
    exp = pulse_search(series(x, np.float32), nstat, nwidth, np.float32, [nwin, nwin])['records'][1]
    ffi.call("xengPulseInitialize", 0, npair, ndm, nwin, 1, nwidth, nstat)
    d0, d1 = ffi.DeviceBuffer(x[:nwin].nbytes).upload(x[:nwin]), ffi.DeviceBuffer(x[nwin:].nbytes).upload(x[nwin:])

    def run(o):                                     # two calls from a reset: the second one's plane stays in o
        ffi.call("xengPulseReset")
        ffi.call("xengPulseRun", d0.ptr, nwin, o.ptr)
        ffi.call("xengPulseRun", d1.ptr, nwin, o.ptr)

    def check(o):
        got = o.download(np.uint8).view(RECORD).reshape(npair, ndm)
        assert np.array_equal(got['n'], exp['n']) and np.array_equal(got['iw'], exp['iw']) and (got['n'] >= 0).all()
        assert np.array_equal(got['B'].view(np.uint32), exp['B'].view(np.uint32))

    outs = [ffi.DeviceBuffer(npair * ndm * 16) for _ in range(6)]
    tickets, done = [], ctypes.c_int(-1)
    for o in outs:
        run(o)
        t = ctypes.c_ulonglong()
        ffi.call("xengPulseMark", ctypes.byref(t))
        tickets.append(t.value)
    assert tickets == list(range(1, 7))
    ffi.call("xengPulseTicketDone", tickets[-1], ctypes.byref(done))       # returns at once, whatever the answer
    assert done.value in (0, 1)
    ffi.call("xengPulseWait", tickets[2])
    for t in tickets[:3]:                                                   # stream order: everything before it too
        ffi.call("xengPulseTicketDone", t, ctypes.byref(done))
        assert done.value == 1
    check(outs[2])
    ffi.call("xengPulseSync")
    ffi.call("xengPulseTicketDone", tickets[-1], ctypes.byref(done))
    assert done.value == 1
    check(outs[-1])
    for bad in (0, tickets[-1] + 1):
        with pytest.raises(ffi.XengError):
            ffi.call("xengPulseTicketDone", bad, ctypes.byref(done))
        with pytest.raises(ffi.XengError):
            ffi.call("xengPulseWait", bad)
    with pytest.raises(ffi.XengError):
        ffi.call("xengPulseTicketDone", tickets[0], None)
    with pytest.raises(ffi.XengError):
        ffi.call("xengPulseMark", None)
    from caltech_bifrost_dsp_amd.backend import HipBackend
    be = HipBackend()
    run(outs[0])
    tk = be.pulse_mark()
    assert tk == tickets[-1] + 1
    be.pulse_wait(tk)
    be.pulse_wait(tk)                   # already complete: answered by the query
    assert be.pulse_ticket_done(tk) and be.pulse_info() == (2 * nwin, 2) and be.pulse_guards_intact()
    check(outs[0])
    ffi.call("xengPulseDestroy")


def test_argument_checks_with_a_context():
    """Every INVALID_ARGUMENT of Initialize (a live context survives none of them being tried first: each is refused before the
    old context is touched), of Run with a context (nwin_call outside 1..nwin, misaligned or null pointers: nothing launched, the
    count unchanged), GetBaseline before a block is complete (INVALID_STATE) and after; Reset moves only the count."""
    ps = PS(2, 16, 4, 1, 3, 4)
    for args in ((0, 0, 16, 4, 1, 3, 4), (0, 2, 0, 4, 1, 3, 4), (0, 2, 16, 0, 1, 3, 4), (0, 2, 16, 4, 2, 3, 4), (0, 2, 16, 4, 1, 0, 4), (0, 2, 16, 4, 1, 9, 4),
                 (0, 2, 16, 4, 1, 3, 1), (0, 2, 16, 4, 1, 3, (1 << 20) + 1), (0, 2, 16, 4, 1, 4, 7), (0, 2, 16, 129, 1, 1, 4), (0, 1 << 13, 1 << 12, 4, 1, 3, 4)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPulseInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info() == (0, 0)                    # (the context is still there)
    for args in ((ps.din.ptr, 0, ps.dout.ptr), (ps.din.ptr, 5, ps.dout.ptr), (ps.din.ptr + 4, 1, ps.dout.ptr), (ps.din.ptr, 1, ps.dout.ptr + 8),
                 (None, 1, ps.dout.ptr), (ps.din.ptr, 1, None)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPulseRun", *args)
        assert ei.value.status == INVALID_ARGUMENT and _info() == (0, 0)
    x = np.arange(8 * 2 * 16, dtype=np.float32).reshape(8, 2, 16, 1) % 7
    assert ps.run(x[:3]).tobytes() == NONE_BYTES * 32 and _info() == (3, 0)
    with pytest.raises(ffi.XengError) as ei:
        ps.baseline()
    assert ei.value.status == INVALID_STATE
    for bad in ((None, 1, 1), (1, None, 1), (1, 1, None)):
        f = np.zeros(32, np.float32)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPulseGetBaseline", *[None if b is None else _fp(f) for b in bad])
        assert ei.value.status == INVALID_ARGUMENT
    ps.run(x[3:4])
    c, m, v = ps.baseline()
    r32 = pulse_search(series(x, np.float32), 4, 3, np.float32)
    assert np.array_equal(c, r32['c'][0]) and np.array_equal(m, r32['m'][0]) and np.array_equal(v, r32['v'][0]) and _info() == (4, 1)
    ffi.call("xengPulseReset")
    assert _info() == (0, 0)
    with pytest.raises(ffi.XengError) as ei:
        ps.baseline()
    assert ei.value.status == INVALID_STATE
    ps.close()
    for name, args in (("xengPulseRun", (ps.din.ptr, 1, ps.dout.ptr)), ("xengPulseReset", ()), ("xengPulseSync", ())):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name


# ---------------------------------------------------------------- 6. the live shape once
def live_case():
    """16 x 256 series, 1200 windows of noise (mean / sigma = 78) and one box of 8 windows, 9 sigma / sqrt(8) each, in series
    (5, 123), ending at window 799 -- inside block 3, so that the block before it is free of the pulse."""
    npair, ndm, total, p0, d0, n1 = 16, 256, 1200, 5, 123, 799
    rng = np.random.default_rng(2024)
    z = rng.chisquare(4 * 3072, (total, npair, ndm))
    sigma = np.sqrt(2 * 4 * 3072)
    z[n1 - 7:n1 + 1, p0, d0] += 9 * sigma / np.sqrt(8)
    return z.astype(np.float32)[..., None], (p0, d0, n1)


def test_live_shape_finds_a_planted_pulse():
    """30-window calls, nwidth = 8, nstat = 256: the pulse is the best record of its series over the run, at its (n, iw = 3),
    near 9 sigma and above every other series; and the checks of the float test hold on all 4096 series."""
    npair, ndm, nwin, nwidth, nstat = 16, 256, 30, 8, 256
    x, (p0, d0, n1) = live_case()
    sizes = [nwin] * (x.shape[0] // nwin)
    ref = pulse_search(series(x, np.float64), nstat, nwidth, np.float64)
    ps = PS(npair, ndm, nwin, 1, nwidth, nstat)
    planes = ps.stream(x, sizes)
    ps.close()
    worst = check_against_float64(planes, sizes, ref, "live shape")
    print("pulse live shape: worst |snr - ref| / max(1, |ref|) = %.3g (tol 1e-4)" % worst)
    best = merge_records(planes_as_records(planes), sizes)
    assert (best['n'][p0, d0], best['iw'][p0, d0]) == (n1, 3)
    assert abs(best['snr'][p0, d0] - ref['snr'][n1, 3, p0, d0]) <= tol(ref['snr'][n1, 3, p0, d0]) and 7 < best['snr'][p0, d0] < 11
    rest = best['snr'].copy()
    rest[p0, d0] = 0
    assert rest.max() < 7 < best['snr'][p0, d0]
    k = n1 // nwin
    assert (planes[k][p0, d0]['n'], planes[k][p0, d0]['iw']) == (n1 - k * nwin, 3)


# ---------------------------------------------------------------- 7. the chain on device rings
def chain_case():
    """Dual-pol power beams [nwindows][2 pairs][4 x 8 fine channels][4] of values 0..49 with one pulse of 150 in XX of pair 1,
    dispersed at trial 5 of 8 and reaching the top channel at window t0; the header UpchanSumBeams writes."""
    from tests.test_dedisp_cpu import header_table, power_header
    nchan, npair, N, W, nwin, nspan, t0, d0 = 4, 2, 8, 4, 16, 5, 34, 5
    nfine = nchan * N
    dms = [float(d) for d in np.linspace(0.0, 0.14, 8)]
    hdr = power_header(nchan, npair, N, W, seq0=4096)
    table, tsamp = header_table(hdr, nfine, dms)
    rng = np.random.default_rng(99)
    x = rng.integers(0, 50, (nspan * nwin, npair, nfine, 4)).astype(np.float32)
    x[t0 + table[d0], 1, np.arange(nfine), 0] += 150
    return dict(nchan=nchan, npair=npair, N=N, W=W, nwin=nwin, nspan=nspan, t0=t0, d0=d0, nfine=nfine, dms=dms, hdr=hdr, table=table, x=x)


def test_chain_source_dedisperse_pulse_search_on_device_rings():
    """Source -> BeamDedisperse -> BeamPulseSearch, nstat = 16 = nwin: on_candidates receives exactly one candidate, the planted
    pair, the planted DM's trial and `sample` = the sample at which the pulse reached the top channel; the output ring's planes
    equal a direct run of xengPulseRun on the spans BeamDedisperse wrote, bit for bit."""
    c = chain_case()
    npair, nwin, ndm, nstat, nwidth = c['npair'], c['nwin'], len(c['dms']), 16, 3
    r0, r1, r2 = Ring("ub-output", space="cuda"), Ring("dd-output", space="cuda"), Ring("ps-output", space="cuda_host")
    got = []
    dd = BeamDedisperse(LOG, r0, r1, npair=npair, nchan=c['nchan'], nupchan=c['N'], nwin=nwin, dms=c['dms'], gpu=0)
    ps = BeamPulseSearch(LOG, r1, r2, npair=npair, ndm=ndm, nwin=nwin, nwidth=nwidth, nstat=nstat, threshold=8.0, on_candidates=got.extend, gpu=0)
    mid, sink = Sink(r1, nwin * npair * ndm * 4), Sink(r2, npair * ndm * 16)
    run_blocks([dd, ps], Source(r0, [(c['hdr'], c['x'], nwin * npair * c['nfine'] * 16)]), [mid, sink])
    (dh, _, dspans), = mid.sequences
    (hd, tag, planes), = sink.sequences
    assert len(dspans) == len(planes) == c['nspan'] and tag == 4096
    S = int(c['table'].max())
    assert dh['dedisp_latency'] == S and 0 < S < nstat - 2
    assert hd['nwidth'] == nwidth and hd['nstat'] == nstat and hd['widths'] == [1, 2, 4] and hd['threshold'] == 8.0 and hd['ndm'] == ndm
    assert len(got) == 1, got
    cand, = got
    acc_len = c['W'] * c['N']
    assert (cand['pair'], cand['idm'], cand['dm'], cand['width']) == (1, c['d0'], c['dms'][c['d0']], 1)
    assert cand['sample'] == 4096 + c['t0'] * acc_len and cand['window'] == (c['t0'] + S) % nwin and cand['snr'] > 8
    assert ps.stats['ncand'] == 1 and ps.stats['nwindow'] == c['nspan'] * nwin
    direct = PS(npair, ndm, nwin, 1, nwidth, nstat)
    for k, (sp, pl) in enumerate(zip(dspans, planes)):
        assert direct.run(sp.view(np.float32).reshape(nwin, npair, ndm, 1)).tobytes() == pl.tobytes(), k
    direct.close()
    assert (as_records(planes[0], npair, ndm)['n'] == -1).all() and (as_records(planes[2], npair, ndm)['n'] >= 0).all()
