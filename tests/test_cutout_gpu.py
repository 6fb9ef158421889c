"""BeamPulseCutout on the MI355X: xengCutout* against the restatement (tests/cutout_ref.py), byte for byte and with no tolerance: which
requests every call serves and which expire, and every byte of a serving call's output -- the records, the waterfalls and the
planes of the served slots, and the poison everywhere else.  The output sits between poisoned guard bands that are checked after
every call, the input is read back after every call and must be what was uploaded, the state's guards are checked at every close.
The shapes are the smallest at which each mechanism can fail (the docstrings say which).  Integer data against the float64 statement
(blocks/pulse_cutout.py cutout_reference); xengDedispRun -> xengPulseRun -> pulse_candidates -> cutout_requests -> xengCutoutRun on
the device.  No wall-clock assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import cutout_fine_dms, cutout_reference, cutout_requests, pulse_candidates  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.dedisp import dm_delays  # noqa: E402
from tests import cutout_cases, cutout_ref  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
K_MAD = cutout_cases.K_MAD
_pi = ctypes.POINTER(ctypes.c_int)
PULSE_RECORD = np.dtype([('snr', '<f4'), ('n', '<i4'), ('iw', '<i4'), ('B', '<f4')])


def _info():
    n, k, b = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong()
    ffi.call("xengCutoutGetInfo", ctypes.byref(n), ctypes.byref(k), ctypes.byref(b))
    return n.value, k.value, b.value


def _run(din, nc, out_ptr, nreq_max):
    ns, ne = ctypes.c_int(-1), ctypes.c_int(-1)
    served, expired = (ctypes.c_int * nreq_max)(), (ctypes.c_int * 1024)()
    ffi.call("xengCutoutRun", din, nc, out_ptr, ctypes.byref(ns), served, ctypes.byref(ne), expired)
    return list(served[:ns.value]), list(expired[:ne.value])


class CO:
    """The xengCutout context (one per process), an input buffer, the output between poisoned guard bands, and the restatement
    beside it: every request and every call goes to both and is compared byte for byte."""

    def __init__(self, npair, nfine, nwin, delays, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, weights=None):
        self.npair, self.nfine, self.nwin, self.nreq_max = npair, nfine, nwin, nreq_max
        self.ref = cutout_ref.CutoutRef(npair, nfine, nwin, delays, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, K_MAD, weights)
        # the buffers come first, the context second: tests/test_accel_gpu.py says why
        self.din = ffi.DeviceBuffer(nwin * npair * nfine * 16)
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.ref.out_bytes)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        ffi.call("xengCutoutInitialize", 0, npair, nfine, nwin, delays.shape[0], nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, K_MAD)
        ffi.call("xengCutoutSetDelays", np.ascontiguousarray(delays, np.int32).ctypes.data_as(_pi))
        if weights is not None:
            self.set_weights(weights)
        assert _info() == (0, 0, self.ref.out_bytes)
        self.cuts = {}              # id -> (record bytes, W bytes, P bytes)
        self.expired = []

    def set_weights(self, w):
        w = np.ascontiguousarray(w, np.float32)
        ffi.call("xengCutoutSetWeights", w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        self.ref.set_weights(w)

    def request(self, rows):
        r = cutout_ref.requests(rows)
        ffi.call("xengCutoutRequest", r.size, r.ctypes.data)
        self.ref.request(r)

    def reset(self):
        ffi.call("xengCutoutReset")
        self.ref.reset()
        assert _info()[:2] == (0, 0)

    def run(self, x):
        nc = x.shape[0]
        sent = np.ascontiguousarray(x, np.float32)
        self.din.upload(sent)
        served, expired = _run(self.din.ptr, nc, self.dout.ptr + GUARD, self.nreq_max)
        ffi.call("xengCutoutSync")
        assert self.din.download(np.uint8, sent.nbytes).tobytes() == sent.tobytes(), "the input was written"
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.ref.out_bytes:] == POISON).all(), "bytes past the output were written"
        eserved, eexpired, exp = self.ref.run(sent, fill=POISON)
        assert (served, expired) == (eserved, eexpired)
        got = raw[GUARD:GUARD + self.ref.out_bytes]
        if exp is None:
            assert (got == POISON).all(), "a call that serves nothing wrote to the output"
        else:
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, "the output differs from byte %d on (%d bytes; records end at %d, waterfalls at %d)" % (
                bad[0], bad.size, self.ref.rec_bytes, self.ref.rec_bytes + self.nreq_max * self.ref.w_bytes)
            for z, rid in enumerate(served):
                rec, W, P = self.ref.last[z]
                self.cuts[rid] = (rec.tobytes(), W.tobytes(), P.tobytes())
            ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        self.expired += expired
        return served, expired

    def stream(self, x, sizes):
        n = 0
        for nc in sizes:
            self.run(x[n:n + nc])
            n += nc
        assert n == x.shape[0] and _info()[:2] == (self.ref.n, len(self.ref.pending))

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengCutoutCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengCutoutDestroy")
        self.din.free()
        self.dout.free()


SMALL = dict(npair=2, nfine=70, nwin=4, nband=7, nt=16, tscr=2, ndmc=5, nwidth=4, nreq_max=2)


def small_requests(ndmf):
    """(id, pair, n_c, ic, dstep) for nt 16, tscr 2 (ntu 32) over 150 windows of a 9-trial grid with S = 9: 100 begins before window
    0 (a(0) = -13: windows before 0 read +0); 101 and 102 have rows absent below and above the grid; 103, 104 and 105 fall due in
    the same call with nreq_max 2 (105 waits one call); 106 with dstep 3 has rows absent at both ends."""
    return [(100, 0, 3, 4, 1), (101, 1, 40, 0, 1), (102, 0, 44, ndmf - 1, 1), (103, 1, 80, 4, 1), (104, 0, 80, 4, 1), (105, 1, 80, 4, 1),
            (106, 0, 110, 4, 3)]


@pytest.mark.parametrize("shape", ["nband7_tscr2", "tight_calls_of_one", "nband70_tscr1_ndmc1_nwidth1", "nfine3_tscr64", "nt1024_ndmc256"])
def test_float_data_equal_the_restatement_byte_for_byte(shape):
    """nband7_tscr2: 2 pairs x 70 channels (three ingest tiles of 32, the last with 6 live channels), bands of 10, calls of 1..4
    windows, a ring of 52 slots that 150 windows wrap almost three times; a request that begins before window 0, rows absent at
    either end and at both, two requests in one call, one more than nreq_max due at once, one that has expired when it is asked
    for.  tight_calls_of_one: nhist = ntu + S exactly, a ring of 45 slots, calls of one window: a request whose plane reaches the
    largest delay can be served by exactly one call, the one that brings its last window.  nband70: one channel a band, no time
    scrunch, one row, one width.  nfine3_tscr64: ntu = 1024, an LDS sum of 64 words per column, 4 columns per work-group.
    nt1024_ndmc256: the largest plane, 4 KiB rows, 10 widths, 256 rows to pick from."""
    if shape == "nband7_tscr2":
        k = dict(SMALL)
        ndmf, S, total = 9, 9, 150
        reqs = small_requests(ndmf)
        late = [(107, 0, 30, 4, 1)]             # asked for at window ~100: first = 14 < n - 48
    elif shape == "tight_calls_of_one":
        k = dict(SMALL, nreq_max=1)
        ndmf, S, total = 9, 9, 150
        reqs, late = [(1, 0, 3, 8, 1), (2, 1, 50, 8, 1), (3, 0, 100, 2, 2)], []
    elif shape == "nband70_tscr1_ndmc1_nwidth1":
        k = dict(SMALL, nband=70, tscr=1, ndmc=1, nwidth=1)
        ndmf, S, total = 9, 9, 80
        reqs, late = [(1, 0, 20, 8, 1), (2, 1, 30, 0, 2), (3, 1, 5, 3, 1)], []
    elif shape == "nfine3_tscr64":
        k = dict(npair=1, nfine=3, nwin=40, nband=3, nt=16, tscr=64, ndmc=5, nwidth=4, nreq_max=1)
        ndmf, S, total = 6, 50, 2300
        reqs, late = [(7, 0, 600, 2, 1), (8, 0, 1100, 5, 2)], []
    else:
        k = dict(npair=1, nfine=3, nwin=40, nband=1, nt=1024, tscr=1, ndmc=256, nwidth=10, nreq_max=1)
        ndmf, S, total = 300, 60, 1400
        reqs, late = [(9, 0, 700, 140, 1)], []
    delays = cutout_cases.table(ndmf, k['nfine'], S)
    # ntu + S windows hold a cut-out; a request is served for certain if the history has nwin - 1 more (the call that brings its
    # last window may bring nwin - 1 after it), and nwin more again if it may have to wait a call for a free slot
    nhist = k['nt'] * k['tscr'] + S + (0 if shape == "tight_calls_of_one" else 2 * k['nwin'] - 1)
    x = cutout_cases.float_scene(len(shape), total, k['npair'], k['nfine'])
    sizes = cutout_cases.random_sizes(3, total, k['nwin']) if k['nwin'] == 4 else cutout_cases.whole(total, k['nwin'])
    if shape == "tight_calls_of_one":
        sizes = [1] * total
    co = CO(delays=delays, nhist=nhist, **k)
    try:
        co.request(reqs)
        n = 0
        for nc in sizes:
            if late and n >= 100:
                co.request(late)
                late = []
            co.run(x[n:n + nc])
            n += nc
        assert sorted(co.cuts) == sorted(r[0] for r in reqs) and co.expired == ([107] if shape == "nband7_tscr2" else [])
        assert all(np.frombuffer(c[0], cutout_ref.RECORD)[0]['status'] == 0 for c in co.cuts.values())
        assert _info()[:2] == (total, 0)
    finally:
        co.close()


def test_three_splits_give_the_same_cut_outs_and_a_reset_is_a_fresh_context():
    """The small shape: calls of 4, of 1 and of 1..4 windows serve the requests in different calls (and at nreq_max 2 in different
    slots) and give the same bytes per request; after a prefix of other data and a Reset the run equals a fresh context's."""
    ndmf, S, total = 9, 9, 150
    delays = cutout_cases.table(ndmf, 70, S)
    x = cutout_cases.float_scene(21, total, 2, 70)
    runs = []
    for sizes in (cutout_cases.whole(total, 4), [1] * total, cutout_cases.random_sizes(8, total, 4)):
        co = CO(delays=delays, nhist=32 + S + 7, **SMALL)
        try:
            co.request(small_requests(ndmf))
            co.stream(x, sizes)
            runs.append(co.cuts)
        finally:
            co.close()
    assert len(runs[0]) == 7 and runs[0] == runs[1] == runs[2]
    co = CO(delays=delays, nhist=32 + S + 7, **SMALL)
    try:
        co.request([(1, 0, 20, 4, 1), (2, 0, 400, 4, 1)])
        co.stream(cutout_cases.float_scene(22, 47, 2, 70), cutout_cases.whole(47, 4))
        assert 1 in co.cuts and _info()[1] == 1
        co.reset()                              # (request 2 is dropped)
        co.cuts = {}
        co.request(small_requests(ndmf))
        co.stream(x, cutout_cases.random_sizes(9, total, 4))
        assert co.cuts == runs[0]
    finally:
        co.close()


def test_a_left_out_channel_with_nan_rows_without_a_score_and_heavy_ties():
    """The small shape with one pair's worth of special data.  Channel 11 holds NaN throughout and has weight 0: nothing of it
    arrives (request 1 is scored).  Then the weight is 1 again, on the history held: every row of request 2 has a NaN, status 1,
    S0 = +0.  Request 3: one NaN in channel 0 at the last window that only the highest trial's row needs: that row alone has no
    score.  Pair 1 is constant: A = 0, no row is valid (request 4).  Request 5 on data of two values (0 and 1 in one channel, 0
    elsewhere): heavy ties, decided by the smallest i, iw, j.  All equal the restatement (CO.run compares)."""
    ndmf, S, total = 9, 9, 150
    k = dict(SMALL, nreq_max=1)
    delays = cutout_cases.table(ndmf, 70, S)
    x = cutout_cases.float_scene(33, total, 2, 70)
    x[:, 1] = 3.0
    x[:, 0, 11] = np.nan
    x[96:, 0] = 0                               # from window 96 on pair 0 holds two values
    x[96:, 0, 5, 0] = (np.arange(total - 96) % 4 == 0)
    n3 = 70
    x[n3 - 16 + 31 + int(delays[8, 0]), 0, 0, 1] = np.nan
    assert delays[8, 0] > delays[7, 0]
    w = np.ones(70, np.float32)
    w[11] = 0
    co = CO(delays=delays, nhist=32 + S + 3, weights=w, **k)
    try:
        co.request([(1, 0, 20, 4, 1)])
        co.stream(x[:48], cutout_cases.whole(48, 4))
        assert np.frombuffer(co.cuts[1][0], cutout_ref.RECORD)[0]['status'] == 0
        w[11] = 1
        co.set_weights(w)
        co.request([(2, 0, 24, 4, 1)])
        co.run(x[48:52])
        rec = np.frombuffer(co.cuts[2][0], cutout_ref.RECORD)[0]
        assert rec['status'] == 1 and rec['S0'] == 0 and rec['i'] == -1
        w[11] = 0
        co.set_weights(w)
        co.request([(3, 0, n3, 6, 1), (4, 1, 60, 4, 1), (5, 0, 125, 4, 1)])
        co.stream(x[52:], cutout_cases.whole(total - 52, 4))
        rec = np.frombuffer(co.cuts[3][0], cutout_ref.RECORD)[0]
        P = np.frombuffer(co.cuts[3][2], np.float32).reshape(5, 16)
        assert rec['status'] == 0 and np.isnan(P[4]).any() and np.isfinite(P[:4]).all() and rec['i'] < 4
        assert np.frombuffer(co.cuts[4][0], cutout_ref.RECORD)[0]['status'] == 1
        rec = np.frombuffer(co.cuts[5][0], cutout_ref.RECORD)[0]
        assert rec['status'] == 0 and rec['S'] > 0
    finally:
        co.close()


def test_integer_data_equal_the_float64_statement():
    """Integer noise and a pulse of 2 windows x 25 per channel planted at fine trial 3 of 5 (S = 16: four windows a trial at the
    lowest channel) on a column of its own: W and P equal cutout_reference's float64 sums word for word (every sum is an integer
    below 2^24), and so do M, A, i, iw and j; S and S0 to the three roundings that form them (2^-22).  The float64 statement gives
    S = 19.80 at (i, iw, j) = (3, 0, 8) against S0 = 14.85 at the centre trial."""
    ndmf, S, total = 5, 16, 120
    delays = cutout_cases.table(ndmf, 70, S)
    x = cutout_cases.integer_scene(4, total, 2, 70)
    cutout_cases.plant(x, 1, delays[3], 61, 25.0, width=2)
    co = CO(delays=delays, nhist=32 + S + 7, **SMALL)
    try:
        co.request([(1, 1, 61, 2, 1)])
        co.stream(x, cutout_cases.random_sizes(5, total, 4))
        rec = np.frombuffer(co.cuts[1][0], cutout_ref.RECORD)[0]
        e = cutout_reference(x, delays, 1, 61, 2, 1, 7, 16, 2, 5, 4, K_MAD)
        assert np.array_equal(np.frombuffer(co.cuts[1][1], np.float32).reshape(7, 16).astype(np.float64), e['W'])
        assert np.array_equal(np.frombuffer(co.cuts[1][2], np.float32).reshape(5, 16).astype(np.float64), e['P'])
        assert (rec['i'], rec['iw'], rec['j'], float(rec['M']), float(rec['A'])) == (e['i'], e['iw'], e['j'], e['M'], e['A']) == (3, 0, 8, 2685.5, 113.5)
        assert abs(rec['S'] - e['S']) <= 2.0 ** -22 * e['S'] and abs(rec['S0'] - e['S0']) <= 2.0 ** -22 * abs(e['S0'])
        assert rec['S'] > rec['S0'] > 0
    finally:
        co.close()


def test_refusals():
    L = ffi.lib()
    good = dict(npair=2, nfine=8, nwin=4, ndmf=3, nhist=40, nband=2, nt=16, tscr=2, ndmc=3, nwidth=2, nreq_max=2, k_mad=1.0)

    def init(**kw):
        a = dict(good, **kw)
        return L.xengCutoutInitialize(0, a['npair'], a['nfine'], a['nwin'], a['ndmf'], a['nhist'], a['nband'], a['nt'], a['tscr'], a['ndmc'], a['nwidth'],
                                      a['nreq_max'], ctypes.c_float(a['k_mad']))

    L.xengCutoutDestroy()
    assert init() == 0
    try:
        buf = ffi.DeviceBuffer(1 << 16)
        ns, ne = ctypes.c_int(-7), ctypes.c_int(-7)
        ids, ex = (ctypes.c_int * 2)(), (ctypes.c_int * 1024)()
        r = cutout_ref.requests([(1, 0, 20, 1, 1)])
        assert L.xengCutoutRequest(1, r.ctypes.data) == INVALID_STATE                  # (no table yet)
        assert L.xengCutoutRun(buf.ptr, 1, buf.ptr, ctypes.byref(ns), ids, ctypes.byref(ne), ex) == INVALID_STATE
        bad = np.zeros((3, 8), np.int32)
        bad[2, 0] = 9                           # (9 + ntu = 41 > nhist)
        assert L.xengCutoutSetDelays(bad.ctypes.data_as(_pi)) == INVALID_ARGUMENT
        bad[2, 0] = -1
        assert L.xengCutoutSetDelays(bad.ctypes.data_as(_pi)) == INVALID_ARGUMENT
        bad[2, 0] = 8
        assert L.xengCutoutSetDelays(bad.ctypes.data_as(_pi)) == 0
        for row in ((1, 2, 20, 1, 1), (1, -1, 20, 1, 1), (1, 0, 20, 3, 1), (1, 0, 20, -1, 1), (1, 0, -1, 1, 1), (1, 0, 20, 1, 0)):
            r = cutout_ref.requests([(5, 0, 20, 1, 1), row])
            assert L.xengCutoutRequest(2, r.ctypes.data) == INVALID_ARGUMENT, row
        assert _info()[1] == 0                  # (none of a refused call's requests is taken)
        r = cutout_ref.requests([(5, 0, 4, 1, 1)])
        assert L.xengCutoutRequest(1, r.ctypes.data) == 0
        for args in ((None, 1, buf.ptr), (buf.ptr + 4, 1, buf.ptr), (buf.ptr, 1, buf.ptr + 8), (buf.ptr, 0, buf.ptr), (buf.ptr, 5, buf.ptr)):
            assert L.xengCutoutRun(*args, ctypes.byref(ns), ids, ctypes.byref(ne), ex) == INVALID_ARGUMENT
        ffi.call("xengMemset", buf.ptr, 0, buf.nbytes)
        for _ in range(6):                      # windows 0..23: the request needs windows -12..27
            assert L.xengCutoutRun(buf.ptr, 4, None, ctypes.byref(ns), ids, ctypes.byref(ne), ex) == 0 and ns.value == 0
        assert L.xengCutoutRun(buf.ptr, 4, None, ctypes.byref(ns), ids, ctypes.byref(ne), ex) == INVALID_ARGUMENT    # (it would serve)
        assert _info()[:2] == (24, 1)
        assert L.xengCutoutRun(buf.ptr, 4, buf.ptr + 4096, ctypes.byref(ns), ids, ctypes.byref(ne), ex) == 0 and ns.value == 1 and ids[0] == 5
        ffi.call("xengCutoutSync")
        buf.free()
    finally:
        ffi.call("xengCutoutDestroy")


def test_dedisperse_search_and_cut_out_on_the_device():
    """1 pair x 64 channels, integer noise and a pulse planted at fine trial 14, midway between search trials 3 and 4 (nsplit 4).
    xengDedispRun writes a device buffer, xengPulseRun reads it; the host groups the record plane (pulse_candidates), makes the
    request (cutout_requests, the nearest fine trial), and xengCutoutRun, fed the same input spans, serves it a few spans later.
    The search's own answer is coarse -- the pulse shows in more than one span, at search trials 4 and 5 and up to 13 windows off --
    and every cut-out (17 fine trials x 64 windows around it) names fine trial 14 and window 200, above its centre row."""
    npair, nfine, nwin, nstat, nwidth_s = 1, 64, 16, 32, 4
    dms = np.arange(8.0)
    fine = cutout_fine_dms(dms, 4)
    freqs = 60e6 + (20e6 / nfine) * np.arange(nfine)
    tsamp = 0.0045 * 7
    ds, df = dm_delays(freqs, dms, tsamp), dm_delays(freqs, fine, tsamp)
    S = int(ds.max())
    assert df.shape[0] == 29 and S == int(df.max()) and 100 <= S <= 120 and not np.array_equal(df[13], df[14]) and not np.array_equal(df[14], df[15])
    total, n_top = 22 * nwin, 200
    x = cutout_cases.integer_scene(6, total, npair, nfine)
    cutout_cases.plant(x, 0, df[14], n_top, 100.0)
    nt, tscr, ndmc, nband, nwidth, nreq_max = 64, 1, 17, 8, 3, 2
    nhist = nt * tscr + S + 3 * nwin
    trust = (-(-S // nstat) + 1) * nstat
    ref = cutout_ref.CutoutRef(npair, nfine, nwin, df, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, K_MAD)
    din = ffi.DeviceBuffer(nwin * npair * nfine * 16)
    dy = ffi.DeviceBuffer(nwin * npair * 8 * 4)
    drec = ffi.DeviceBuffer(npair * 8 * 16)
    dout = ffi.DeviceBuffer(ref.out_bytes)
    ffi.call("xengDedispInitialize", 0, npair, nfine, nwin, 8, S, 1)
    ffi.call("xengDedispSetDelays", np.ascontiguousarray(ds).ctypes.data_as(_pi))
    ffi.call("xengPulseInitialize", 0, npair, 8, nwin, 1, nwidth_s, nstat)
    ffi.call("xengCutoutInitialize", 0, npair, nfine, nwin, 29, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, K_MAD)
    ffi.call("xengCutoutSetDelays", np.ascontiguousarray(df).ctypes.data_as(_pi))
    try:
        found, asked = [], []
        for j in range(total // nwin):
            span = np.ascontiguousarray(x[j * nwin:(j + 1) * nwin])
            din.upload(span)
            ffi.call("xengDedispRun", din.ptr, nwin, dy.ptr)
            ffi.call("xengPulseRun", dy.ptr, nwin, drec.ptr)
            served, expired = _run(din.ptr, nwin, dout.ptr, nreq_max)
            ffi.call("xengCutoutSync")
            es, ee, exp = ref.run(span, fill=0)
            assert (served, expired) == (es, ee)
            if served:
                rec = dout.download(np.uint8)[:32 * nreq_max].view(cutout_ref.RECORD)
                assert rec.tobytes() == exp[:32 * nreq_max].tobytes()
                found += [rec[z].copy() for z in range(len(served))]
            plane = drec.download(np.uint8).view(PULSE_RECORD).reshape(npair, 8)
            cands = pulse_candidates(plane, 8.0, dms, [1 << i for i in range(nwidth_s)])
            # (BeamPulseSearch's rule: a boxcar that begins before the first block measured on whole sums is left out)
            cands = [c for c in cands if j * nwin + c['window'] - c['width'] + 1 >= trust]
            for c in cutout_requests(cands, j * nwin, S, 1, first_id=len(asked)):
                ic = int(np.argmin(np.abs(fine - c['dm'])))
                r = cutout_ref.requests([(c['id'], c['pair'], c['seq'], ic, 1)])
                ffi.call("xengCutoutRequest", 1, r.ctypes.data)
                ref.request(r)
                asked.append((ic, c['seq']))
        assert asked and len(found) == len(asked) and all(abs(ic - 14) <= 8 and abs(seq - n_top) <= 16 for ic, seq in asked)
        for (ic, seq), rec in zip(asked, found):
            assert rec['status'] == 0 and ic + (rec['i'] - ndmc // 2) == 14 and rec['iw'] == 0 and seq - nt // 2 + rec['j'] == n_top
            assert rec['S'] > rec['S0'] > 0
    finally:
        for name in ("Cutout", "Pulse", "Dedisp"):
            ffi.call("xeng%sDestroy" % name)
        for b in (din, dy, drec, dout):
            b.free()
