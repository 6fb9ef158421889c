"""BeamPulseCutout without a GPU: the host helpers (cutout_fine_dms, cutout_plan, cutout_requests, CutoutQueue, cutout_refined), the
CUTOUT_ENGINES row under the per-row checks of tests/test_engine_table_cpu.py, the C entry points' argument checks, the block on
CPU rings with a backend that serves xengCutout* by the restatement (tests/cutout_ref.py) -- a request served spans later, two
served in one call, more than nreq_max due at once, one expired, one before the sequence, one dropped by a gap, the header -- and a
planted scene on integer data: the restatement against the float64 statement (cutout_reference)."""
import ctypes

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import (CUTOUT_RECORD, CUTOUT_REQUEST, BeamPulseCutout, CutoutQueue, as_cutouts, cutout_fine_dms, cutout_k_mad,
                                            cutout_offsets, cutout_plan, cutout_reference, cutout_refined, cutout_requests, dm_delays)
from caltech_bifrost_dsp_amd.ring import Ring
from tests import cutout_cases, cutout_ref, test_engine_table_cpu
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink
from tests.test_dedisp_cpu import header_table, power_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2
F = np.float32
K_MAD = cutout_cases.K_MAD


# ---------------------------------------------------------------- the host helpers
def test_fine_grid_plan_requests_and_records():
    fine = cutout_fine_dms([0.0, 1.0, 3.0], 4)
    assert fine.tolist() == [0, 0.25, 0.5, 0.75, 1, 1.5, 2, 2.5, 3] and cutout_fine_dms([2.0, 4.0], 1).tolist() == [2, 4]
    for bad in (([1.0], 2), ([0.0, 0.0], 2), ([0.0, 1.0], 0), ([-1.0, 1.0], 2), ([0.0, float('nan')], 2)):
        with pytest.raises(ValueError):
            cutout_fine_dms(*bad)
    assert CUTOUT_RECORD == cutout_ref.RECORD and CUTOUT_REQUEST == cutout_ref.REQUEST and cutout_k_mad() == K_MAD
    freqs = 60e6 + (20e6 / 64) * np.arange(64)
    tsamp = 0.063
    fine = cutout_fine_dms([0.0, 2.0, 4.0, 6.0], 2)
    S = int(dm_delays(freqs, fine, tsamp).max())
    p = cutout_plan(freqs, fine, tsamp, widest=8, dm_span=4.0, nt=32, late=12)
    sweep = int(dm_delays(freqs, [2.0], tsamp).max())
    assert (S, sweep) == (48, 16) and p == dict(nt=32, tscr=2, ntu=64, ndmc=5, dstep=1, nhist=64 + S + 12, S=S)      # (4 x 16 = 64 = 8 x 8 windows)
    assert cutout_plan(freqs, fine, tsamp, widest=100, dm_span=1.0, nt=16)['tscr'] == 64                               # (800 windows: the largest scrunch)
    with pytest.raises(ValueError):
        cutout_plan(freqs, fine, tsamp, widest=8, dm_span=4.0, nt=15)
    # a boxcar of 4 windows that ends at window 9 of the span at sample 1000, latency 5, 32 samples a window: the pulse stands at
    # window 4 at the top of the band, the boxcar's middle 1.5 windows earlier
    r, = cutout_requests([dict(pair=1, idm=2, dm=4.0, snr=9.0, window=9, iw=2, width=4, ntrial=1)], 1000, 5, 32, first_id=7)
    assert r == dict(id=7, pair=1, dm=4.0, seq=1000 + 4 * 32 - 48)
    rec = np.array([(7, 0, 9.5, 3.0, 3, 1, 17, 0, 100.0, 5.0)], CUTOUT_RECORD)[0]
    out = cutout_refined(rec, fine, ic=2, dstep=1, ndmc=5, nt=32, tscr=2, seq_c=5000, acc_len=32)
    # row 3 is fine trial 3; width 2 columns x 2; columns 16..17 = windows [32, 36) of 64, the middle 2 windows after the centre
    assert out == dict(id=7, dm=3.0, idm_fine=3, width=4, seq=5000 + 2 * 32, snr=9.5, snr0=3.0)
    assert cutout_refined(np.array([cutout_ref.EMPTY], CUTOUT_RECORD)[0], fine, 2, 1, 5, 32, 2, 0, 32) is None
    a, b, n = cutout_offsets(2, 7, 16, 5)
    assert (a, b, n) == (64, 64 + 2 * 7 * 16 * 4, 64 + 2 * (7 + 5) * 16 * 4)
    with pytest.raises(ValueError):
        as_cutouts(np.zeros(n + 1, np.uint8), 2, 7, 16, 5)


def test_the_queue_is_the_restatements_serving_rule():
    delays = cutout_cases.table(9, 8, 9)
    q = CutoutQueue(delays, nhist=48, ntu=32, ndmc=5, nreq_max=2)
    ref = cutout_ref.CutoutRef(1, 8, 4, delays, 48, 2, 16, 2, 5, 2, 2, K_MAD)
    rows = [(1, 0, 3, 4, 1), (2, 0, 40, 0, 1), (3, 0, 80, 4, 1), (4, 0, 80, 4, 1), (5, 0, 80, 4, 1), (6, 0, 110, 4, 3)]
    for r in rows:
        q.add(*r)
    ref.request(rows)
    x = cutout_cases.integer_scene(1, 160, 1, 8)
    n = 0
    for k, nc in enumerate(cutout_cases.random_sizes(2, 160, 4)):
        if k == 30:
            q.add(9, 0, 20, 4, 1)
            ref.request([(9, 0, 20, 4, 1)])
        served, expired, _ = ref.run(x[n:n + nc])
        assert q.take(nc) == (served, expired)
        n += nc
    assert not q.pending and q.reset() == 0


# ---------------------------------------------------------------- the engine table and the C entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.CUTOUT_ENGINES == [("Cutout", "cutout", True)]
    older = ffi.ENGINES + ffi.MORE_ENGINES + ffi.NEWER_ENGINES + ffi.NEWEST_ENGINES + ffi.LATEST_ENGINES + ffi.FURTHER_ENGINES
    assert not {r[0] for r in ffi.CUTOUT_ENGINES} & {r[0] for r in older} and not {r[1] for r in ffi.CUTOUT_ENGINES} & {r[1] for r in older}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.CUTOUT_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.CUTOUT_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    L = ffi.lib()
    names = ["xengCutout" + n for n in ("Initialize", "SetDelays", "SetWeights", "Request", "Run", "Reset", "GetInfo", "CheckGuards", "Mark", "Wait",
                                        "TicketDone", "Sync", "Destroy")]
    for name in names:
        assert hasattr(L, name) and name in ffi.SYMBOLS and name in test_engine_table_cpu.DECLARED, name
        assert (name in ffi.ENQUEUE_ONLY) == (name[10:] in ("Run", "Reset", "Request", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_delays", "set_weights", "request", "run", "reset", "info", "guards_intact", "mark", "wait", "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "cutout_" + m)), m
    # (npair, nfine, nwin, ndmf, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, k_mad)
    good = [2, 8, 4, 3, 40, 2, 16, 2, 3, 2, 2, 1.0]
    for i, v in ((0, 0), (0, 65536), (1, 0), (2, 0), (3, 0), (4, 31), (5, 0), (5, 3), (5, 257), (6, 14), (6, 17), (6, 1026), (7, 0), (7, 3), (7, 128), (8, 0),
                 (8, 257), (9, 0), (9, 5), (9, 11), (10, 0), (10, 65), (11, 0.0), (11, -1.0), (11, float('nan')), (11, float('inf'))):
        args = list(good)
        args[i] = v
        assert L.xengCutoutInitialize(0, *args[:11], ctypes.c_float(args[11])) == INVALID_ARGUMENT, args
    assert L.xengCutoutInitialize(0, 16, 1 << 16, 4, 3, 1020, 2, 16, 2, 3, 2, 2, ctypes.c_float(1.0)) == INVALID_ARGUMENT   # exactly 2^32 bytes
    assert b"history" in L.xengGetLastError()
    assert L.xengCutoutInitialize(0, 1, 1 << 15, 4, (1 << 13) + 1, 40, 2, 16, 2, 3, 2, 2, ctypes.c_float(1.0)) == INVALID_ARGUMENT    # a table above 2^28 words
    if not _gpu_present():
        assert L.xengCutoutInitialize(0, *good[:11], ctypes.c_float(good[11])) not in (0, INVALID_ARGUMENT)    # (good sizes get as far as the device)
    ns, ne = ctypes.c_int(-1), ctypes.c_int(-1)
    ids = (ctypes.c_int * 1024)()
    for args in ((None, 1, 16, ctypes.byref(ns), ids, ctypes.byref(ne), ids), (16, 1, 16, None, ids, ctypes.byref(ne), ids),
                 (16, 1, 16, ctypes.byref(ns), None, ctypes.byref(ne), ids), (16, 1, 16, ctypes.byref(ns), ids, None, ids),
                 (16, 1, 16, ctypes.byref(ns), ids, ctypes.byref(ne), None), (20, 1, 16, ctypes.byref(ns), ids, ctypes.byref(ne), ids),
                 (16, 1, 24, ctypes.byref(ns), ids, ctypes.byref(ne), ids)):
        assert L.xengCutoutRun(*args) == INVALID_ARGUMENT
    assert L.xengCutoutGetInfo(None, None, None) == INVALID_ARGUMENT and L.xengCutoutSetDelays(None) == INVALID_ARGUMENT
    assert L.xengCutoutRequest(1, None) == INVALID_ARGUMENT and L.xengCutoutRequest(-1, None) == INVALID_ARGUMENT
    if not _gpu_present():
        n, k = ctypes.c_longlong(), ctypes.c_int()
        r = cutout_ref.requests([(1, 0, 20, 1, 1)])
        t = np.zeros((3, 8), np.int32)
        assert L.xengCutoutRun(16, 1, None, ctypes.byref(ns), ids, ctypes.byref(ne), ids) == INVALID_STATE and L.xengCutoutReset() == INVALID_STATE
        assert L.xengCutoutRequest(1, r.ctypes.data) == INVALID_STATE and L.xengCutoutSetWeights(None) == INVALID_STATE
        assert L.xengCutoutSetDelays(t.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == INVALID_STATE
        assert L.xengCutoutGetInfo(ctypes.byref(n), ctypes.byref(k), ctypes.byref(n)) == INVALID_STATE and (ns.value, ne.value) == (-1, -1)


# ---------------------------------------------------------------- the block on CPU rings
class CutoutBackend(OracleBackend):
    """The oracle backend plus xengCutout* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.co, self.calls, self.k = None, [], None

    def cutout_initialize(self, gpu, npair, nfine, nwin, ndmf, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, k_mad):
        self.k = dict(npair=npair, nfine=nfine, nwin=nwin, nhist=nhist, nband=nband, nt=nt, tscr=tscr, ndmc=ndmc, nwidth=nwidth, nreq_max=nreq_max, k_mad=k_mad)
        self.ndmf, self.w = ndmf, None
        self.calls.append(('init', nhist, k_mad))
        return 0

    def cutout_set_delays(self, delays):
        assert delays.dtype == np.int32 and delays.shape == (self.ndmf, self.k['nfine']) and delays.flags.c_contiguous
        if delays.min() < 0 or delays.max() + self.k['nt'] * self.k['tscr'] > self.k['nhist']:
            return INVALID_ARGUMENT
        self.co = cutout_ref.CutoutRef(delays=delays, weights=self.w, **self.k)
        self.calls.append('set_delays')
        return 0

    def cutout_set_weights(self, weights):
        self.w = None if weights is None else weights.copy()
        if self.co is not None:
            self.co.set_weights(self.w)
        self.calls.append('set_weights')
        return 0

    def cutout_request(self, reqs):
        assert reqs.dtype == CUTOUT_REQUEST
        self.co.request(reqs)
        self.calls.append(('request', reqs['id'].tolist()))
        return 0

    def cutout_run(self, in_arr, nwin_call, out_arr, nreq_max):
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, self.k['npair'], self.k['nfine'], 4)
        served, expired, out = self.co.run(x, fill=0)
        if served:
            if out_arr is None:
                return INVALID_ARGUMENT, [], []
            out_arr.numpy().reshape(-1).view(np.uint8)[...] = out
        self.calls.append('run')
        return 0, served, expired

    def cutout_reset(self):
        self.co.reset()
        self.calls.append('reset')

    def cutout_mark(self):
        return self.beam_mark()

    def cutout_wait(self, ticket):
        self.beam_wait(ticket)

    def cutout_sync(self):
        pass


NWIN, ACC = 4, 32
FINE = cutout_fine_dms([0.0, 0.05, 0.1, 0.2], 2)
BLK = dict(npair=2, nchan=2, nupchan=4, nwin=NWIN, fine_dms=FINE, nband=2, nt=16, tscr=1, ndmc=3, nwidth=2, nreq_max=2)


def _block(spans, hdr, nhist, got, be=None, **kw):
    be = be or CutoutBackend()
    r1 = Ring("co-output")
    span = NWIN * 2 * 8 * 16
    blk = BeamPulseCutout(LOG, _FakeRing([_FakeSeq(hdr, spans, span)]), r1, nhist=nhist, backend=be, on_cutout=got.extend, **dict(BLK, **kw))
    sink = Sink(r1, cutout_offsets(2, 2, 16, 3)[2])
    return blk, be, sink


def test_block_serves_spans_later_two_in_a_call_one_too_many_one_expired_and_one_before_the_sequence():
    """30 spans of 4 windows from sample 6400, S = 6, nhist = 16 + 6 + 7.  Request 1 (window 30) is served by the span that brings
    window 30 + 7 + 6; 2 and 3 (window 60) by one call; 4, 5 and 6 (window 90) fall due together: two in one call, the third in the
    next; 7 lies before the sequence (counted, never given to the library); 8 is asked for from the callback of request 1, for
    window 9, whose first window has left the history by then: the library reports it expired at the next call."""
    seq0 = 6400
    hdr = power_header(2, 2, 4, 8, seq0=seq0)
    table, tsamp = header_table(hdr, 8, FINE)
    S = int(table.max())
    assert S == 6
    x = cutout_cases.integer_scene(3, 30 * NWIN, 2, 8)
    spans = [(k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])) for k in range(30)]
    got = []
    blk, be, sink = _block(spans, hdr, 16 + S + 7, got)

    def on_cutout(cuts):
        got.extend(cuts)
        if cuts[0]['id'] == 1:
            blk.request([dict(id=8, pair=0, dm=0.0, seq=seq0 + 9 * ACC)])
    blk.on_cutout = on_cutout
    at = lambda n: seq0 + n * ACC + 5            # (a sample inside window n)
    blk.request([dict(id=1, pair=0, dm=0.1, seq=at(30)), dict(id=2, pair=1, dm=0.1, seq=at(60)), dict(id=3, pair=0, dm=0.1, seq=at(60)),
                 dict(id=4, pair=0, dm=0.1, seq=at(90)), dict(id=5, pair=1, dm=0.1, seq=at(90)), dict(id=6, pair=1, dm=0.11, seq=at(90)),
                 dict(id=7, pair=0, dm=0.1, seq=seq0 - 1)])
    sink.start()
    blk.main()
    sink.join(20)
    (hd, tag, out), = sink.sequences
    assert [c['id'] for c in got] == [1, 2, 3, 4, 5, 6] and len(out) == 4
    assert blk.stats['nserved'] == 6 and blk.stats['nexpired'] == 2 and blk.stats['npending'] == 0 and blk.stats['ndropped'] == 0
    assert blk.stats['nwindow'] == 120 and blk.stats['ngap'] == 0
    assert be.calls[:4] == [('init', 16 + S + 7, cutout_k_mad()), 'set_delays', ('request', [1, 2, 3, 4, 5, 6]), 'run']
    assert ('request', [8]) in be.calls and be.calls.count('run') == 30
    # the spans are the restatement's: records, waterfalls, planes at the header's offsets
    assert (hd['cutout'], hd['nband'], hd['nt'], hd['tscr'], hd['ndmc'], hd['nwidth'], hd['nreq_max'], hd['dstep']) == (True, 2, 16, 1, 3, 2, 2, 1)
    assert hd['fine_dms'] == FINE.tolist() and hd['tsamp'] == tsamp and (hd['record_offset'], hd['waterfall_offset'], hd['plane_offset']) == (0, 64, 64 + 2 * 2 * 16 * 4)
    assert hd['span_bytes'] == out[0].size and tag == hd['seq0'] == seq0
    rec, W, P = as_cutouts(out[1], 2, 2, 16, 3)
    assert rec['id'].tolist() == [2, 3] and np.array_equal(W[0], got[1]['waterfall']) and np.array_equal(P[1], got[2]['plane'])
    rec, W, P = as_cutouts(out[3], 2, 2, 16, 3)
    assert rec['id'].tolist() == [6, -1] and not W[1].any() and not P[1].any()
    # request 1: fine trial 4 (DM 0.1), rows at trials 3, 4, 5; the plane is the float64 statement of the same windows
    e = cutout_reference(x, table, 0, 30, 4, 1, 2, 16, 1, 3, 2, cutout_k_mad())
    assert np.array_equal(got[0]['plane'].astype(np.float64), e['P']) and np.array_equal(got[0]['waterfall'].astype(np.float64), e['W'])
    assert got[0]['seq'] == at(30) and got[0]['dm'] == 0.1 and got[5]['dm'] == 0.11
    r = got[0]['refined']
    assert (got[0]['record']['i'], got[0]['record']['iw'], got[0]['record']['j']) == (e['i'], e['iw'], e['j'])
    assert r['dm'] == FINE[4 + e['i'] - 1] and r['width'] == 1 << e['iw'] and abs(r['snr'] - e['S']) <= 2.0 ** -22 * abs(e['S'])


def test_block_gap_resets_and_drops_what_was_pending():
    """Spans 0..9 and 12..29 (10 and 11 never read): request 1 is served before the gap; request 2, for a window after it, is
    dropped by it (the window count starts again: its window means nothing now); request 3, asked for after the gap for a sample
    64 windows behind it, counts from the gap."""
    seq0 = 0
    hdr = power_header(2, 2, 4, 8, seq0=seq0)
    x = cutout_cases.integer_scene(4, 30 * NWIN, 2, 8)
    spans = [(k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])) for k in list(range(10)) + list(range(12, 30))]
    got = []
    blk, be, sink = _block(spans, hdr, 16 + 6 + 7, got)

    def on_cutout(cuts):
        got.extend(cuts)
        if cuts[0]['id'] == 1:
            blk.request([dict(id=2, pair=0, dm=0.1, seq=70 * ACC)])
    blk.on_cutout = on_cutout
    blk.request([dict(id=1, pair=1, dm=0.05, seq=12 * ACC), dict(id=3, pair=1, dm=0.05, seq=(48 + 40) * ACC)])
    sink.start()
    blk.main()
    sink.join(20)
    assert [c['id'] for c in got] == [1] and blk.stats['ndropped'] == 2 and blk.stats['ngap'] == 1 and blk.stats['nserved'] == 1
    assert be.calls.count('reset') == 1 and [len(q[2]) for q in sink.sequences] == [1, 0] and blk.stats['npending'] == 0     # (the output restarts after the gap)


@pytest.mark.parametrize("kw", [dict(npair=0), dict(nband=3), dict(nband=0), dict(tscr=3), dict(tscr=128), dict(nt=15), dict(nt=14), dict(nt=1026), dict(ndmc=0),
                                dict(ndmc=257), dict(nwidth=0), dict(nwidth=5), dict(nreq_max=0), dict(nreq_max=65), dict(nhist=15), dict(fine_dms=[]),
                                dict(fine_dms=[-1.0]), dict(k_mad=0.0), dict(nwin=2.0), dict(dstep=0), dict(on_cutout=3), dict(weights=[1.0])])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(BLK, nhist=40)
    args.update(kw)
    be = CutoutBackend()
    with pytest.raises(ValueError, match="BEAM_PULSE_CUTOUT"):
        BeamPulseCutout(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.k is None


def test_block_refuses_a_dedispersed_ring_and_a_grid_beyond_the_history():
    hdr = power_header(2, 2, 4, 8)
    x = cutout_cases.integer_scene(5, NWIN, 2, 8)
    for h, nhist, msg in ((dict(hdr, ndm=4), 40, "dedispersed"), (hdr, 16 + 5, "nhist")):
        blk, _, _ = _block([(0, x)], h, nhist, [])
        with pytest.raises(ValueError, match=msg):
            blk.main()


# ---------------------------------------------------------------- the planted scene
def test_planted_scene_the_restatement_equals_the_float64_statement_and_names_the_planted_trial():
    """1 pair x 64 channels of 60 to 80 MHz, windows of 63 ms: the search grid is DM 0, 2, 4, 6 and the fine grid cuts every interval
    in two (delays of 0, 8, 16 .. 48 windows at the lowest channel).  Seeded integer noise, uniform in 0..19 per hand, and a pulse
    of 2 windows x 8 per channel at DM 3 -- midway between the search trials 2 and 4 -- that reaches the top of the band at window
    70.  The request is the search's: fine trial 2 (DM 2) at window 70, five rows one fine trial apart, 32 columns, three widths.
    cutout_reference gives, for amplitudes 4, 6, 8 and 12, S = 6.03, 8.53, 11.02 and 16.00 at (i, iw, j) = (3, 1, 17) -- fine trial
    3, two windows, ending one after the centre column -- against S0 = 2.73, 3.22, 3.78 and 4.72 at the centre row, with M = 1246
    and A = 49.  The test plants 8.  The restatement equals it word for word in W, P, M, A, i, iw and j (every sum is an integer
    below 2^24) and in S and S0 to the three roundings that form them."""
    nfine, total, n_top = 64, 160, 70
    freqs = 60e6 + (20e6 / nfine) * np.arange(nfine)
    fine = cutout_fine_dms([0.0, 2.0, 4.0, 6.0], 2)
    df = dm_delays(freqs, fine, 0.063)
    assert df[:, 0].tolist() == [0, 8, 16, 24, 32, 40, 48]
    x = cutout_cases.integer_scene(11, total, 1, nfine)
    cutout_cases.plant(x, 0, df[3], n_top, 8.0, width=2)
    ref = cutout_ref.CutoutRef(1, nfine, 16, df, 32 + 48 + 15, 8, 32, 1, 5, 3, 1, K_MAD)
    ref.request([(1, 0, n_top, 2, 1)])
    outs = [ref.run(x[n:n + 16]) for n in range(0, total, 16)]
    (served, _, out), = [o for o in outs if o[0]]
    rec, W, P = cutout_ref.split_out(out, 1, 8, 32, 5)
    e = cutout_reference(x, df, 0, n_top, 2, 1, 8, 32, 1, 5, 3, K_MAD)
    assert np.array_equal(W[0].astype(np.float64), e['W']) and np.array_equal(P[0].astype(np.float64), e['P'])
    r = rec[0]
    assert (r['id'], r['status'], r['i'], r['iw'], r['j'], float(r['M']), float(r['A'])) == (1, 0, e['i'], e['iw'], e['j'], e['M'], e['A']) == (1, 0, 3, 1, 17, 1246.0, 49.0)
    assert abs(r['S'] - e['S']) <= 2.0 ** -22 * e['S'] and abs(r['S0'] - e['S0']) <= 2.0 ** -22 * e['S0'] and r['S'] > r['S0']
    assert abs(e['S'] - 11.018218) < 1e-5 and abs(e['S0'] - 3.777148) < 1e-5
    out = cutout_refined(r, fine, 2, 1, 5, 32, 1, n_top * 100, 100)
    assert out['dm'] == 3.0 and out['width'] == 2 and out['seq'] == (n_top + 1) * 100          # (windows 70 and 71: the middle is the start of 71)
