"""BeamDetrend without a GPU: the restatement's median and MAD against brute force (ties, -0), detrend_plan and detrend_startup, the
FURTHER_ENGINES row under the per-row checks of tests/test_engine_table_cpu.py, the C entry points' argument checks, the block on
CPU rings with a backend that serves xengDetrend* by the restatement (tests/detrend_ref.py) -- time alignment, the uncommitted head
of D / nwin + detrend_startup spans, the header, a gap, the constructor's refusals -- and a planted chain: noise on a 20 sigma
sinusoid and a ramp with a 4-window pulse, detrended by the restatement and searched by tests/pulse_ref.py."""
import ctypes

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import BeamDetrend, detrend_k_mad, detrend_plan, detrend_reference, detrend_startup
from caltech_bifrost_dsp_amd.ring import Ring
from tests import detrend_cases, detrend_ref, test_engine_table_cpu
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.pulse_ref import pulse_search
from tests.test_pulse_cpu import dedisp_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2
F = np.float32
K_MAD = detrend_cases.K_MAD


# ---------------------------------------------------------------- the median and the MAD
def _brute_median(v):
    """rank = the count of entries below it, ties by index, compared as floats with -0 = +0; the values are fl(v + 0)"""
    v = [F(a) + F(0) for a in v]
    n = len(v)
    rank = {}
    for i in range(n):
        rank[sum(1 for j in range(n) if v[j] < v[i] or (v[j] == v[i] and j < i))] = v[i]
    return F(F(0.5) * F(rank[n // 2 - 1] + rank[n // 2]))


@pytest.mark.parametrize("seed", range(6))
def test_median_and_mad_against_brute_force_with_ties(seed):
    rng = np.random.default_rng(seed)
    n = 2 * int(rng.integers(2, 20))
    v = rng.integers(-3, 4, n).astype(F) * F(0.1)               # few distinct values: many ties
    v[rng.random(n) < 0.2] = F(-0.0)
    M, A, G, valid = detrend_ref.knot(v[None], True, K_MAD)
    assert M.tobytes() == np.asarray(_brute_median(v), F).tobytes()
    dev = np.abs(v - M[0])
    assert A.tobytes() == np.asarray(_brute_median(dev), F).tobytes()
    s = F(F(K_MAD) * A[0])
    assert bool(valid[0]) == bool(s > 0) and G[0].tobytes() == (F(1) / s if s > 0 else F(0)).tobytes()
    assert not np.signbit(M[0]) or M[0] != 0                    # (a median of zeros is +0)


def test_a_block_with_a_value_that_is_not_finite_has_no_knot():
    blk = np.array([[1, 2, np.nan, 4], [1, 2, np.inf, 4], [1, 2, 3, 4], [5, 5, 5, 5]], F)
    M, A, G, valid = detrend_ref.knot(blk, True, K_MAD)
    assert valid.tolist() == [False, False, True, False] and M.tolist() == [0, 0, 2.5, 5] and A.tolist() == [0, 0, 1, 0] and G[[0, 1, 3]].tolist() == [0, 0, 0]
    assert detrend_ref.knot(blk, False, K_MAD)[3].tolist() == [False, False, True, True]


# ---------------------------------------------------------------- the host helpers
def test_detrend_plan_and_startup_arithmetic():
    assert detrend_plan(0.001, 1.0, 30) == 1000                 # 1500 windows = 50 spans
    assert detrend_plan(0.001, 1.001, 30) == 1000 and detrend_plan(0.001, 1.011, 30) == 1020       # (3 nblk / 2) % 30 == 0: nblk a multiple of 20
    assert detrend_plan(0.001, 0.0001, 4) == 8 and detrend_plan(0.001, 100.0, 4) == 8192 and detrend_plan(1.0, 7.0, 1) == 6
    assert detrend_plan(0.5, 15.0, 15) == 30
    for n in (detrend_plan(0.002, 0.7, 7), detrend_plan(0.01, 3.0, 45)):
        assert n % 2 == 0 and 4 <= n <= 8192
    assert (3 * detrend_plan(0.002, 0.7, 7) // 2) % 7 == 0
    for bad in ((0, 1.0, 4), (0.001, float('nan'), 4), (0.001, 1.0, 0), (0.001, 1.0, 2.0), (0.001, 1.0, 8193)):
        with pytest.raises(ValueError):
            detrend_plan(*bad)
    # W = ceil(S / nblk) nblk + nblk / 2, the count ceil(W / nwin)
    assert detrend_startup(5, 8, 4) == 3 and detrend_startup(8, 8, 4) == 3 and detrend_startup(9, 8, 4) == 5 and detrend_startup(0, 8, 4) == 1
    assert detrend_startup(700, 1000, 30) == 50 and detrend_startup(1001, 1000, 30) == 84
    for bad in ((-1, 8, 4), (5, 7, 4), (5, 8, 0), (5.0, 8, 4)):
        with pytest.raises(ValueError):
            detrend_startup(*bad)
    assert detrend_k_mad() == float(F(1.4826))


def test_detrend_reference_equals_the_restatement_on_integer_data():
    x = detrend_cases.integer_scene(3, 160, 1, 5, 1)
    out, knots = detrend_ref.detrend(x, [16] * 10, 16, False, K_MAD)
    y, M, A, valid = detrend_reference(x[..., 0].reshape(160, 5), 16, normalise=False)
    assert np.array_equal(out[24:].astype(np.float64), y[:136]) and valid.all() and out[24:].any()
    assert all(np.array_equal(k[0].astype(np.float64), M[i]) and np.array_equal(k[1].astype(np.float64), A[i]) for i, k in enumerate(knots))


# ---------------------------------------------------------------- the engine table and the C entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.FURTHER_ENGINES == [("Detrend", "detrend", True)]
    older = ffi.ENGINES + ffi.MORE_ENGINES + ffi.NEWER_ENGINES + ffi.NEWEST_ENGINES + ffi.LATEST_ENGINES
    assert not {r[0] for r in ffi.FURTHER_ENGINES} & {r[0] for r in older} and not {r[1] for r in ffi.FURTHER_ENGINES} & {r[1] for r in older}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.FURTHER_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.FURTHER_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    L = ffi.lib()
    names = ["xengDetrend" + n for n in ("Initialize", "Run", "Reset", "GetInfo", "GetKnots", "CheckGuards", "Mark", "Wait", "TicketDone", "Sync", "Destroy")]
    for name in names:
        assert hasattr(L, name) and name in ffi.SYMBOLS and name in test_engine_table_cpu.DECLARED, name
        assert (name in ffi.ENQUEUE_ONLY) == (name[11:] in ("Run", "Reset", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "run", "reset", "info", "knots", "guards_intact", "mark", "wait", "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "detrend_" + m)), m
    good = [2, 8, 4, 1, 8, 1, 1.0]              # (npair, ndm, nwin, nprod, nblk, normalise, k_mad)
    for i, v in ((0, 0), (1, 0), (2, 0), (2, 9), (3, 2), (3, 0), (4, 7), (4, 2), (4, 8194), (5, 2), (5, -1), (6, 0.0), (6, -1.0), (6, float('nan')),
                 (6, float('inf'))):
        args = list(good)
        args[i] = v
        assert L.xengDetrendInitialize(0, *args[:6], ctypes.c_float(args[6])) == INVALID_ARGUMENT, args
    assert L.xengDetrendInitialize(0, 4097, 4096, 4, 1, 8, 1, ctypes.c_float(1.0)) == INVALID_ARGUMENT          # more than 2^24 series
    assert L.xengDetrendInitialize(0, 4096, 4096, 4, 1, 40, 1, ctypes.c_float(1.0)) == INVALID_ARGUMENT         # exactly 2^32 bytes: not below the limit
    assert b"history" in L.xengGetLastError()
    if not _gpu_present():
        assert L.xengDetrendInitialize(0, *good[:6], ctypes.c_float(good[6])) not in (0, INVALID_ARGUMENT)      # (good sizes get as far as the device)
    done = ctypes.c_int(-1)
    for args in ((None, 1, 16, ctypes.byref(done)), (16, 1, None, ctypes.byref(done)), (16, 1, 16, None), (20, 1, 16, ctypes.byref(done)),
                 (16, 1, 24, ctypes.byref(done))):
        assert L.xengDetrendRun(*args) == INVALID_ARGUMENT
    assert L.xengDetrendGetInfo(None, None) == INVALID_ARGUMENT and L.xengDetrendGetKnots(None, None, None) == INVALID_ARGUMENT
    if not _gpu_present():
        n = ctypes.c_longlong()
        b = (ctypes.c_float * 4)()
        assert L.xengDetrendRun(16, 1, 16, ctypes.byref(done)) == INVALID_STATE and L.xengDetrendReset() == INVALID_STATE
        assert L.xengDetrendGetInfo(ctypes.byref(n), ctypes.byref(n)) == INVALID_STATE and done.value == -1
        assert L.xengDetrendGetKnots(b, b, ctypes.cast(b, ctypes.POINTER(ctypes.c_ubyte))) == INVALID_STATE


# ---------------------------------------------------------------- the block on CPU rings
class DetrendBackend(OracleBackend):
    """The oracle backend plus xengDetrend* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.dt, self.calls = None, []

    def detrend_initialize(self, gpu, npair, ndm, nwin, nprod, nblk, normalise, k_mad):
        self.dt = detrend_ref.DetrendRef(npair * ndm, nblk, normalise, k_mad, nprod)
        self.dims = (nwin, npair, ndm, nprod)
        self.calls.append(('init', nwin, nprod, nblk, int(normalise), k_mad))
        return 0

    def detrend_run(self, in_arr, nwin_call, out_arr):
        assert 1 <= nwin_call <= self.dims[0]
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape((nwin_call,) + self.dims[1:])
        before = self.dt.nblocks
        out = self.dt.run(x)
        out_arr.numpy().reshape(-1).view(np.uint8)[...] = np.frombuffer(out.tobytes(), np.uint8)
        self.calls.append('run')
        return 0, int(self.dt.nblocks > before)

    def detrend_knots(self, npair, ndm):
        return tuple(a.reshape(npair, ndm) for a in self.dt.newest)

    def detrend_reset(self):
        self.dt.reset()
        self.calls.append('reset')

    def detrend_mark(self):
        return self.beam_mark()

    def detrend_wait(self, ticket):
        self.beam_wait(ticket)

    def detrend_sync(self):
        pass


BLK = dict(npair=2, ndm=3, nwin=4, nblk=8)
NWIN, NBLK, HEAD = 4, 8, 3                      # D = 12 windows = 3 spans


def _reference(x, nprod, normalise=True):
    ref = detrend_ref.DetrendRef(6, NBLK, normalise, detrend_k_mad(), nprod)
    return [ref.run(x[j * NWIN:(j + 1) * NWIN]) for j in range(x.shape[0] // NWIN)]


@pytest.mark.parametrize("nprod", [1, 4])
def test_block_is_time_aligned_drops_head_and_startup_and_writes_the_header(nprod):
    """12 spans of 4 windows, nblk 8, dedisp_latency 5: D / nwin = 3 outputs lie before the sequence and detrend_startup(5, 8, 4) = 3
    more lie against knot 0, which saw partial sums.  Every span is enqueued, the first 6 outputs are not committed, and the output
    sequence begins at input span 3's time: output span j is the detrended input span 3 + j.  The tail of 12 windows is not flushed."""
    seq0, acc_len, S = 4096, 32, 5
    nstart = detrend_startup(S, NBLK, NWIN)
    assert nstart == 3
    x = detrend_cases.float_scene(21, 12 * NWIN, 2, 3, nprod, NBLK, special=False)
    hdr = dedisp_header(2, 3, nprod, seq0=seq0, S=S, acc_len=acc_len)
    be = DetrendBackend()
    dt = BeamDetrend(LOG, Ring("dd-output"), Ring("dt-output"), backend=be, **BLK)
    ispan, ospan = NWIN * 6 * nprod * 4, NWIN * 6 * 4
    sink = Sink(dt.oring, ospan)
    run_blocks([dt], Source(dt.iring, [(hdr, x, ispan)]), [sink])
    (hd, tag, spans), = sink.sequences
    step = NWIN * acc_len
    assert tag == seq0 + nstart * step == hd['seq0'] and len(spans) == 12 - HEAD - nstart
    exp = _reference(x, nprod)
    assert [s.tobytes() for s in spans] == [o.tobytes() for o in exp[HEAD + nstart:]] and all(o.any() for o in exp[HEAD + nstart:])
    # output span j is input span nstart + j, detrended: the float64 statement of window m sits at m itself
    y64 = detrend_reference(detrend_ref.series(x, nprod), NBLK, True, detrend_k_mad())[0]
    got = np.concatenate([np.frombuffer(s.tobytes(), F).reshape(NWIN, 6) for s in spans])
    assert np.allclose(got, y64[nstart * NWIN:nstart * NWIN + got.shape[0]], rtol=1e-4, atol=1e-4)
    assert (hd['nprod'], hd['detrended'], hd['detrend_nblk'], hd['detrend_normalised'], hd['detrend_nskipped']) == (1, True, NBLK, True, nstart * NWIN)
    assert all(hd[k] == v for k, v in hdr.items() if k not in ('seq0', 'nprod'))
    assert (hd['dedisp_latency'], hd['ndm'], hd['dms'], hd['tsamp'], hd['acc_len']) == (S, 3, hdr['dms'], hdr['tsamp'], acc_len)
    assert be.calls == [('init', NWIN, nprod, NBLK, 1, detrend_k_mad())] + ['run'] * 12
    assert dt.stats['nwindow'] == 48 and dt.stats['nblock'] == 6 and dt.stats['ngap'] == 0
    assert all(a.tobytes() == b.reshape(2, 3).tobytes() for a, b in zip(dt.knots(), be.dt.newest))
    # a detrended ring is not detrended again (and the searches' own check takes the header)
    from caltech_bifrost_dsp_amd.blocks.beam_dedisperse_block import check_dedispersed_header
    assert check_dedispersed_header("X", hd, 2, 3)[0] == 1
    dt2 = BeamDetrend(LOG, _FakeRing([_FakeSeq(hd, [(0, x[:NWIN, ..., :1])], ospan)]), Ring("x"), backend=DetrendBackend(), **BLK)
    with pytest.raises(ValueError, match="already"):
        dt2.main()


def test_block_gap_resets_and_restarts_the_sequence():
    """Spans 0..8 and 10..19 of a sequence (9 never read), dedisp_latency 0 (detrend_startup = 1): the first output sequence has
    spans 1..5 detrended, the gap resets the context and the output restarts at span 11's time in a sequence of its own."""
    seq0, acc_len = 640, 32
    nstart = detrend_startup(0, NBLK, NWIN)
    assert nstart == 1
    x = detrend_cases.float_scene(22, 20 * NWIN, 2, 3, 1, NBLK, special=False)
    hdr = dedisp_header(2, 3, 1, seq0=seq0, S=0, acc_len=acc_len)
    be, r1 = DetrendBackend(), Ring("dt-output")
    span = NWIN * 6 * 4
    spans = [(k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])) for k in list(range(9)) + list(range(10, 20))]
    dt = BeamDetrend(LOG, _FakeRing([_FakeSeq(hdr, spans, span)]), r1, backend=be, normalise=False, **BLK)
    sink = Sink(r1, span)
    sink.start()
    dt.main()
    sink.join(20)
    (h0, t0, s0), (h1, t1, s1) = sink.sequences
    step = NWIN * acc_len
    assert (t0, t1) == (seq0 + step, seq0 + 11 * step) and (h0['seq0'], h1['seq0']) == (t0, t1)
    assert (len(s0), len(s1)) == (9 - HEAD - nstart, 10 - HEAD - nstart) and h0['detrend_normalised'] is False
    assert [s.tobytes() for s in s0] == [o.tobytes() for o in _reference(x[:9 * NWIN], 1, False)[HEAD + nstart:]]
    assert [s.tobytes() for s in s1] == [o.tobytes() for o in _reference(x[10 * NWIN:], 1, False)[HEAD + nstart:]]
    assert be.calls == [('init', NWIN, 1, NBLK, 0, detrend_k_mad())] + ['run'] * 9 + ['reset'] + ['run'] * 10
    assert dt.stats['ngap'] == 1 and dt.stats['nwindow'] == 19 * NWIN


@pytest.mark.parametrize("kw", [dict(npair=0), dict(ndm=0), dict(nwin=0), dict(nblk=7), dict(nblk=2), dict(nblk=8194), dict(nwin=16, nblk=8), dict(nwin=5),
                                dict(nblk=10, nwin=4), dict(npair=4097, ndm=4096), dict(npair=4096, ndm=4096, nblk=40, nwin=4), dict(normalise=None),
                                dict(nwin=2.0), dict(nblk=True)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(BLK)
    args.update(kw)
    be = DetrendBackend()
    with pytest.raises(ValueError, match="BEAM_DETREND"):
        BeamDetrend(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.dt is None


# ---------------------------------------------------------------- the planted chain
def test_planted_chain_the_pulse_is_found_and_the_wander_is_gone():
    """One series of 64 blocks of nblk = 64: unit normal noise, a sinusoid of amplitude 20 sigma and period 32 nblk, a ramp of 10
    sigma over the run, and a pulse of 4 windows x 5 sigma at window 2000.  The chain is the restatement, normalised, then
    tests/pulse_ref.py in float32 with 8 widths and blocks of 64.
      The pulse: the best record of the run has iw = 2 (4 windows) and ends at window 2003.
      The wander: the detrended series smoothed over nblk windows.  Its bar is what the float64 statement (detrend_reference) leaves
      on the same scene, max |smoothed| = 0.348 sigma here (the float32 chain leaves 0.348 too; the bar is 0.504), plus the knot noise: a median of nblk normal values scatters by
      1.2533 / sqrt(nblk) sigma, the 1.25 / sqrt(nblk) = 0.16 of the bar.  The float32 chain must stay below their sum.
      Without the block: the 128-window boxcar of pulse_ref on the raw scene scores the wander alone at 33.6 sigma (printed),
      which buries the pulse's 6.4; behind the block the widest boxcar reaches 2.6 and must stay below 6."""
    nblk, nb, at = 64, 64, 2000
    rng = np.random.default_rng(12)
    n = np.arange(nb * nblk)
    noise = rng.standard_normal(n.size)
    z = noise + 20.0 * np.sin(2 * np.pi * n / (32.0 * nblk)) + 10.0 * n / n.size
    z[at:at + 4] += 5.0
    z = (100.0 + 3.0 * z).astype(F)             # (a level and a scale of its own: the block normalises)
    D = 3 * nblk // 2
    out, _ = detrend_ref.detrend(z[:, None, None], [nblk] * nb, nblk, True, K_MAD)
    y = out[D:, 0]                              # y[m] = the detrended window m, m < nwindows - D
    r = pulse_search(y[:, None], 64, 8, np.float32)
    snr = np.where(r['scored'], r['snr'], -np.inf)[..., 0]
    m, iw = np.unravel_index(np.argmax(snr), snr.shape)
    assert (m, iw) == (at + 3, 2) and snr[m, iw] > 5      # (4 windows x 5 sigma are 10 sigma in a 4-window boxcar; half of it is the floor)
    smooth = lambda v: np.convolve(v, np.ones(nblk) / nblk, mode='valid')
    y64 = detrend_reference(z.astype(np.float64), nblk, True, 1.4826)[0][:y.size]
    keep = slice(nblk, y.size - 2 * nblk)       # (clear of the first half block, which has one knot, and of the pulse's own smoothing)
    w32, w64 = np.abs(smooth(y)[keep]).max(), np.abs(smooth(y64)[keep]).max()
    bar = w64 + 1.25 / np.sqrt(nblk)
    raw = pulse_search(z[:, None], 64, 8, np.float32)
    raw7 = np.nanmax(np.where(raw['scored'][:, 7, 0], raw['snr'][:, 7, 0], np.nan))
    wide = np.nanmax(np.where(r['scored'][:, 7, 0], r['snr'][:, 7, 0], np.nan))
    print("wander: float32 %.3f, float64 %.3f, bar %.3f; 128-window score raw %.1f, detrended %.1f; pulse %.1f" % (w32, w64, bar, raw7, wide, snr[m, iw]))
    assert w32 <= bar
    assert raw7 > 30 and wide < 6
