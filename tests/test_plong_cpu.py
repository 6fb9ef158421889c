"""BeamPeriodSearchLong without a GPU: the banded harmonic-sum restatement (tests/plong_ref.py) against xengPeriod*'s at one band,
against a term-by-term loop and against the single-band maximum; period_bands; period_candidates_long and period_sift on hand-built
planes (a fundamental with its harmonics 2, 3 and 1/2 collapses to one candidate, an unrelated line survives, the result does not
depend on the order of the input); the block on CPU rings with a backend that keeps the context's state and serves xengPlong* by
the float32 restatement -- window counting, the start-up skip, a gap, the commands, the header; the MORE_ENGINES row under the
per-row checks of tests/test_engine_table_cpu.py; and the C entry points' argument checks."""
import ctypes
import itertools
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import BeamPeriodSearch, BeamPeriodSearchLong, period_bands, period_candidates_long, period_sift
from caltech_bifrost_dsp_amd.blocks.period_search import RECORD, as_records_long, band_bins
from caltech_bifrost_dsp_amd.ring import Ring
from tests import period_ref, plong_ref, test_engine_table_cpu
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_pulse_cpu import dedisp_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
NT, NWIN = 1 << 15, 1 << 12                     # the smallest segment; 8 spans fill it


# ---------------------------------------------------------------- the restatement
def _spectrum(rng, shape):
    """A stack as the sums meet it: exponential powers, a few exact ties, a NaN series."""
    A = rng.exponential(1.0, shape).astype(np.float32)
    A[..., 0] = 0
    return A


def test_one_band_is_the_rule_of_the_short_search_bit_for_bit():
    rng = np.random.default_rng(1)
    A = _spectrum(rng, (2, 3, 4096))
    A[1, 1] = np.nan
    A[0, 2, 100:200] = 2.0                                      # equal maxima wherever these win
    for kmin in (1, 2, 127):
        new, old = plong_ref.harmonic_records(A, 5, [kmin, 4096]), period_ref.harmonic_records(A, 5, kmin)
        assert new['H'][..., 0].tobytes() == old['H'].tobytes() and new['k'][..., 0].tobytes() == old['k'].tobytes()
    assert (new['k'][1, 1] == -1).all() and (new['H'][1, 1] == 0).all()


def test_banded_records_are_the_definition_term_by_term():
    rng = np.random.default_rng(2)
    N, kedge = 256, [1, 2, 5, 17, 40, 256]
    A = np.round(_spectrum(rng, (3, N)) * 4)                    # (small integers: ties abound)
    A[2, 37] = np.nan
    rec = plong_ref.harmonic_records(A, 5, kedge)
    for s in range(3):
        naive = plong_ref.harmonic_records_naive(A[s], 5, kedge)
        for lv in range(5):
            for b in range(5):
                H, k = naive[lv][b]
                assert (rec['H'][s, lv, b], rec['k'][s, lv, b]) == (np.float32(H), k), (s, lv, b)
    assert rec['k'][0, 4, 4] == -1 and rec['k'][0, 3, 4] == -1     # 16 * 40 and 8 * 40 are past N: empty bands
    assert rec['k'][0, 2, 4] >= 160


def test_the_union_of_the_bands_reproduces_the_single_band_maximum():
    rng = np.random.default_rng(3)
    N = 8192
    A = _spectrum(rng, (4, N))
    kedge = period_bands(2 * N, 7, 3)
    one, many = plong_ref.harmonic_records(A, 5, [3, N]), plong_ref.harmonic_records(A, 5, kedge)
    for lv in range(5):
        H = np.where(many['k'][:, lv] >= 0, many['H'][:, lv], -np.inf)
        b = H.argmax(axis=1)                                    # (the first of equal maxima: the lowest band, the smallest k)
        assert (H[np.arange(4), b] == one['H'][:, lv, 0]).all() and (many['k'][np.arange(4), lv, b] == one['k'][:, lv, 0]).all()


def test_period_bands_edges():
    assert period_bands(1 << 15, 1, 2) == [2, 1 << 14]
    e = period_bands(1 << 20, 32, 2)
    assert len(e) == 33 and e[0] == 2 and e[-1] == 1 << 19 and all(b > a for a, b in zip(e, e[1:]))
    r = np.array(e[9:], float)
    assert np.allclose(r[1:] / r[:-1], (2 ** 18) ** (1 / 32), rtol=0.02)      # log-spaced where a bin is fine enough
    assert period_bands(1 << 15, 32, 1, 40)[:30] == list(range(1, 31))          # closer than a bin: steps of one bin
    assert period_bands(1 << 15, 3, 5, 8) == [5, 6, 7, 8]
    assert period_bands(1 << 15, 7, 2, 1000)[-1] == 1000
    for bad in ((1 << 15, 0, 2), (1 << 15, 33, 2), (1 << 15, 4, 0), (1 << 15, 4, 1 << 10), (1 << 15, 4, 5, 8), (1 << 15, 4, 2, (1 << 14) + 1)):
        with pytest.raises(ValueError):
            period_bands(*bad)
    assert band_bins([2, 10, 100, 1 << 14], 4, 1 << 15) == [128, 1440, (1 << 14) - 1600]
    assert band_bins([2, 2000, 1 << 14], 4, 1 << 15) == [16384 - 32, 0]


# ---------------------------------------------------------------- candidates and sifting
def _plane(npair, ndm, nlevel, nband):
    p = np.zeros((npair, ndm, nlevel, nband), RECORD)
    p['k'] = -1
    return p


def _band(kedge, f):
    return max(b for b in range(len(kedge) - 1) if kedge[b] <= f)


def test_candidates_of_a_banded_plane_group_over_trials_and_bands():
    nt, kedge, dms = 1 << 15, [2, 100, 1000, 1 << 14], np.arange(4) * 0.5
    p = _plane(2, 4, 2, 3)
    p[1, 2, 0, 1] = (40.0, 999)                                 # a source at a band's edge: band 1 at trial 2 ...
    p[1, 1, 0, 2] = (35.0, 1000)                                # ... band 2 at trial 1
    p[1, 3, 0, 0] = (30.0, 50)                                  # another, elsewhere
    p[0, 0, 1, 2] = (3.0, 4000)                                 # below any threshold
    c = period_candidates_long(p, 6.0, dms, nt, 1, 1e-3, kedge)
    assert [(x['pair'], x['idm'], x['band'], x['k'], x['ntrial']) for x in c] == [(1, 2, 1, 999, 2), (1, 3, 0, 50, 1)]
    assert abs(c[0]['freq'] - 999 / (nt * 1e-3)) < 1e-12 and c[0]['dm'] == 1.0 and c[0]['h'] == 1
    ntr = sum(sum(band_bins(kedge, lv, nt)) for lv in range(2))
    assert ntr == (16384 - 2) + (16384 - 4)
    assert abs(c[0]['log10_pfa'] - (-40.0 + np.log(ntr)) / np.log(10)) < 1e-9
    assert period_candidates_long(p, 6.0, dms, nt, 1, 1e-3, kedge, ntrials=1)[0]['log10_pfa'] < c[0]['log10_pfa']
    assert period_candidates_long(_plane(2, 4, 2, 3), 0.0, dms, nt, 1, 1e-3, kedge) == []
    raw = p.view(np.uint8).reshape(-1)
    assert as_records_long(raw, 2, 4, 2, 3).tobytes() == p.tobytes()
    for bad in (lambda: period_candidates_long(p, 6.0, dms, nt, 1, 1e-3, kedge[:-1]), lambda: period_candidates_long(p, 6.0, dms[:3], nt, 1, 1e-3, kedge),
                lambda: as_records_long(raw, 2, 4, 2, 4), lambda: as_records_long(raw)):
        with pytest.raises(ValueError):
            bad()


def test_sifting_collapses_a_fundamental_with_its_harmonics_and_keeps_an_unrelated_line():
    """A fundamental at 300.4 bins seen at 16 harmonics (k = 4806), its 2nd and 3rd harmonic and its half as candidates of their own
    at lower levels, in three different bands and two trials, and an unrelated line at 1373 bins: two survivors, the fundamental
    with three harmonics at ratios (2, 1), (3, 1) and (1, 2) and the line with none; the same for every order of the input; a
    source in another pair is never merged."""
    nt, kedge, dms = 1 << 16, period_bands(1 << 16, 7, 2), np.arange(3) * 1.0
    p = _plane(2, 3, 5, 7)
    f0 = 300.4
    p[0, 1, 4, _band(kedge, f0)] = (120.0, round(16 * f0))              # the fundamental, 16 harmonics
    p[0, 1, 3, _band(kedge, 2 * f0)] = (70.0, round(8 * 2 * f0))        # the 2nd harmonic, 8 harmonics
    p[0, 2, 2, _band(kedge, 3 * f0)] = (45.0, round(4 * 3 * f0))        # the 3rd, 4 harmonics, the next trial
    p[0, 2, 4, _band(kedge, f0 / 2)] = (90.0, round(16 * f0 / 2))       # the half (the fundamental's own band: another trial)
    p[0, 0, 0, _band(kedge, 1373)] = (30.0, 1373)                       # unrelated: 1373 / 300.4 = 4.5706
    p[1, 1, 4, _band(kedge, f0)] = (120.0, round(16 * f0))              # the same source in another pair
    cands = period_candidates_long(p, 6.0, dms, nt, 1, 1e-3, kedge)
    assert len(cands) == 6
    out = period_sift(cands, nt)
    assert [(c['pair'], c['k'], c['h'], len(c['harmonics'])) for c in out] == [(0, 4806, 16, 3), (0, 1373, 1, 0), (1, 4806, 16, 0)]
    assert [(h['k'], h['h'], h['ratio']) for h in out[0]['harmonics']] == [(2403, 16, (1, 2)), (4806, 8, (2, 1)), (3605, 4, (3, 1))]
    assert all('harmonics' not in c for c in cands)             # (the input is left as it was)
    for perm in itertools.islice(itertools.permutations(cands), 0, 720, 7):
        assert period_sift(list(perm), nt) == out
    assert len(period_sift(cands, nt, max_ratio=1)) == 6 and period_sift([], nt) == []
    assert len(period_sift(cands, nt, max_ratio=2)) == 4         # (the third harmonic stands alone)
    with pytest.raises(ValueError):
        period_sift([dict(cands[0], k=nt)], nt)


# ---------------------------------------------------------------- the block on CPU rings
class PlongBackend(OracleBackend):
    """The oracle backend plus xengPlong* served by the float32 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.pl, self.calls = None, []

    def plong_initialize(self, gpu, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kedge):
        self.pl = dict(npair=npair, ndm=ndm, nwin=nwin, nprod=nprod, nt=nt, nstack=nstack, nlevel=nlevel, nwhite=nwhite, kedge=list(kedge))
        self.keep, self.seg, self.A, self.nseg = None, [], None, 0
        self.calls.append(('init', nprod))
        return 0

    def plong_set_mask(self, keep):
        self.keep = None if keep is None else np.array(keep, np.uint8)
        self.calls.append('mask')
        return 0

    def plong_run(self, in_arr, nwin_call, out_arr):
        u = self.pl
        assert 1 <= nwin_call <= u['nwin']
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, u['npair'] * u['ndm'], u['nprod'])
        completed = 0
        self.seg.append(plong_ref.series(x, np.float32))
        if sum(len(s) for s in self.seg) == u['nt']:
            S = plong_ref.segment_spectrum(np.concatenate(self.seg), u['nwhite'], self.keep, np.float32)
            self.A = S if self.nseg == 0 else (self.A + S).astype(np.float32)
            self.seg, self.nseg = [], self.nseg + 1
            if self.nseg == u['nstack']:
                rec = plong_ref.harmonic_records(self.A.reshape(u['npair'], u['ndm'], -1), u['nlevel'], u['kedge'])
                out_arr.numpy().reshape(-1).view(np.uint8)[...] = plong_ref.plane_of(rec).reshape(-1).view(np.uint8)
                self.nseg, completed = 0, 1
        if not completed:
            assert out_arr is None
        self.calls.append('run+' if completed else 'run')
        return 0, completed

    def plong_reset(self):
        self.seg, self.nseg = [], 0
        self.calls.append('reset')

    def plong_mark(self):
        return self.beam_mark()

    def plong_wait(self, ticket):
        self.beam_wait(ticket)

    def plong_sync(self):
        pass


def _noise(rng, nwindows, npair, ndm, nprod):
    return rng.integers(0, 50, (nwindows, npair, ndm, nprod)).astype(np.float32)


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _expected_planes(x, nt, nstack, nlevel, nwhite, kedge, keep=None):
    z = plong_ref.series(x, np.float32).reshape(x.shape[0], -1)
    return [plong_ref.plane_of(plong_ref.harmonic_records(A.reshape(x.shape[1], x.shape[2], -1), nlevel, kedge))
            for A, nseg in plong_ref.stacks(z, nt, nstack, nwhite, keep, np.float32) if nseg == nstack]


def test_block_counts_windows_skips_the_start_up_and_writes_the_header():
    """dedisp_latency = 5000 windows and spans of 4096: spans 0 and 1 begin inside the partial sums and are skipped; a stack of 2
    segments of 8 spans completes at span 17 and 3 spans more complete nothing.  One plane, the restatement's, of nlevel x nband
    records per series; only the completing call carries an output; the header adds nband and kedge."""
    npair, ndm, nstack, nlevel, nwhite, nprod, seq0, acc_len, S = 1, 3, 2, 3, 64, 4, 4096, 32, 5000
    nspan = 2 + nstack * NT // NWIN + 3
    rng = np.random.default_rng(5)
    x = _noise(rng, nspan * NWIN, npair, ndm, nprod)
    hdr = dedisp_header(npair, ndm, nprod, seq0=seq0, S=S, acc_len=acc_len)
    be, got = PlongBackend(), []
    pr = BeamPeriodSearchLong(LOG, Ring("dd-output"), Ring("pl-output"), npair=npair, ndm=ndm, nwin=NWIN, nt=NT, nstack=nstack, nlevel=nlevel, nwhite=nwhite,
                              kmin=3, nband=5, threshold=0.5, on_candidates=got.append, backend=be)
    assert isinstance(pr, BeamPeriodSearch) and pr.kedge == period_bands(NT, 5, 3) and pr.nband == 5
    sink = Sink(pr.oring, npair * ndm * nlevel * 5 * 8)
    run_blocks([pr], Source(pr.iring, [(hdr, x, NWIN * npair * ndm * nprod * 4)]), [sink])
    (hd, tag, planes), = sink.sequences
    first = seq0 + 2 * NWIN * acc_len
    assert tag == first == hd['seq0'] and len(planes) == 1
    exp, = _expected_planes(x[2 * NWIN:], NT, nstack, nlevel, nwhite, pr.kedge)
    assert planes[0].tobytes() == exp.tobytes() and exp.shape == (npair, ndm, nlevel, 5)
    assert (hd['nt'], hd['nstack'], hd['nlevel'], hd['nwhite'], hd['kmin'], hd['nband'], hd['kedge'], hd['threshold']) == (
        NT, nstack, nlevel, nwhite, 3, 5, pr.kedge, 0.5)
    assert hd['dedisp_latency'] == S and hd['nprod'] == nprod and hd['dms'] == hdr['dms']
    assert be.calls == [('init', nprod)] + ['run'] * (nstack * NT // NWIN - 1) + ['run+'] + ['run'] * 3
    assert pr.stats['nstartup'] == 2 and pr.stats['nwindow'] == (nspan - 2) * NWIN and pr.stats['nstack_done'] == 1 and pr.stats['ndropped'] == 0
    assert pr.stats['ncand'] == sum(len(c) for c in got) and all('harmonics' in c for cs in got for c in cs)


def test_block_gap_drops_the_partial_stack_and_commands_take_effect():
    """Spans 0..10 and 12..27 of a sequence (11 never read), a stack of one segment of 8 spans: stack 0 completes at span 7, spans
    8-10 are a partial segment that the gap drops; the output restarts in a sequence of its own at span 12's sample.  A tone at
    bin 3000.  A `threshold` command before span 12 makes the second sequence's first stack report it (the first stack, judged at
    1000, reports nothing); a `mask` command before span 20 zaps it in the last stack, whose plane is the restatement under that
    mask."""
    npair, ndm, nlevel, nwhite, seq0, acc_len = 1, 3, 1, 64, 700, 32
    kedge = [2, 500, 5000, NT // 2]
    rng = np.random.default_rng(11)
    x = _noise(rng, 28 * NWIN, npair, ndm, 1)
    x[:, 0, 1, 0] += np.round(20 * np.cos(2 * np.pi * 3000 * np.arange(28 * NWIN) / NT)).astype(np.float32)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, S=0, acc_len=acc_len)
    be, r1, box, got = PlongBackend(), Ring("pl-output"), {}, []

    def spans():
        for k in list(range(11)) + list(range(12, 28)):
            if k == 12:
                box['pr'].process_command_strings(_cmd(threshold=6.0))
                assert box['pr'].last_response['val']['status'] == 'normal'
            if k == 20:
                box['pr'].process_command_strings(_cmd("2", mask=[[2990, 3010]]))
                assert box['pr'].last_response['val']['status'] == 'normal'
                box['pr'].process_command_strings(_cmd("3", mask=[[5, 2]]))
                assert box['pr'].last_response['val']['status'] == 'error'
            yield k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])

    pr = box['pr'] = BeamPeriodSearchLong(LOG, _FakeRing([_FakeSeq(hdr, spans(), NWIN * npair * ndm * 4)]), r1, npair=npair, ndm=ndm, nwin=NWIN, nt=NT,
                                          nlevel=nlevel, nwhite=nwhite, kedge=kedge, threshold=1000, on_candidates=got.append, backend=be)
    sink = Sink(r1, npair * ndm * nlevel * 3 * 8)
    sink.start()
    pr.main()
    sink.join(20)
    run8 = ['run'] * 7 + ['run+']
    assert be.calls == [('init', 1)] + run8 + ['run'] * 3 + ['reset'] + run8 + ['mask'] + run8
    (h0, t0, a), (h1, t1, b) = sink.sequences
    step = NWIN * acc_len
    assert (h0['seq0'], t0, h1['seq0'], t1) == (seq0, seq0, seq0 + 12 * step, seq0 + 12 * step) and (len(a), len(b)) == (1, 2)
    keep = np.ones(NT // 2, np.uint8)
    keep[2990:3010] = 0
    assert a[0].tobytes() == _expected_planes(x[:NT], NT, 1, nlevel, nwhite, kedge)[0].tobytes()
    free, zapped = _expected_planes(x[12 * NWIN:], NT, 1, nlevel, nwhite, kedge), _expected_planes(x[12 * NWIN:], NT, 1, nlevel, nwhite, kedge, keep)
    assert [o.tobytes() for o in b] == [free[0].tobytes(), zapped[1].tobytes()]
    assert free[0]['k'][0, 1, 0, 1] == 3000 and zapped[1]['k'][0, 1, 0, 1] != 3000
    assert len(got) == 1 and [(c['pair'], c['idm'], c['band'], c['k'], c['h']) for c in got[0]] == [(0, 1, 1, 3000, 1)]
    assert pr.stats['ndropped'] == 1 and pr.stats['nstack_done'] == 3 and pr.stats['threshold'] == 6.0 and pr.stats['ncand'] == 1


@pytest.mark.parametrize("kw", [dict(npair=0), dict(nwin=NT + 1), dict(nt=1 << 14), dict(nt=1 << 21), dict(nt=40000), dict(nstack=0), dict(nlevel=6),
                                dict(nwhite=4), dict(nwhite=1 << 14), dict(nwhite=24), dict(kmin=0), dict(kmin=NT // 32), dict(nband=0), dict(nband=33),
                                dict(kedge=[2]), dict(kedge=[2, 2]), dict(kedge=[5, 3, 9]), dict(kedge=[0, 9]), dict(kedge=[NT // 32, NT // 2]),
                                dict(kedge=[2, NT // 2 + 1]), dict(kedge=list(range(2, 36))), dict(threshold=float('nan')), dict(on_candidates=3)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(npair=1, ndm=5, nwin=NWIN, nt=NT)
    args.update(kw)
    be = PlongBackend()
    with pytest.raises(ValueError, match="BEAM_PERIOD_SEARCH_LONG|period_bands"):
        BeamPeriodSearchLong(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.pl is None


# ---------------------------------------------------------------- the engine table and the C entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.MORE_ENGINES == [("Plong", "plong", True)] and len(ffi.ENGINES) == 19
    assert not {r[0] for r in ffi.MORE_ENGINES} & {r[0] for r in ffi.ENGINES} and not {r[1] for r in ffi.MORE_ENGINES} & {r[1] for r in ffi.ENGINES}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.MORE_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.MORE_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def _edges(*e):
    return (ctypes.c_int * len(e))(*e)


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported, declared and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are
    not; HipBackend has a method for each.  Initialize refuses every size outside the contract's table before it touches a device;
    Run refuses null and misaligned pointers, the getters null results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    names = ["xengPlong" + n for n in ("Initialize", "SetMask", "Run", "Reset", "GetInfo", "GetSpectrum", "SetBatch", "GetBatch", "CheckGuards", "Mark",
                                       "Wait", "TicketDone", "Sync", "Destroy")]
    for name in names:
        assert hasattr(L, name) and name in ffi.SYMBOLS and name in test_engine_table_cpu.DECLARED, name
        assert (name in ffi.ENQUEUE_ONLY) == (name[9:] in ("Run", "Reset", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_mask", "run", "reset", "info", "spectrum", "guards_intact", "mark", "wait", "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "plong_" + m)), m
    # (gpu, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, nband, kedge)
    good = [0, 16, 256, 30, 1, 1 << 15, 4, 5, 64, 2, _edges(2, 100, 1 << 14)]
    bad = [(1, 0), (2, 0), (3, 0), (3, (1 << 15) + 1), (4, 2), (5, 1 << 14), (5, 1 << 21), (5, 40000), (6, 0), (7, 0), (7, 6), (8, 4), (8, 48),
           (8, 1 << 14), (9, 0), (9, 33), (9, 3), (10, None), (10, _edges(0, 100, 1 << 14)), (10, _edges(1 << 10, 2000, 1 << 14)),
           (10, _edges(2, 2, 1 << 14)), (10, _edges(2, 100, 50)), (10, _edges(2, 100, (1 << 14) + 1))]
    for i, v in bad:
        args = list(good)
        args[i] = v
        if (i, v) == (9, 3):
            args[10] = _edges(2, 100, 1 << 14, 1 << 14)          # (the last edge repeated)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPlongInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, (i, v)
    for npair, ndm, nt in ((1 << 13, 1 << 12, 1 << 15), (1 << 12, 1 << 10, 1 << 15), (4096, 4, 1 << 20), (16384, 4, 1 << 18)):
        with pytest.raises(ffi.XengError) as ei:                # 2^25 series; 2^22 series of 2^15 windows, and four times what the contract names at 2^20 and 2^18
            ffi.call("xengPlongInitialize", 0, npair, ndm, 30, 1, nt, 1, 1, 8, 1, _edges(1, nt // 2))
        assert ei.value.status == INVALID_ARGUMENT
    f = np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n, s = ctypes.c_longlong(), ctypes.c_int()
    for name, args in (("xengPlongRun", (None, 1, 4096, ctypes.byref(s))), ("xengPlongRun", (4096, 1, 4096, None)),
                       ("xengPlongRun", (4100, 1, 4096, ctypes.byref(s))), ("xengPlongRun", (4096, 1, 4104, ctypes.byref(s))),
                       ("xengPlongGetInfo", (None, ctypes.byref(s), ctypes.byref(n))), ("xengPlongGetInfo", (ctypes.byref(n), None, ctypes.byref(n))),
                       ("xengPlongGetInfo", (ctypes.byref(n), ctypes.byref(s), None)), ("xengPlongGetSpectrum", (0, 1, None, ctypes.byref(s))),
                       ("xengPlongGetSpectrum", (0, 1, f, None)), ("xengPlongGetBatch", (None, ctypes.byref(s))), ("xengPlongGetBatch", (ctypes.byref(s), None)),
                       ("xengPlongMark", (None,)), ("xengPlongTicketDone", (1, None)), ("xengPlongCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_plong_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengPlongRun", (4096, 1, 4096, ctypes.byref(s))), ("xengPlongRun", (4096, 1, None, ctypes.byref(s))), ("xengPlongReset", ()),
                       ("xengPlongSetMask", (None,)), ("xengPlongGetInfo", (ctypes.byref(n), ctypes.byref(s), ctypes.byref(n))),
                       ("xengPlongGetSpectrum", (0, 1, f, ctypes.byref(s))), ("xengPlongSetBatch", (1,)), ("xengPlongGetBatch", (ctypes.byref(s), ctypes.byref(s))),
                       ("xengPlongMark", (ctypes.byref(t),)), ("xengPlongWait", (1,)), ("xengPlongTicketDone", (1, ctypes.byref(s))), ("xengPlongSync", ()),
                       ("xengPlongCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengPlongDestroy")        # (nothing to destroy: success)
