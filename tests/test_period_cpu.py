"""BeamPeriodSearch without a GPU, both ring implementations: the harmonic-sum restatement (tests/period_ref.py) against a
term-by-term loop; period_pfa against direct summation and the closed form at a = 1; period_candidates on hand-built planes (ties,
an empty plane, a record exactly at the threshold, grouping over trials); the block on CPU rings with a backend that keeps the
context's state and serves xengPeriod* by the float32 restatement -- one plane per stack and none in between, the start-up spans
skipped, a gap dropping the partial stack, `threshold` and `mask` commands, the seq0 arithmetic, a planted pulse train reported
at its period and DM, refusals -- and the C entry points' argument checks."""
import ctypes
import json
import math

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import BeamPeriodSearch, period_candidates, period_pfa
from caltech_bifrost_dsp_amd.blocks.period_search import RECORD, as_records
from caltech_bifrost_dsp_amd.ring import Ring
from tests.fake_backend import OracleBackend
from tests.period_ref import harmonic_records, harmonic_records_naive, harmonic_sums, segment_spectrum, series
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_pulse_cpu import dedisp_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
NT, NWIN = 256, 32                              # the smallest segment; 8 spans fill it


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def plane_of(rec):
    """A period_ref record (dict of arrays [npair][ndm][nlevel]) as the plane the library writes."""
    out = np.zeros(rec['k'].shape, RECORD)
    out['H'], out['k'] = rec['H'], rec['k']
    return out


class PeriodBackend(OracleBackend):
    """The oracle backend plus xengPeriod* served by the float32 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.pr, self.calls = None, []

    def period_initialize(self, gpu, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin):
        self.pr = dict(npair=npair, ndm=ndm, nwin=nwin, nprod=nprod, nt=nt, nstack=nstack, nlevel=nlevel, nwhite=nwhite, kmin=kmin)
        self.keep, self.seg, self.A, self.nseg = None, [], None, 0
        self.calls.append(('init', nprod))
        return 0

    def period_set_mask(self, keep):
        self.keep = None if keep is None else np.array(keep, np.uint8)
        self.calls.append('mask')
        return 0

    def period_run(self, in_arr, nwin_call, out_arr):
        u = self.pr
        assert 1 <= nwin_call <= u['nwin']
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, u['npair'] * u['ndm'], u['nprod'])
        completed = 0
        for row in series(x, np.float32):
            self.seg.append(row)
            if len(self.seg) == u['nt']:
                S = segment_spectrum(np.array(self.seg), u['nwhite'], self.keep, np.float32)
                self.A = S if self.nseg == 0 else (self.A + S).astype(np.float32)
                self.seg, self.nseg = [], self.nseg + 1
                if self.nseg == u['nstack']:
                    rec = harmonic_records(self.A.reshape(u['npair'], u['ndm'], -1), u['nlevel'], u['kmin'])
                    out_arr.numpy().reshape(-1).view(np.uint8)[...] = plane_of(rec).reshape(-1).view(np.uint8)
                    self.nseg, completed = 0, 1
        if not completed:
            assert out_arr is None
        self.calls.append('run+' if completed else 'run')
        return 0, completed

    def period_reset(self):
        self.seg, self.nseg = [], 0
        self.calls.append('reset')

    def period_mark(self):
        return self.beam_mark()

    def period_wait(self, ticket):
        self.beam_wait(ticket)

    def period_sync(self):
        pass


def _noise(rng, nwindows, npair, ndm, nprod):
    return rng.integers(0, 50, (nwindows, npair, ndm, nprod)).astype(np.float32)


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _expected_planes(x, nt, nstack, nlevel, nwhite, kmin, keep=None):
    """The planes of a run from a reset, one per completed stack, by the float32 restatement."""
    z = series(x, np.float32).reshape(x.shape[0], -1)
    out, A = [], None
    for s in range(z.shape[0] // nt):
        S = segment_spectrum(z[s * nt:(s + 1) * nt], nwhite, keep, np.float32)
        A = S if s % nstack == 0 else (A + S).astype(np.float32)
        if s % nstack == nstack - 1:
            out.append(plane_of(harmonic_records(A.reshape(x.shape[1], x.shape[2], -1), nlevel, kmin)))
    return out


# ---------------------------------------------------------------- the restatement
def test_harmonic_sums_are_the_definition():
    """Against one term at a time: random A with a NaN word, an all-NaN series, planted equal maxima (the smallest k wins) and a
    series of equal words (every sum equal: k = h * kmin); the integer index (j*k + h/2) div h written out for one (h, k)."""
    rng = np.random.default_rng(3)
    N, nlevel, kmin = 128, 5, 3
    A = rng.exponential(1.0, (6, N)).astype(np.float32)
    A[1, 40] = np.nan
    A[2] = np.nan
    A[3, [50, 70]] = 30.0
    A[4] = 3.0
    got = harmonic_records(A, nlevel, kmin)
    for s in range(A.shape[0]):
        for lv, (H, k) in enumerate(harmonic_records_naive(A[s], nlevel, kmin)):
            assert got['k'][s, lv] == k and np.float32(got['H'][s, lv]).tobytes() == np.float32(H).tobytes(), (s, lv)
    assert (got['k'][2] == -1).all() and (got['H'][2] == 0).all() and not np.signbit(got['H'][2]).any()
    assert got['k'][3, 0] == 50 and got['H'][3, 0] == 30.0
    assert [int(k) for k in got['k'][4]] == [kmin << lv for lv in range(nlevel)] and [float(h) for h in got['H'][4]] == [3.0 * (1 << lv) for lv in range(nlevel)]
    k, H = harmonic_sums(A[0], 2, kmin)                          # h = 4, k = 13: bins (13+2)/4, (26+2)/4, (39+2)/4, (52+2)/4 = 3, 7, 10, 13
    assert k[1] == 13
    assert H[1] == np.float32(np.float32(np.float32(A[0, 3] + A[0, 7]) + A[0, 10]) + A[0, 13])
    assert got['k'][1, 0] >= 0 and got['k'][1, 0] != 40


def test_segment_spectrum_whitens_masks_and_flags():
    """A tone in noise: the whitened spectrum has mean 1 over the counted bins of every block, the tone's bin stands out, zapped
    bins and blocks without a counted bin read 1.0, bin 0 reads +0, a dead series is all ones, a series with a NaN is all NaN."""
    rng = np.random.default_rng(5)
    nt, B = 256, 16
    z = rng.normal(60.0, 1.0, (nt, 4))
    z[:, 0] += 0.8 * np.cos(2 * np.pi * 37 * np.arange(nt) / nt)
    z[:, 1] = 0.0
    z[100, 2] = np.nan
    keep = np.ones(nt // 2, np.uint8)
    keep[14:19] = 0                                             # crosses the edge between blocks 0 and 1
    keep[48:64] = 0                                             # the whole of block 3
    S = segment_spectrum(z, B, keep)
    assert S[0].argmax() == 37 and S[0, 37] > 10
    assert (S[[0, 3]][:, ~keep.astype(bool)] == 1.0).all() and (S[:, 0] == 0).all() and not np.signbit(S[:, 0]).any()
    assert (S[1, 1:] == 1.0).all() and np.isnan(S[2, 1:]).all()
    for b in (0, 1, 2, 5):
        k = np.arange(b * B, (b + 1) * B)
        k = k[(k >= 1) & (keep[k] != 0)]
        assert abs(S[3, k].mean() - 1) < 1e-12


# ---------------------------------------------------------------- period_pfa, period_candidates
def test_period_pfa_against_direct_summation():
    H = np.array([0.0, 0.5, 3.0, 17.25, 60.0])
    assert np.allclose(period_pfa(H, 1, 1), -H, rtol=0, atol=1e-12)             # a = 1: Q = exp(-H)
    for h, nstack in ((1, 3), (4, 1), (16, 3), (8, 2)):
        a = h * nstack
        direct = np.array([math.exp(-x) * sum(x ** i / math.factorial(i) for i in range(a)) for x in H])
        assert np.allclose(np.exp(period_pfa(H, h, nstack)), direct, rtol=1e-12, atol=0), (h, nstack)
    assert period_pfa(0.0, 4, 2) == 0.0 and period_pfa(-1.0, 4, 2) == 0.0 and isinstance(period_pfa(3.0, 1, 1), float)
    far = period_pfa(5000.0, 16, 8)                                             # exp(-5000) underflows; the log does not
    assert np.isfinite(far) and -5000 < far < -4000
    with pytest.raises(ValueError, match="period_search"):
        period_pfa(1.0, 0, 1)


def _plane(npair, ndm, nlevel):
    p = np.zeros((npair, ndm, nlevel), RECORD)
    p['k'] = -1
    return p


def test_period_candidates_groups_ties_empty_and_threshold():
    dms = np.arange(6) * 0.5
    nt, nstack, tsamp = 1024, 1, 1e-3
    p = _plane(2, 6, 2)
    assert period_candidates(p, 3.0, dms, nt, nstack, tsamp) == []
    assert period_candidates(p, -1.0, dms, nt, nstack, tsamp) == []            # (nothing qualified: not a candidate at any threshold)
    # pair 0, level 0: trials 1-3 at k = 100, 101, 100 (one group, best at 2), trial 5 at k = 300 (its own); level 1: trial 2
    for d, (H, k) in {1: (30.0, 100), 2: (40.0, 101), 3: (35.0, 100), 5: (32.0, 300)}.items():
        p[0, d, 0] = (H, k)
    p[0, 2, 1] = (45.0, 202)
    p[1, 3, 0] = (33.0, 50)                                     # pair 1: a tie over trials 3 and 4: the lowest trial
    p[1, 4, 0] = (33.0, 51)
    p[1, 0, 0] = (500.0, -1)                                    # (nothing qualified, whatever the word holds)
    got = period_candidates(p, 3.0, dms, nt, nstack, tsamp, ntrials=1000)
    assert [(c['pair'], c['h'], c['idm'], c['k'], c['ntrial']) for c in got] == [(0, 1, 2, 101, 3), (0, 1, 5, 300, 1), (0, 2, 2, 202, 1), (1, 1, 3, 50, 2)]
    c = got[0]
    assert c['dm'] == 1.0 and c['H'] == 40.0 and c['freq'] == 101 / (1024 * 1e-3) and c['period'] == 1 / c['freq']
    assert abs(c['log10_pfa'] - (-40.0 + math.log(1000)) / math.log(10)) < 1e-9 and 6.5 < c['sigma'] < 8.5
    assert got[2]['freq'] == 202 / (2 * 1024 * 1e-3)            # (k indexes the top harmonic)
    # exactly at the threshold: in; one ulp above: out.  The default ntrials is nlevel * nt / 2
    at = -(period_pfa(32.0, 1, nstack) + math.log(1000)) / math.log(10)
    assert [c['idm'] for c in period_candidates(p, at, dms, nt, nstack, tsamp, ntrials=1000) if c['pair'] == 0 and c['h'] == 1] == [2, 5]
    assert [c['idm'] for c in period_candidates(p, np.nextafter(at, 100), dms, nt, nstack, tsamp, ntrials=1000) if c['pair'] == 0 and c['h'] == 1] == [2]
    dflt = period_candidates(p, 3.0, dms, nt, nstack, tsamp)
    assert abs(dflt[0]['log10_pfa'] - (-40.0 + math.log(2 * 512)) / math.log(10)) < 1e-9
    # more stacked segments make the same H less significant
    assert period_candidates(p, 3.0, dms, nt, 8, tsamp, ntrials=1000)[0]['log10_pfa'] > c['log10_pfa']
    # the same plane as raw words, and refusals
    raw = p.reshape(-1).view(np.uint32).reshape(2, 6, 2, 2)
    assert period_candidates(raw, 3.0, dms, nt, nstack, tsamp, ntrials=1000) == got
    assert as_records(p.tobytes(), 2, 6, 2).shape == (2, 6, 2)
    with pytest.raises(ValueError, match="period_search"):
        period_candidates(p, 3.0, dms[:-1], nt, nstack, tsamp)
    with pytest.raises(ValueError, match="period_search"):
        as_records(np.zeros(7, np.uint32))


# ---------------------------------------------------------------- the block on CPU rings
@pytest.mark.parametrize("nprod", [1, 4])
def test_block_one_plane_per_stack_and_none_in_between(nprod):
    """Source -> BeamPeriodSearch -> Sink, two sequences of 2 stacks of 2 segments and 3 spans more: the output holds exactly two
    planes per sequence, each the restatement's; only the calls that complete a stack carry an output; the header adds nt,
    nstack, nlevel, nwhite, kmin and carries dedisp_latency through."""
    npair, ndm, nstack, nlevel, nwhite, kmin = 2, 5, 2, 3, 16, 2
    nspan = 2 * nstack * NT // NWIN + 3
    rng = np.random.default_rng(5 + nprod)
    xs = [_noise(rng, nspan * NWIN, npair, ndm, nprod) for _ in range(2)]
    hdrs = [dedisp_header(npair, ndm, nprod, seq0=1000 * (s + 1), S=0) for s in range(2)]
    r0, r1 = Ring("dd-output"), Ring("pr-output")
    be = PeriodBackend()
    got = []
    pr = BeamPeriodSearch(LOG, r0, r1, npair=npair, ndm=ndm, nwin=NWIN, nt=NT, nstack=nstack, nlevel=nlevel, nwhite=nwhite, kmin=kmin, threshold=0.5,
                          on_candidates=got.append, backend=be)
    sink = Sink(r1, npair * ndm * nlevel * 8)
    run_blocks([pr], Source(r0, [(hdrs[s], xs[s], NWIN * npair * ndm * nprod * 4) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hdrs[s]['seq0'] == hd['seq0'] and len(spans) == 2
        exp = _expected_planes(xs[s], NT, nstack, nlevel, nwhite, kmin)
        assert len(exp) == 2
        for k, o in enumerate(spans):
            assert o.tobytes() == exp[k].tobytes(), (s, k)
            assert (as_records(o, npair, ndm, nlevel)['k'] >= 0).all()
    hd = sink.sequences[0][0]
    assert (hd['nt'], hd['nstack'], hd['nlevel'], hd['nwhite'], hd['kmin'], hd['threshold']) == (NT, nstack, nlevel, nwhite, kmin, 0.5)
    assert hd['ndm'] == ndm and hd['dedisp_latency'] == 0 and hd['nprod'] == nprod and hd['dms'] == hdrs[0]['dms']
    per = ['run'] * (nstack * NT // NWIN - 1) + ['run+']
    assert be.calls == [('init', nprod)] + per * 2 + ['run'] * 3 + ['reset'] + per * 2 + ['run'] * 3
    assert pr.stats['nwindow'] == 2 * nspan * NWIN and pr.stats['nstack_done'] == 4 and pr.stats['ndropped'] == 0 and pr.stats['nstartup'] == 0
    assert pr.stats['ncand'] == sum(len(c) for c in got)


def test_block_skips_the_start_up_spans_and_counts_seq0_from_there():
    """dedisp_latency = 40 windows and spans of 32: spans 0 and 1 begin inside the partial sums and are skipped; the first stack
    starts at span 2, whose sample is the output's seq0 and time tag, and the plane is the restatement of the windows from there."""
    npair, ndm, nlevel, nwhite, kmin, seq0, acc_len, S = 1, 5, 2, 8, 1, 4096, 32, 40
    nspan = 2 + NT // NWIN + 1
    rng = np.random.default_rng(19)
    x = _noise(rng, nspan * NWIN, npair, ndm, 1)
    x[:S] *= (np.arange(S)[:, None, None, None] + 1) / (S + 1)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, S=S, acc_len=acc_len)
    be = PeriodBackend()
    pr = BeamPeriodSearch(LOG, Ring("dd-output"), Ring("pr-output"), npair=npair, ndm=ndm, nwin=NWIN, nt=NT, nlevel=nlevel, nwhite=nwhite, kmin=kmin,
                          backend=be)
    sink = Sink(pr.oring, npair * ndm * nlevel * 8)
    run_blocks([pr], Source(pr.iring, [(hdr, x, NWIN * npair * ndm * 4)]), [sink])
    (hd, tag, planes), = sink.sequences
    first = seq0 + 2 * NWIN * acc_len
    assert tag == first and hd['seq0'] == first and hd['dedisp_latency'] == S and len(planes) == 1
    assert planes[0].tobytes() == _expected_planes(x[2 * NWIN:], NT, 1, nlevel, nwhite, kmin)[0].tobytes()
    assert pr.stats['nstartup'] == 2 and pr.stats['nwindow'] == (nspan - 2) * NWIN and pr.stats['nstack_done'] == 1
    assert be.calls == [('init', 1)] + ['run'] * (NT // NWIN - 1) + ['run+', 'run']


def test_block_gap_drops_the_partial_stack():
    """Spans 0..10 and 12..27 of a sequence (11 never read), a stack of one segment of 8 spans: stack 0 completes at span 7, spans
    8-10 are a partial segment that the gap drops (ndropped = 1); the output restarts in a sequence of its own at span 12's
    sample, whose planes are the restatement of a run that begins at span 12."""
    npair, ndm, nlevel, nwhite, kmin, seq0, acc_len = 1, 5, 2, 8, 1, 700, 32
    rng = np.random.default_rng(11)
    x = _noise(rng, 28 * NWIN, npair, ndm, 1)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, S=0, acc_len=acc_len)
    seen = [(k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])) for k in list(range(11)) + list(range(12, 28))]
    be = PeriodBackend()
    r1 = Ring("pr-output")
    pr = BeamPeriodSearch(LOG, _FakeRing([_FakeSeq(hdr, seen, NWIN * npair * ndm * 4)]), r1, npair=npair, ndm=ndm, nwin=NWIN, nt=NT, nlevel=nlevel,
                          nwhite=nwhite, kmin=kmin, backend=be)
    sink = Sink(r1, npair * ndm * nlevel * 8)
    sink.start()
    pr.main()
    sink.join(20)
    assert be.calls == [('init', 1)] + ['run'] * 7 + ['run+'] + ['run'] * 3 + ['reset'] + (['run'] * 7 + ['run+']) * 2
    (h0, t0, a), (h1, t1, b) = sink.sequences
    step = NWIN * acc_len
    assert (h0['seq0'], t0, h1['seq0'], t1) == (seq0, seq0, seq0 + 12 * step, seq0 + 12 * step) and (len(a), len(b)) == (1, 2)
    assert a[0].tobytes() == _expected_planes(x, NT, 1, nlevel, nwhite, kmin)[0].tobytes()
    exp = _expected_planes(x[12 * NWIN:], NT, 1, nlevel, nwhite, kmin)
    assert [o.tobytes() for o in b] == [e.tobytes() for e in exp]
    assert pr.stats['ndropped'] == 1 and pr.stats['nstack_done'] == 3


def test_block_threshold_and_mask_commands():
    """A tone at bin 37 in one series, three stacks of one segment.  Stack 0 is judged at threshold 1000 (nothing); a `threshold`
    command before span 8 makes stack 1 report the tone; a `mask` command before span 16 zaps bins [36, 39) and stack 2 reports
    nothing at level 1 there: its plane is the restatement under that mask.  Commands that are not numbers or bin ranges are
    refused and change nothing."""
    npair, ndm, nlevel, nwhite, kmin = 1, 5, 1, 16, 2
    rng = np.random.default_rng(13)
    x = _noise(rng, 3 * NT, npair, ndm, 1)
    x[:, 0, 2, 0] += np.round(20 * np.cos(2 * np.pi * 37 * np.arange(3 * NT) / NT)).astype(np.float32)
    hdr = dedisp_header(npair, ndm, 1, S=0)
    be = PeriodBackend()
    r1 = Ring("pr-output")
    box, got = {}, []

    def spans():
        for k in range(3 * NT // NWIN):
            if k == 8:
                box['pr'].process_command_strings(_cmd(threshold=3.0))
                assert box['pr'].last_response['val']['status'] == 'normal'
            if k == 16:
                box['pr'].process_command_strings(_cmd("2", mask=[[36, 39]]))
                assert box['pr'].last_response['val']['status'] == 'normal'
            if k == 17:
                for n, bad in enumerate(({'threshold': "high"}, {'threshold': float('nan')}, {'mask': [[3]]}, {'mask': [[5, 2]]}, {'mask': "all"},
                                         {'mask': [[-1, 4]]})):
                    box['pr'].process_command_strings(_cmd(str(3 + n), **bad))
                    assert box['pr'].last_response['val']['status'] == 'error', bad
            yield k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])

    seq = _FakeSeq(hdr, spans(), NWIN * npair * ndm * 4)
    pr = box['pr'] = BeamPeriodSearch(LOG, _FakeRing([seq]), r1, npair=npair, ndm=ndm, nwin=NWIN, nt=NT, nlevel=nlevel, nwhite=nwhite, kmin=kmin,
                                      threshold=1000, on_candidates=got.append, backend=be)
    sink = Sink(r1, npair * ndm * nlevel * 8)
    sink.start()
    pr.main()
    sink.join(20)
    (hd, _, out), = sink.sequences
    assert hd['threshold'] == 1000 and len(out) == 3
    keep = np.ones(NT // 2, np.uint8)
    keep[36:39] = 0
    free, zapped = _expected_planes(x, NT, 1, nlevel, nwhite, kmin), _expected_planes(x, NT, 1, nlevel, nwhite, kmin, keep)
    assert [o.tobytes() for o in out] == [free[0].tobytes(), free[1].tobytes(), zapped[2].tobytes()]
    assert free[1]['k'][0, 2, 0] == 37 and zapped[2]['k'][0, 2, 0] != 37
    assert len(got) == 1 and [(c['pair'], c['idm'], c['k'], c['h']) for c in got[0]] == [(0, 2, 37, 1)]
    assert be.calls.count('mask') == 1 and be.calls.index('mask') == 1 + 16
    assert pr.stats['threshold'] == 3.0 and pr.threshold == 3.0 and pr.stats['ncand'] == 1 and pr.stats['candidates'] == []


def test_block_reports_a_planted_pulse_train_at_its_period_and_dm():
    """A one-window pulse every 32 windows in series (pair 1, trial 3) of integer noise, and fainter in the neighbouring trial: the
    fundamental is NT/32 = 8 bins and 15 harmonics lie below Nyquist.  Every candidate is one of the two series; at the top level
    (8 harmonics) there is exactly one, the planted series at k = 64 with the neighbour grouped in, and its period is 32 windows."""
    npair, ndm, nlevel, nwhite, kmin, acc_len = 2, 5, 4, 16, 2, 32
    rng = np.random.default_rng(29)
    x = _noise(rng, NT, npair, ndm, 1)
    x[::32, 1, 3, 0] += 120
    x[::32, 1, 2, 0] += 80
    hdr = dedisp_header(npair, ndm, 1, seq0=64, S=0, acc_len=acc_len)
    got = []
    pr = BeamPeriodSearch(LOG, Ring("dd-output"), Ring("pr-output"), npair=npair, ndm=ndm, nwin=NWIN, nt=NT, nlevel=nlevel, nwhite=nwhite, kmin=kmin,
                          threshold=6.0, on_candidates=got.extend, backend=PeriodBackend())
    sink = Sink(pr.oring, npair * ndm * nlevel * 8)
    run_blocks([pr], Source(pr.iring, [(hdr, x, NWIN * npair * ndm * 4)]), [sink])
    assert got and {(c['pair'], c['idm']) for c in got} <= {(1, 2), (1, 3)}
    top, = [c for c in got if c['h'] == 8]
    assert (top['pair'], top['idm'], top['dm'], top['k'], top['ntrial']) == (1, 3, 1.5, 8 * NT // 32, 2)
    assert abs(top['period'] - 32 * hdr['tsamp']) < 1e-12 * top['period'] and top['sigma'] > 6 and top['log10_pfa'] < -6
    assert pr.stats['ncand'] == len(got)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(npair=0), dict(ndm=-1), dict(nwin=0), dict(nwin=NT + 1), dict(nt=300), dict(nt=128), dict(nt=1 << 15), dict(nstack=0),
                                dict(nlevel=0), dict(nlevel=6), dict(nwhite=4), dict(nwhite=24), dict(nwhite=NT), dict(kmin=0), dict(kmin=NT // 32),
                                dict(threshold=float('nan')), dict(threshold="8"), dict(on_candidates=3)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(npair=1, ndm=5, nwin=NWIN, nt=NT)
    args.update(kw)
    be = PeriodBackend()
    with pytest.raises(ValueError, match="BEAM_PERIOD_SEARCH"):
        BeamPeriodSearch(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.pr is None


class _FakeOut:
    name, space = "device-output", "cuda"


def test_constructor_refuses_a_device_output_ring():
    with pytest.raises(ValueError, match="BEAM_PERIOD_SEARCH"):
        BeamPeriodSearch(LOG, Ring("a"), _FakeOut(), npair=1, ndm=5, nwin=NWIN, nt=NT, backend=PeriodBackend())


@pytest.mark.parametrize("bad", [dict(ndm=None), dict(ndm=4), dict(nbeam=2), dict(nprod=2), dict(nprod=None), dict(tsamp=None), dict(tsamp=0.0),
                                 dict(dms=[0.0]), dict(dedisp_latency=None), dict(dedisp_latency=-1), dict(acc_len=0)])
def test_block_refuses_what_is_not_dedispersed_beams(bad):
    npair, ndm = 1, 5
    be = PeriodBackend()
    hdr = dedisp_header(npair, ndm, 1)
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NWIN, npair, ndm, 1), np.float32)
    pr = BeamPeriodSearch(LOG, _FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), npair=npair, ndm=ndm, nwin=NWIN, nt=NT, backend=be)
    with pytest.raises(ValueError, match="BEAM_PERIOD_SEARCH"):
        pr.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengPeriodInitialize", "xengPeriodSetMask", "xengPeriodRun", "xengPeriodReset", "xengPeriodGetInfo", "xengPeriodGetSpectrum",
         "xengPeriodCheckGuards", "xengPeriodMark", "xengPeriodWait", "xengPeriodTicketDone", "xengPeriodSync", "xengPeriodDestroy")


def test_backend_forwards_every_call_the_block_makes():
    """HipBackend has a method for each period_* call (and the fake backend above has the ones the block makes)."""
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("period_initialize", "period_set_mask", "period_run", "period_reset", "period_info", "period_spectrum", "period_guards_intact",
              "period_mark", "period_wait", "period_ticket_done", "period_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("period_initialize", "period_set_mask", "period_run", "period_reset", "period_mark", "period_wait", "period_sync"):
        assert callable(getattr(PeriodBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are not.
    Initialize refuses every size outside the contract's table before it touches a device; Run refuses null and misaligned
    pointers, the getters null results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengPeriodRun", "xengPeriodReset", "xengPeriodMark", "xengPeriodTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengPeriodInitialize", "xengPeriodSetMask", "xengPeriodGetSpectrum", "xengPeriodWait", "xengPeriodSync", "xengPeriodCheckGuards",
                 "xengPeriodGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin)
    good = (0, 16, 256, 30, 1, 1 << 14, 4, 5, 64, 2)
    for i, v in ((1, 0), (2, 0), (3, 0), (3, (1 << 14) + 1), (4, 2), (4, 0), (5, 128), (5, 1 << 15), (5, 3000), (6, 0), (7, 0), (7, 6), (8, 4), (8, 48),
                 (8, 1 << 14), (9, 0), (9, 512), (1, 1 << 13)):
        args = list(good)
        args[i] = v
        if (i, v) == (1, 1 << 13):
            args[2] = 1 << 12                                   # 2^25 series
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeriodInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    with pytest.raises(ffi.XengError) as ei:                    # 2^24 series of 2^14 windows: the state's limit
        ffi.call("xengPeriodInitialize", 0, 1 << 12, 1 << 12, 30, 1, 1 << 14, 1, 1, 8, 1)
    assert ei.value.status == INVALID_ARGUMENT
    f = np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n, s = ctypes.c_longlong(), ctypes.c_int()
    for name, args in (("xengPeriodRun", (None, 1, 4096, ctypes.byref(s))), ("xengPeriodRun", (4096, 1, 4096, None)),
                       ("xengPeriodRun", (4100, 1, 4096, ctypes.byref(s))), ("xengPeriodRun", (4096, 1, 4104, ctypes.byref(s))),
                       ("xengPeriodGetInfo", (None, ctypes.byref(s), ctypes.byref(n))), ("xengPeriodGetInfo", (ctypes.byref(n), None, ctypes.byref(n))),
                       ("xengPeriodGetInfo", (ctypes.byref(n), ctypes.byref(s), None)), ("xengPeriodGetSpectrum", (None, ctypes.byref(s))),
                       ("xengPeriodGetSpectrum", (f, None)), ("xengPeriodMark", (None,)), ("xengPeriodTicketDone", (1, None)),
                       ("xengPeriodCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_period_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengPeriodRun", (4096, 1, 4096, ctypes.byref(s))), ("xengPeriodRun", (4096, 1, None, ctypes.byref(s))), ("xengPeriodReset", ()),
                       ("xengPeriodSetMask", (None,)), ("xengPeriodGetInfo", (ctypes.byref(n), ctypes.byref(s), ctypes.byref(n))),
                       ("xengPeriodGetSpectrum", (f, ctypes.byref(s))), ("xengPeriodMark", (ctypes.byref(t),)), ("xengPeriodWait", (1,)),
                       ("xengPeriodTicketDone", (1, ctypes.byref(s))), ("xengPeriodSync", ()), ("xengPeriodCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengPeriodDestroy")       # (nothing to destroy: success)
