"""BeamFfaSearch without a GPU, both ring implementations: the host module (ffa_rows on exact fits and one short of them, ffa_period
with a plan round trip, ffa_candidates on hand-built planes); the float32 restatement (tests/ffa_ref.py) on a planted pulse train,
with numbers that were worked out once and are pinned here; the block on CPU rings with a backend that keeps the context's state
and serves xengFfa* by the restatement -- one plane per segment and none in between, the start-up spans skipped, a gap dropping
the partial segment, a `threshold` command, the header, refusals -- and the C entry points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import BeamFfaSearch, ffa_candidates, ffa_period, ffa_plan, ffa_rows
from caltech_bifrost_dsp_amd.blocks.ffa_search import RECORD, as_records
from caltech_bifrost_dsp_amd.ring import Ring
from tests import ffa_ref
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_pulse_cpu import dedisp_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
NT, NWIN = 256, 32                              # the smallest segment; 8 spans fill it at nds = 1
SIZES = dict(nt=NT, pmin=16, pmax=20, nds=1, noct=2, nwidth=2)


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


class FfaBackend(OracleBackend):
    """The oracle backend plus xengFfa* served by the float32 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.fa, self.calls = None, []

    def ffa_initialize(self, gpu, npair, ndm, nwin, nprod, nds, nt, noct, pmin, pmax, nwidth):
        self.fa = dict(npair=npair, ndm=ndm, nwin=nwin, nprod=nprod, nds=nds, nt=nt, noct=noct, pmin=pmin, pmax=pmax, nwidth=nwidth)
        self.win = []
        self.calls.append(('init', nprod))
        return 0

    def ffa_run(self, in_arr, nwin_call, out_arr):
        u = self.fa
        assert 1 <= nwin_call <= u['nwin']
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, u['npair'] * u['ndm'], u['nprod'])
        completed = 0
        for row in ffa_ref.series(x):
            self.win.append(row)
            if len(self.win) == u['nt'] * u['nds']:
                rec, _ = ffa_ref.records(ffa_ref.downsample(np.array(self.win), u['nds']), u['noct'], u['pmin'], u['pmax'], u['nwidth'])
                out_arr.numpy().reshape(-1).view(np.uint8)[...] = rec.reshape(-1).view(np.uint8)
                self.win, completed = [], 1
        if not completed:
            assert out_arr is None
        self.calls.append('run+' if completed else 'run')
        return 0, completed

    def ffa_reset(self):
        self.win = []
        self.calls.append('reset')

    def ffa_mark(self):
        return self.beam_mark()

    def ffa_wait(self, ticket):
        self.beam_wait(ticket)

    def ffa_sync(self):
        pass


def _noise(rng, nwindows, npair, ndm, nprod):
    return rng.integers(0, 50, (nwindows, npair, ndm, nprod)).astype(np.float32)


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _expected_planes(x, nt, pmin, pmax, nds, noct, nwidth):
    """The planes of a run from a reset, one per completed segment, by the float32 restatement."""
    z = ffa_ref.series(x)
    seg = nt * nds
    return [ffa_ref.records(ffa_ref.downsample(z[s * seg:(s + 1) * seg], nds), noct, pmin, pmax, nwidth)[0].reshape(x.shape[1], x.shape[2], noct, nwidth)
            for s in range(z.shape[0] // seg)]


def _block(iring, oring, backend, npair=1, ndm=5, **kw):
    args = dict(SIZES)
    args.update(kw)
    return BeamFfaSearch(LOG, iring, oring, npair=npair, ndm=ndm, nwin=NWIN, backend=backend, **args)


def _plane_bytes(npair, ndm, noct=SIZES['noct'], nwidth=SIZES['nwidth']):
    return npair * ndm * noct * nwidth * 16


# ---------------------------------------------------------------- the host module
def test_ffa_rows_on_exact_fits_and_one_short_of_them():
    assert [ffa_rows(n, p) for n, p in ((256, 16), (255, 16), (64, 32), (63, 32), (16384, 8192), (16383, 8192), (4096, 100), (3200, 100), (3199, 100))] == \
        [16, 8, 2, 1, 2, 1, 32, 32, 16]
    assert ffa_rows(10, 16) == 0 and ffa_rows(16, 16) == 1
    assert all(ffa_rows(n, p) == ffa_ref.ffa_rows(n, p) for n in (256, 300, 768, 4096) for p in range(16, n // 2 + 1, 7))
    with pytest.raises(ValueError, match="ffa_search"):
        ffa_rows(100, 0)


def test_ffa_period_and_a_plan_round_trip():
    """1 s to 60 s at windows of 1 ms and a duty cycle of 1 %: 100..199 samples a period, 10 windows a sample, 6 octaves and widths of
    1..32 samples; the first profile of the first octave is the shortest period asked for, the last of the top octave reaches past
    the longest, and neighbouring octaves overlap."""
    assert ffa_period(100, 12, 32, 0, 1, 1.0) == 100 + 12 / 31 and ffa_period(50, 6, 64, 1, 3, 0.5) == (50 + 6 / 63) * 2 * 3 * 0.5
    for bad in ((100, 32, 32), (100, -1, 32), (100, 0, 1)):
        with pytest.raises(ValueError, match="ffa_search"):
            ffa_period(bad[0], bad[1], bad[2], 0, 1, 1.0)
    nds, nt, noct, pmin, pmax, nwidth = ffa_plan(1.0, 60.0, 1e-3, 0.01)
    assert (nds, nt, noct, pmin, pmax, nwidth) == (10, 1 << 14, 6, 100, 199, 6)
    M0, Mt = ffa_rows(nt, pmin), ffa_rows(nt >> (noct - 1), pmax)
    assert Mt >= 2 and abs(ffa_period(pmin, 0, M0, 0, nds, 1e-3) - 1.0) < 1e-12 and ffa_period(pmax, Mt - 1, Mt, noct - 1, nds, 1e-3) >= 60.0
    for o in range(noct - 1):
        M = ffa_rows(nt >> o, pmax)
        assert abs(ffa_period(pmax, M - 1, M, o, nds, 1e-3) - ffa_period(pmin, 0, 2, o + 1, nds, 1e-3)) < 1e-12
    BeamFfaSearch(LOG, Ring("a"), Ring("b"), npair=1, ndm=5, nwin=30, nt=nt, pmin=pmin, pmax=pmax, nds=nds, noct=noct, nwidth=nwidth, backend=FfaBackend())
    # a range the longest segment cannot hold ends early; a short one takes one octave; 5 % pulses need no more than 20 samples
    assert ffa_plan(1.0, 1e4, 1e-3, 0.01)[2] == 6 and ffa_plan(1.0, 1.5, 1e-3, 0.01)[2] == 1
    assert ffa_plan(0.5, 4.0, 1e-3, 0.05) == (25, 1 << 14, 3, 20, 39, 4) and ffa_plan(0.5, 4.0, 1e-3, 0.5)[3] == 16
    for bad in ((0.0, 1.0, 1e-3, 0.01), (2.0, 1.0, 1e-3, 0.01), (1.0, 2.0, 0.0, 0.01), (1.0, 2.0, 1e-3, 0.0), (1.0, 2.0, 1e-3, 0.6), (0.01, 2.0, 1e-3, 0.01),
                (1.0, 2.0, 1e-6, 1e-4)):
        with pytest.raises(ValueError, match="ffa_search"):
            ffa_plan(*bad)


def _plane(npair, ndm, noct, nwidth):
    p = np.zeros((npair, ndm, noct, nwidth), RECORD)
    p['p'] = p['i'] = p['j'] = -1
    return p


def test_ffa_candidates_groups_over_trials_octaves_and_widths():
    dms = np.arange(4) * 0.5
    nt, nds, tsamp = 4096, 2, 1e-3
    p = _plane(2, 4, 2, 3)
    assert ffa_candidates(p, 6.0, dms, nt, nds, tsamp) == [] and ffa_candidates(p, -1.0, dms, nt, nds, tsamp) == []
    # pair 0: a source at 100.387 samples of octave 0 (M = 32): trials 1-3, two widths, and octave 1 at 50.19 (M = 32 there too)
    p[0, 1, 0, 1] = (9.0, 100, 12, 5)
    p[0, 2, 0, 1] = (12.0, 100, 12, 5)
    p[0, 2, 0, 2] = (10.0, 100, 13, 4)          # one profile on: within a step
    p[0, 3, 0, 1] = (8.0, 100, 11, 5)
    p[0, 2, 1, 0] = (11.0, 50, 6, 2)            # (50 + 6/31) * 2 = 100.387
    p[0, 0, 0, 0] = (7.0, 64, 0, 0)             # another period: its own candidate
    p[0, 0, 1, 2] = (50.0, -1, -1, -1)          # (no statistics, whatever the word holds)
    p[1, 3, 1, 1] = (6.0, 33, 5, 7)             # pair 1: exactly at the threshold
    p[1, 0, 0, 0] = (np.nan, 70, 0, 0)          # a NaN is below every threshold
    got = ffa_candidates(p, 6.0, dms, nt, nds, tsamp)
    assert [(c['pair'], c['idm'], c['octave'], c['iw'], c['p'], c['i'], c['ntrial']) for c in got] == \
        [(0, 0, 0, 0, 64, 0, 1), (0, 2, 0, 1, 100, 12, 5), (1, 3, 1, 1, 33, 5, 1)]
    c = got[1]
    assert c['dm'] == 1.0 and c['snr'] == 12.0 and c['width'] == 2 and c['j'] == 5 and c['M'] == 32
    assert c['period'] == ffa_period(100, 12, 32, 0, nds, tsamp) and abs(c['period'] - 100.387 * 2e-3) < 1e-6
    assert got[2]['period'] == ffa_period(33, 5, 32, 1, nds, tsamp)
    assert [x['pair'] for x in ffa_candidates(p, np.nextafter(np.float32(6.0), np.float32(7.0)), dms, nt, nds, tsamp)] == [0, 0]
    # two profiles on is another candidate
    p[0, 1, 0, 0] = (9.5, 100, 14, 5)
    assert [(x['idm'], x['i'], x['ntrial']) for x in ffa_candidates(p, 6.0, dms, nt, nds, tsamp) if x['p'] == 100] == [(2, 12, 5), (1, 14, 1)]
    # the same plane as raw words, and refusals
    raw = p.reshape(-1).view(np.uint32).reshape(2, 4, 2, 3, 4)
    assert ffa_candidates(raw, 6.0, dms, nt, nds, tsamp) == ffa_candidates(p, 6.0, dms, nt, nds, tsamp)
    assert as_records(p.tobytes(), 2, 4, 2, 3).shape == (2, 4, 2, 3)
    with pytest.raises(ValueError, match="ffa_search"):
        ffa_candidates(p, 6.0, dms[:-1], nt, nds, tsamp)
    with pytest.raises(ValueError, match="ffa_search"):
        as_records(np.zeros(7, np.uint32))
    p[1, 1, 1, 0] = (9.0, 1500, 0, 0)           # 1500 samples do not fit twice into 2048
    with pytest.raises(ValueError, match="ffa_search"):
        ffa_candidates(p, 6.0, dms, nt, nds, tsamp)


# ---------------------------------------------------------------- the restatement
def test_restatement_on_a_planted_train():
    """Uniform integers -8..8, NT = 4096, +6 where (n / 100.37) mod 1 < 3 / 100.37: at p = 64..128 and 5 widths the best record is the
    4-sample boxcar at p = 100, i = 12 of M = 32 -- 100.387 samples -- with snr 10.56; octave 1 over 32..64 finds p = 50, i = 6, snr
    9.1; the same noise without the train stays below 4.6, far below a threshold of 6."""
    rng = np.random.default_rng(1)
    nt = 4096
    noise = rng.integers(-8, 9, nt).astype(np.float32)
    n = np.arange(nt)
    train = noise.copy()
    train[(n / 100.37) % 1 < 3 / 100.37] += 6
    rec, st = ffa_ref.records(train[:, None], 1, 64, 128, 5)
    best = rec[0, 0][rec[0, 0]['snr'].argmax()]
    assert rec[0, 0]['snr'].argmax() == 2 and (best['p'], best['i']) == (100, 12) and ffa_rows(nt, 100) == 32 and abs(best['snr'] - 10.56) < 0.005
    assert abs(ffa_period(100, 12, 32, 0, 1, 1.0) - 100.387) < 1e-3
    rec1, _ = ffa_ref.records(train[:, None], 2, 32, 64, 5)
    best1 = rec1[0, 1][rec1[0, 1]['snr'].argmax()]
    assert (best1['p'], best1['i']) == (50, 6) and abs(best1['snr'] - 9.1) < 0.05
    quiet, _ = ffa_ref.records(noise[:, None], 1, 64, 128, 5)
    assert 4.0 < quiet['snr'].max() < 4.6 and quiet['snr'].max() < 6
    cands = ffa_candidates(rec.reshape(1, 1, 1, 5), 6.0, [0.0], nt, 1, 1.0)
    # (the 3-sample pulse drifts over the profiles next to the best one: the widths peak at i = 10, 12 and 15, more than a step apart)
    top = max(cands, key=lambda c: c['snr'])
    assert (top['p'], top['i'], top['iw']) == (100, 12, 2) and [(c['p'], c['i']) for c in cands] == [(100, 10), (100, 12), (100, 15)]
    assert sum(c['ntrial'] for c in cands) == 5 and all(abs(c['period'] - 100.37) < 0.15 for c in cands)
    assert ffa_candidates(quiet.reshape(1, 1, 1, 5), 6.0, [0.0], nt, 1, 1.0) == []
    # the statistics the restatement used are the float64 ones to float32 precision, and a dead or NaN series is invalid
    c, m, v, g = ffa_ref.stats64(train[:, None])
    assert st[0, 0, 0] == c[0] and abs(st[0, 0, 1] - m[0]) * g[0] < 1e-6 and abs(st[0, 0, 3] / g[0] - 1) < 1e-6
    bad = np.stack([np.zeros(nt, np.float32), np.where(n == 7, np.nan, noise)], axis=1)
    dead, _ = ffa_ref.records(bad, 2, 64, 128, 2)
    assert dead.tobytes() == np.array([(0.0, -1, -1, -1)] * 8, RECORD).tobytes()


# ---------------------------------------------------------------- the block on CPU rings
@pytest.mark.parametrize("nprod,nds", [(1, 1), (4, 2)])
def test_block_one_plane_per_segment_and_none_in_between(nprod, nds):
    """Source -> BeamFfaSearch -> Sink, two sequences of 2 segments and 3 spans more: the output holds exactly two planes per
    sequence, each the restatement's; only the calls that complete a segment carry an output; the header adds nds, nt, noct, pmin,
    pmax, nwidth, threshold and seq0 and carries dedisp_latency through."""
    npair, ndm = 2, 5
    nspan = 2 * NT * nds // NWIN + 3
    rng = np.random.default_rng(5 + nprod)
    xs = [_noise(rng, nspan * NWIN, npair, ndm, nprod) for _ in range(2)]
    hdrs = [dedisp_header(npair, ndm, nprod, seq0=1000 * (s + 1), S=0) for s in range(2)]
    r0, r1 = Ring("dd-output"), Ring("fa-output")
    be = FfaBackend()
    got = []
    fa = _block(r0, r1, be, npair, ndm, nds=nds, threshold=0.5, on_candidates=got.append)
    sink = Sink(r1, _plane_bytes(npair, ndm))
    run_blocks([fa], Source(r0, [(hdrs[s], xs[s], NWIN * npair * ndm * nprod * 4) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hdrs[s]['seq0'] == hd['seq0'] and len(spans) == 2
        exp = _expected_planes(xs[s], NT, 16, 20, nds, 2, 2)
        assert len(exp) == 2
        for k, o in enumerate(spans):
            assert o.tobytes() == exp[k].tobytes(), (s, k)
            assert (as_records(o, npair, ndm, 2, 2)['p'] >= 16).all()
    hd = sink.sequences[0][0]
    assert (hd['nds'], hd['nt'], hd['noct'], hd['pmin'], hd['pmax'], hd['nwidth'], hd['threshold']) == (nds, NT, 2, 16, 20, 2, 0.5)
    assert hd['ndm'] == ndm and hd['dedisp_latency'] == 0 and hd['nprod'] == nprod and hd['dms'] == hdrs[0]['dms']
    per = ['run'] * (NT * nds // NWIN - 1) + ['run+']
    assert be.calls == [('init', nprod)] + per * 2 + ['run'] * 3 + ['reset'] + per * 2 + ['run'] * 3
    assert fa.stats['nwindow'] == 2 * nspan * NWIN and fa.stats['nsegment_done'] == 4 and fa.stats['ndropped'] == 0 and fa.stats['nstartup'] == 0
    assert fa.stats['ncand'] == sum(len(c) for c in got) > 0


def test_block_skips_the_start_up_spans_and_counts_seq0_from_there():
    """dedisp_latency = 40 windows and spans of 32: spans 0 and 1 begin inside the partial sums and are skipped; the first segment
    starts at span 2, whose sample is the output's seq0 and time tag, and the plane is the restatement of the windows from there."""
    npair, ndm, seq0, acc_len, S = 1, 5, 4096, 32, 40
    nspan = 2 + NT // NWIN + 1
    rng = np.random.default_rng(19)
    x = _noise(rng, nspan * NWIN, npair, ndm, 1)
    x[:S] *= (np.arange(S)[:, None, None, None] + 1) / (S + 1)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, S=S, acc_len=acc_len)
    be = FfaBackend()
    fa = _block(Ring("dd-output"), Ring("fa-output"), be)
    sink = Sink(fa.oring, _plane_bytes(npair, ndm))
    run_blocks([fa], Source(fa.iring, [(hdr, x, NWIN * npair * ndm * 4)]), [sink])
    (hd, tag, planes), = sink.sequences
    first = seq0 + 2 * NWIN * acc_len
    assert tag == first and hd['seq0'] == first and hd['dedisp_latency'] == S and len(planes) == 1
    assert planes[0].tobytes() == _expected_planes(x[2 * NWIN:], NT, 16, 20, 1, 2, 2)[0].tobytes()
    assert fa.stats['nstartup'] == 2 and fa.stats['nwindow'] == (nspan - 2) * NWIN and fa.stats['nsegment_done'] == 1
    assert be.calls == [('init', 1)] + ['run'] * (NT // NWIN - 1) + ['run+', 'run']


def test_block_gap_drops_the_partial_segment():
    """Spans 0..10 and 12..27 of a sequence (11 never read), a segment of 8 spans: segment 0 completes at span 7, spans 8-10 are a
    partial segment that the gap drops (ndropped = 1); the output restarts in a sequence of its own at span 12's sample, whose
    planes are the restatement of a run that begins at span 12."""
    npair, ndm, seq0, acc_len = 1, 5, 700, 32
    rng = np.random.default_rng(11)
    x = _noise(rng, 28 * NWIN, npair, ndm, 1)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, S=0, acc_len=acc_len)
    seen = [(k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])) for k in list(range(11)) + list(range(12, 28))]
    be = FfaBackend()
    r1 = Ring("fa-output")
    fa = _block(_FakeRing([_FakeSeq(hdr, seen, NWIN * npair * ndm * 4)]), r1, be)
    sink = Sink(r1, _plane_bytes(npair, ndm))
    sink.start()
    fa.main()
    sink.join(20)
    assert be.calls == [('init', 1)] + ['run'] * 7 + ['run+'] + ['run'] * 3 + ['reset'] + (['run'] * 7 + ['run+']) * 2
    (h0, t0, a), (h1, t1, b) = sink.sequences
    step = NWIN * acc_len
    assert (h0['seq0'], t0, h1['seq0'], t1) == (seq0, seq0, seq0 + 12 * step, seq0 + 12 * step) and (len(a), len(b)) == (1, 2)
    assert a[0].tobytes() == _expected_planes(x, NT, 16, 20, 1, 2, 2)[0].tobytes()
    exp = _expected_planes(x[12 * NWIN:], NT, 16, 20, 1, 2, 2)
    assert [o.tobytes() for o in b] == [e.tobytes() for e in exp]
    assert fa.stats['ndropped'] == 1 and fa.stats['nsegment_done'] == 3


def test_block_threshold_command_and_a_planted_train():
    """A pulse every 18 samples in one series, two segments.  Segment 0 is judged at threshold 1000 (nothing); a `threshold` command
    before span 8 makes segment 1 report the train: one candidate, the planted series at 18 samples, with the neighbouring trial
    grouped in.  Commands that are not numbers are refused and change nothing."""
    npair, ndm = 2, 5
    rng = np.random.default_rng(13)
    x = _noise(rng, 2 * NT, npair, ndm, 1)
    x[::18, 1, 2, 0] += 120
    x[::18, 1, 3, 0] += 60
    hdr = dedisp_header(npair, ndm, 1, S=0)
    be = FfaBackend()
    r1 = Ring("fa-output")
    box, got = {}, []

    def spans():
        for k in range(2 * NT // NWIN):
            if k == 8:
                box['fa'].process_command_strings(_cmd(threshold=8.0))
                assert box['fa'].last_response['val']['status'] == 'normal'
            if k == 9:
                for n, bad in enumerate(({'threshold': "high"}, {'threshold': float('nan')})):
                    box['fa'].process_command_strings(_cmd(str(3 + n), **bad))
                    assert box['fa'].last_response['val']['status'] == 'error', bad
            yield k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])

    seq = _FakeSeq(hdr, spans(), NWIN * npair * ndm * 4)
    fa = box['fa'] = _block(_FakeRing([seq]), r1, be, npair, ndm, threshold=1000, on_candidates=got.append)
    sink = Sink(r1, _plane_bytes(npair, ndm))
    sink.start()
    fa.main()
    sink.join(20)
    (hd, _, out), = sink.sequences
    assert hd['threshold'] == 1000 and len(out) == 2
    assert [o.tobytes() for o in out] == [e.tobytes() for e in _expected_planes(x, NT, 16, 20, 1, 2, 2)]
    assert len(got) == 1 and {(c['pair'], c['idm']) for c in got[0]} == {(1, 2)}
    top = max(got[0], key=lambda c: c['snr'])
    assert (top['p'], top['octave'], top['iw']) == (18, 0, 0) and top['ntrial'] >= 2 and abs(top['period'] - 18 * hdr['tsamp']) < 0.1 * hdr['tsamp']
    assert fa.stats['threshold'] == 8.0 and fa.threshold == 8.0 and fa.stats['ncand'] == len(got[0]) and fa.stats['candidates'] == got[0]


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(npair=0), dict(ndm=-1), dict(nwin=0), dict(nwin=NT + 1), dict(nt=128), dict(nt=1 << 15), dict(nt=257), dict(nt=2.0 ** 8),
                                dict(nds=0), dict(nds=1 << 17), dict(nds=1.0), dict(noct=0), dict(noct=7), dict(pmin=15), dict(pmin=21), dict(pmax=65),
                                dict(noct=3, pmax=33), dict(nwidth=0), dict(nwidth=9), dict(nwidth=5), dict(threshold=float('nan')),
                                dict(threshold="8"), dict(on_candidates=3)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(npair=1, ndm=5, nwin=NWIN)
    args.update(SIZES)
    args.update(kw)
    be = FfaBackend()
    with pytest.raises(ValueError, match="BEAM_FFA_SEARCH"):
        BeamFfaSearch(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.fa is None


class _FakeOut:
    name, space = "device-output", "cuda"


def test_constructor_refuses_a_device_output_ring():
    with pytest.raises(ValueError, match="BEAM_FFA_SEARCH"):
        _block(Ring("a"), _FakeOut(), FfaBackend())


@pytest.mark.parametrize("bad", [dict(ndm=None), dict(ndm=4), dict(nbeam=2), dict(nprod=2), dict(tsamp=0.0), dict(dms=[0.0]), dict(dedisp_latency=-1)])
def test_block_refuses_what_is_not_dedispersed_beams(bad):
    npair, ndm = 1, 5
    be = FfaBackend()
    hdr = dedisp_header(npair, ndm, 1)
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NWIN, npair, ndm, 1), np.float32)
    fa = _block(_FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), be)
    with pytest.raises(ValueError, match="BEAM_FFA_SEARCH"):
        fa.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengFfaInitialize", "xengFfaRun", "xengFfaReset", "xengFfaGetInfo", "xengFfaGetStats", "xengFfaCheckGuards", "xengFfaMark", "xengFfaWait",
         "xengFfaTicketDone", "xengFfaSync", "xengFfaDestroy")


def test_backend_forwards_every_call_the_block_makes():
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("ffa_initialize", "ffa_run", "ffa_reset", "ffa_info", "ffa_stats", "ffa_guards_intact", "ffa_mark", "ffa_wait", "ffa_ticket_done", "ffa_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("ffa_initialize", "ffa_run", "ffa_reset", "ffa_mark", "ffa_wait", "ffa_sync"):
        assert callable(getattr(FfaBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are not.
    Initialize refuses every size outside the contract's ranges before it touches a device; Run refuses null and misaligned
    pointers, the getters null results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengFfaRun", "xengFfaReset", "xengFfaMark", "xengFfaTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengFfaInitialize", "xengFfaGetStats", "xengFfaWait", "xengFfaSync", "xengFfaCheckGuards", "xengFfaGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, npair, ndm, nwin, nprod, nds, nt, noct, pmin, pmax, nwidth)
    good = (0, 16, 256, 30, 1, 4, 1 << 14, 4, 256, 512, 8)
    for i, v in ((1, 0), (2, 0), (3, 0), (3, 4 * (1 << 14) + 1), (4, 2), (4, 0), (5, 0), (5, 65537), (6, 128), (6, 1 << 15), (6, (1 << 14) - 4), (7, 0),
                 (7, 7), (7, 6), (8, 15), (8, 513), (9, 255), (9, 1025), (10, 0), (10, 9), (1, 1 << 13)):
        args = list(good)
        args[i] = v
        if (i, v) == (1, 1 << 13):
            args[2] = 1 << 12                                   # 2^25 series
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFfaInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    for args in ((0, 1, 1, 30, 1, 1, 256, 1, 16, 128, 5), (0, 1, 1, 30, 1, 1, 256, 3, 16, 33, 2), (0, 1, 1, 30, 1, 1, 258, 3, 16, 32, 2)):
        with pytest.raises(ffi.XengError) as ei:                # 2^4 > pmin / 2; 2 * 33 > 256 >> 2; 258 is no multiple of 4
            ffi.call("xengFfaInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    with pytest.raises(ffi.XengError) as ei:                    # 2^24 series of 2^14 samples: the state's limit
        ffi.call("xengFfaInitialize", 0, 1 << 12, 1 << 12, 30, 1, 1, 1 << 14, 1, 16, 16, 1)
    assert ei.value.status == INVALID_ARGUMENT
    f = np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n, s = ctypes.c_longlong(), ctypes.c_int()
    for name, args in (("xengFfaRun", (None, 1, 4096, ctypes.byref(s))), ("xengFfaRun", (4096, 1, 4096, None)),
                       ("xengFfaRun", (4100, 1, 4096, ctypes.byref(s))), ("xengFfaRun", (4096, 1, 4104, ctypes.byref(s))),
                       ("xengFfaGetInfo", (None, ctypes.byref(n))), ("xengFfaGetInfo", (ctypes.byref(n), None)), ("xengFfaGetStats", (None,)),
                       ("xengFfaMark", (None,)), ("xengFfaTicketDone", (1, None)), ("xengFfaCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_ffa_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengFfaRun", (4096, 1, 4096, ctypes.byref(s))), ("xengFfaRun", (4096, 1, None, ctypes.byref(s))), ("xengFfaReset", ()),
                       ("xengFfaGetInfo", (ctypes.byref(n), ctypes.byref(n))), ("xengFfaGetStats", (f,)), ("xengFfaMark", (ctypes.byref(t),)),
                       ("xengFfaWait", (1,)), ("xengFfaTicketDone", (1, ctypes.byref(s))), ("xengFfaSync", ()), ("xengFfaCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengFfaDestroy")          # (nothing to destroy: success)
