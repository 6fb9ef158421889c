"""UpchanImageSearch without a GPU, both ring implementations: the restatement (tests/imsearch_ref.py) against a term-by-term loop and
on a planted dispersed box pulse; image_candidates on hand-built planes (clusters, ties, an empty plane, max_above); the block on
CPU rings with a backend that keeps the context's state and serves xengImsearch* by the float32 restatement -- spans within and
across sequences, the output header, a gap (reset, a new output sequence), `threshold` and `weights` landing at the next
integration, the `sample` arithmetic against a pulse planted at a known sample, a cleaned input span, refusals -- and the C entry
points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanImageSearch, image_candidates
from caltech_bifrost_dsp_amd.blocks.image_search import IMSEARCH_RECORD, as_records, group_frequencies, image_dm_delays, kappa
from caltech_bifrost_dsp_amd.ring import Ring
from tests.fake_backend import OracleBackend
from tests.imsearch_ref import RECORD, imsearch, imsearch_naive, plant, planted_case, ramp_delays, records
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
NONE_BYTES = np.array([(0.0, -1, -1)], RECORD).tobytes()


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


# ---------------------------------------------------------------- the restatement
def test_restatement_is_the_definition():
    """The vectorised restatement in float64 against the one-term-at-a-time loop: the same (n, d, iw, pixel) are scored, to 1e-9
    the same scores and the same records -- with a group of weight 0 that holds NaN, weights set again after 21 integrations, a
    pixel constant in a used group and a NaN in one used word."""
    rng = np.random.default_rng(2)
    npix, ngroup, ndm, nint, nstat, nwidth = 6, 4, 3, 44, 8, 3
    x = rng.normal(100.0, 5.0, (nint, ngroup, 4, npix)).astype(np.float32)
    x[:, 1] = np.nan
    x[:, 2, :2, 4] = 7.0
    x[19, 0, 0, 2] = np.nan
    delays = ramp_delays(ndm, ngroup, 5)
    w = [(0, np.array([1, 0, 2, 1], np.float32)), (21, np.array([2, 0, 1, 1], np.float32))]
    ref = imsearch(x, delays, w, nstat, nwidth, np.float64)
    score, scored, recs = imsearch_naive(x, delays, w, nstat, nwidth)
    assert np.array_equal(ref['scored'], scored) and scored.any() and not scored[:, :, :, 4].any()
    assert np.allclose(ref['score'][scored], score[scored], rtol=1e-9, atol=1e-9)
    assert not scored[21, :, 1:].any() and not scored[22, :, 2].any() and scored[24, :, 2].any() and scored[20, :, 2].any()
    for n in range(nint):
        for p in range(npix):
            snr, idm, iw = recs[n][p]
            assert (ref['idm'][n, p], ref['iw'][n, p]) == (idm, iw), (n, p)
            assert abs(ref['snr'][n, p] - snr) <= 1e-9 * max(1.0, abs(snr))
    gone = ~ref['scored'][:, :, 0, 2].any(axis=1)
    assert gone[:nstat].all() and not gone[nstat + 5:19].any() and gone[24 + 5:32].all() and not gone[32 + 5:].any()


def test_restatement_recovers_the_planted_pulse():
    """The planted dispersed box pulse (imsearch_ref.planted_case): recovered at n = 46, trial 2, width 2 in float32 and float64,
    the best record of the whole run.  Expected: 150 / sigma(I) = 7.35 per group and integration, times sum w = 5 groups' worth, times 2
    integrations, times kappa rho = 1 / sqrt(14): 19.6 with unit noise; here 21.3, the next best of any other record 15.2 (the same
    pulse under a neighbouring trial or width)."""
    x, delays, w, (n, pix, idm, iw) = planted_case()
    for dtype in (np.float32, np.float64):
        ref = imsearch(x, delays, w, 16, 3, dtype)
        assert (ref['idm'][n, pix], ref['iw'][n, pix]) == (idm, iw)
        assert np.unravel_index(ref['snr'].argmax(), ref['snr'].shape) == (n, pix)
        rest = ref['snr'].astype(np.float64).copy()
        rest[n, pix] = 0
        assert 19.6 - 3 < ref['snr'][n, pix] < 19.6 + 3 and rest.max() < 16.5 < ref['snr'][n, pix], (ref['snr'][n, pix], rest.max())
        assert (ref['idm'][:16 + 12] == -1).all() and (ref['idm'][16 + 12:] >= 0).all()
        assert np.isclose(ref['score'][n, idm, iw, pix], ref['z'][n - 1:n + 1, idm, pix].sum() / np.sqrt(7.0) / np.sqrt(2.0), rtol=1e-5)


# ---------------------------------------------------------------- image_candidates
def _sky(n):
    """n unit vectors along a meridian, 0.01 rad apart, the first at the zenith"""
    th = 0.01 * np.arange(n)
    return np.stack([np.sin(th), np.zeros(n), np.cos(th)], axis=1)


def _plane(n):
    p = np.zeros(n, IMSEARCH_RECORD)
    p['idm'] = p['iw'] = -1
    return p


def test_image_candidates_clusters_ties_empty_and_max_above():
    lmn, dms, widths = _sky(12), [0.0, 1.5, 3.0], [1, 2, 4]
    p = _plane(12)
    assert image_candidates(p, 5.0, lmn, 0.025, dms, widths) == [] and not image_candidates(p, 5.0, lmn, 0.025, dms, widths).saturated
    assert image_candidates(p, -1.0, lmn, 0.025, dms, widths) == []        # (a pixel with nothing scored is never above)
    for pix, snr, idm, iw in ((2, 9.0, 1, 0), (3, 12.0, 2, 1), (4, 9.0, 1, 0), (5, 8.0, 0, 2), (6, 7.0, 0, 0), (10, 12.0, 1, 2), (11, 4.0, 0, 0)):
        p[pix] = (snr, idm, iw)
    c = image_candidates(p, 5.0, lmn, 0.025, dms, widths)
    # 3 and 10 tie at 12: pixel order.  3 takes 2 and 4 (0.01 away, in pixel order: they tie too) and 5 (0.02); 6 is 0.03 from 3 and a
    # candidate of its own although it is 0.01 from the member 5; 11 is below the threshold
    assert [(d['pixel'], d['members']) for d in c] == [(3, [3, 2, 4, 5]), (10, [10]), (6, [6])] and not c.saturated
    assert (c[0]['snr'], c[0]['idm'], c[0]['dm'], c[0]['iw'], c[0]['width'], c[0]['window']) == (12.0, 2, 3.0, 1, 2, 0)
    assert c[0]['lmn'] == tuple(lmn[3]) and (c[1]['dm'], c[1]['width']) == (1.5, 4)
    assert [d['pixel'] for d in image_candidates(p, 12.0, lmn, 0.025, dms, widths)] == [3, 10]        # (at exactly a value: above)
    assert [d['pixel'] for d in image_candidates(p, 5.0, lmn, 0.0, dms, widths)] == [3, 10, 2, 4, 5, 6]
    top = image_candidates(p, 5.0, lmn, 0.0, dms, widths, max_above=3)
    assert [d['pixel'] for d in top] == [3, 10, 2] and top.saturated
    assert image_candidates(p.view(np.uint8), 5.0, lmn, 0.025, dms, widths) == c
    p['snr'][7] = np.nan
    p['idm'][7] = p['iw'][7] = 0
    assert image_candidates(p, 5.0, lmn, 0.025, dms, widths) == c
    with pytest.raises(ValueError):
        image_candidates(p, 5.0, lmn[:5], 0.025, dms, widths)
    with pytest.raises(ValueError):
        image_candidates(p, 5.0, lmn, 0.025, dms[:2], widths)
    with pytest.raises(ValueError):
        as_records(np.zeros(12, np.uint8))
    assert kappa([1, 1, 0, 2, 1]) == np.float32(1 / np.sqrt(7.0)) and kappa(np.ones(4)) == np.float32(0.5)
    with pytest.raises(ValueError):
        kappa([0, 0])


# ---------------------------------------------------------------- the block on CPU rings
NPIX, NGROUP, NFAVG, ACC_LEN, NCHAN, TINT = 10, 5, 2, 1000, 5, 1.0
DMS = [0.0, 2.8, 5.6, 8.3]


def image_header(npix=NPIX, seq0=0, **extra):
    """The sequence header UpchanImage writes (upchan_image_block.py output_header), channel groups at 40, 45 ... 60 MHz and
    integrations of 1 s: DM 8.3 lags 12 integrations at the bottom of the band."""
    nfine = NGROUP * NFAVG
    hdr = source_header(NCHAN, 8, 2, seq0=seq0, sfreq=40e6, chan_bw=ACC_LEN * NCHAN / TINT / NCHAN)
    hdr.update(nupchan=2, fine_lo=0, nfine=nfine, fine_bw_hz=2.5e6, fine_sfreq=38.75e6, nframe_per_integration=ACC_LEN // 2, acc_len=ACC_LEN,
               npix=npix, nfavg=NFAVG, nprod=4, autos=False, nbit=32, complex=False, image_sfreq=40e6, image_bw_hz=5e6)
    hdr.update(extra)
    return hdr


def table():
    t = image_dm_delays(group_frequencies(image_header(), NGROUP), DMS, TINT)
    assert t.shape == (4, NGROUP) and t.max() == t[3, 0] == 12 and (t[:, -1] == 0).all() and (np.diff(t, axis=1) <= 0).all() and (t[0] == 0).all()
    return t


class ImsearchBackend(OracleBackend):
    """The oracle backend plus xengImsearch* served by the float32 restatement, with the context's state: the images since the
    reset, the weights and when they were set."""

    def __init__(self):
        super().__init__()
        self.ctx, self.calls = None, []

    def imsearch_initialize(self, gpu, npix, ngroup, ndm, max_delay, nwidth, nstat):
        self.ctx = dict(npix=npix, ngroup=ngroup, ndm=ndm, max_delay=max_delay, nwidth=nwidth, nstat=nstat)
        self.x, self.delays, self.sched = [], None, [(0, np.ones(ngroup, np.float32))]
        self.calls.append(('init', ngroup))
        return 0

    def imsearch_set_delays(self, delays):
        assert delays.dtype == np.int32 and delays.shape == (self.ctx['ndm'], self.ctx['ngroup']) and delays.max() <= self.ctx['max_delay']
        self.delays, self.x, self.sched = delays.copy(), [], [(0, self.sched[-1][1])]
        self.calls.append('delays')
        return 0

    def imsearch_set_weights(self, w):
        assert w.dtype == np.float32 and w.shape == (self.ctx['ngroup'],)
        self.sched = [e for e in self.sched if e[0] < len(self.x)] + [(len(self.x), w.copy())]
        self.calls.append('weights')
        return 0

    def imsearch_run(self, in_arr, out_arr):
        u = self.ctx
        assert self.delays is not None
        words = np.ascontiguousarray(in_arr.numpy()).reshape(-1).view(np.uint8).view(np.float32)
        self.x.append(words[:u['ngroup'] * 4 * u['npix']].reshape(u['ngroup'], 4, u['npix']).copy())
        ref = imsearch(np.stack(self.x), self.delays, list(self.sched), u['nstat'], u['nwidth'], np.float32)
        out_arr.numpy().reshape(-1).view(np.uint8)[...] = records(ref, len(self.x) - 1).view(np.uint8)
        self.calls.append('run')
        return 0

    def imsearch_reset(self):
        self.x, self.sched = [], [(0, self.sched[-1][1])]
        self.calls.append('reset')

    def imsearch_mark(self):
        return self.beam_mark()

    def imsearch_wait(self, ticket):
        self.beam_wait(ticket)

    def imsearch_sync(self):
        pass


def _noise(rng, nint, npix=NPIX):
    x = np.full((nint, NGROUP, 4, npix), np.nan, np.float32)
    x[:, :, :2] = rng.integers(0, 50, (nint, NGROUP, 2, npix)).astype(np.float32)
    return x


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _block(iring, oring, be, npix=NPIX, **kw):
    args = dict(lmn=_sky(npix), dms=DMS, nwidth=2, nstat=4, threshold=100.0, radius=0.015, max_delay=12, backend=be)
    args.update(kw)
    return UpchanImageSearch(LOG, iring, oring, **args)


SPAN = NGROUP * 4 * NPIX * 4


def test_block_spans_within_and_across_sequences():
    """Source -> UpchanImageSearch -> Sink on in-repo rings, two sequences of 22 integrations, nstat = 4, S = 12.  The baselines, the
    delayed series and the boxcars cross the spans of a sequence and not the sequences; every plane equals the restatement's; the
    output header adds ndm, dms, nwidth, widths, nstat, imsearch_latency, tint, threshold."""
    rng = np.random.default_rng(5)
    xs = [_noise(rng, 22) for _ in range(2)]
    hdrs = [image_header(seq0=100000 * (s + 1)) for s in range(2)]
    r0, r1 = Ring("im-output"), Ring("is-output")
    be = ImsearchBackend()
    got = []
    blk = _block(r0, r1, be, threshold=2.5, on_candidates=got.append)
    sink = Sink(r1, NPIX * 8)
    run_blocks([blk], Source(r0, [(hdrs[s], xs[s], SPAN) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    ncand = 0
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hdrs[s]['seq0'] and hd['seq0'] == hdrs[s]['seq0'] and len(spans) == 22
        ref = imsearch(xs[s], table(), np.ones(NGROUP, np.float32), 4, 2, np.float32)
        for k, o in enumerate(spans):
            assert o.tobytes() == records(ref, k).tobytes(), (s, k)
            ncand += len(image_candidates(records(ref, k), 2.5, _sky(NPIX), 0.015, DMS, [1, 2]))
        assert spans[15].tobytes() == NONE_BYTES * NPIX and (as_records(spans[17], NPIX)['idm'] >= 0).all()
    hd = sink.sequences[0][0]
    assert (hd['ndm'], hd['dms'], hd['nwidth'], hd['widths'], hd['nstat'], hd['imsearch_latency'], hd['tint'], hd['threshold']) == \
        (4, DMS, 2, [1, 2], 4, 12, TINT, 2.5)
    assert hd['npix'] == NPIX and hd['image_sfreq'] == 40e6
    assert be.calls == [('init', NGROUP), 'weights', 'delays'] + ['run'] * 22 + ['weights', 'delays'] + ['run'] * 22
    assert blk.stats['nsearched'] == 44 and blk.stats['ncand'] == ncand == sum(len(c) for c in got) and ncand > 0
    assert all(c['window'] >= 16 and c['sample'] == 100000 * (1 + (c['window'] < 0)) + (c['window'] - 12 - c['width'] + 1) * ACC_LEN
               for c in got[0])


def test_block_gap_resets_and_restarts_the_output_sequence():
    """Integrations 0-2 and 4-24 of a sequence (3 never read): the context is reset, the output restarts in a sequence of its own at
    integration 4's sample, and what follows is the restatement of a run that begins at integration 4."""
    rng = np.random.default_rng(11)
    x = _noise(rng, 25)
    hdr = image_header(seq0=7000)
    seen = [(k, np.ascontiguousarray(x[k])) for k in (0, 1, 2) + tuple(range(4, 25))]
    be = ImsearchBackend()
    r1 = Ring("is-output")
    blk = _block(_FakeRing([_FakeSeq(hdr, seen, SPAN)]), r1, be)
    sink = Sink(r1, NPIX * 8)
    sink.start()
    blk.main()
    sink.join(20)
    assert be.calls == [('init', NGROUP), 'weights', 'delays', 'run', 'run', 'run', 'reset'] + ['run'] * 21
    (h0, t0, a), (h1, t1, b) = sink.sequences
    assert (h0['seq0'], t0, h1['seq0'], t1) == (7000, 7000, 7000 + 4 * ACC_LEN, 7000 + 4 * ACC_LEN) and (len(a), len(b)) == (3, 21)
    ref = imsearch(x[4:], table(), np.ones(NGROUP, np.float32), 4, 2, np.float32)
    for k, o in enumerate(b):
        assert o.tobytes() == records(ref, k).tobytes(), k
    assert (as_records(b[15], NPIX)['idm'] == -1).all() and (as_records(b[17], NPIX)['idm'] >= 0).all() and blk.stats['ngap'] == 1


def test_block_threshold_and_weights_land_at_the_next_integration():
    """A `threshold` command that arrives before integration 19 and a `weights` command before 20 (set_weights before 23): planes
    0-18 are judged at 100 (nothing), the later ones at 1.0; the planes equal the restatement with the weights set when 20 and 23
    integrations had been taken.  Commands that are not numbers, not ngroup weights or all zero are refused and change nothing."""
    rng = np.random.default_rng(13)
    x = _noise(rng, 26)
    hdr = image_header()
    w1, w2 = [1.0, 0.0, 2.0, 1.0, 1.0], [1.0, 1.0, 1.0, 0.0, 3.0]
    be = ImsearchBackend()
    r1 = Ring("is-output")
    box, got = {}, []

    def spans():
        for k in range(26):
            b = box['blk']
            if k == 19:
                b.process_command_strings(_cmd(threshold=1.0))
                assert b.last_response['val']['status'] == 'normal'
            if k == 20:
                b.process_command_strings(_cmd("2", weights=w1))
                assert b.last_response['val']['status'] == 'normal'
            if k == 21:
                for bad in (dict(threshold="high"), dict(threshold=float('nan')), dict(weights=[1.0, 1.0]), dict(weights=[0.0] * 5),
                            dict(weights=[1.0, -1.0, 1.0, 1.0, 1.0]), dict(weights="x")):
                    b.process_command_strings(_cmd("3", **bad))
                    assert b.last_response['val']['status'] == 'error', bad
            if k == 23:
                b.set_weights(w2)
                with pytest.raises(ValueError, match="UPCHAN_IMAGE_SEARCH"):
                    b.set_weights([1.0, 2.0])
            yield k, np.ascontiguousarray(x[k])

    blk = box['blk'] = _block(_FakeRing([_FakeSeq(hdr, spans(), SPAN)]), r1, be, on_candidates=got.append)
    sink = Sink(r1, NPIX * 8)
    sink.start()
    blk.main()
    sink.join(20)
    (hd, _, out), = sink.sequences
    assert hd['threshold'] == 100.0 and len(out) == 26
    sched = [(0, np.ones(NGROUP, np.float32)), (20, np.array(w1, np.float32)), (23, np.array(w2, np.float32))]
    ref = imsearch(x, table(), sched, 4, 2, np.float32)
    for k, o in enumerate(out):
        assert o.tobytes() == records(ref, k).tobytes(), k
    assert as_records(out[20], NPIX)['iw'].max() == 0 and as_records(out[23], NPIX)['iw'].max() == 0 and (as_records(out[23], NPIX)['idm'] >= 0).all()
    exp = [list(image_candidates(o, 1.0, _sky(NPIX), 0.015, DMS, [1, 2])) for o in out]
    assert len(exp[18]) > 0
    strip = [[{f: v for f, v in c.items() if f not in ('sample', 'window')} for c in cs] for cs in got]
    assert strip == [[{f: v for f, v in c.items() if f != 'window'} for c in e] for e in exp[19:] if e] and len(strip) >= 2
    assert blk.stats['threshold'] == 1.0 and blk.threshold == 1.0 and blk.stats['ncand'] == sum(len(c) for c in got)
    assert be.calls.count('weights') == 3 and be.calls.index('weights', 4) == 3 + 20


def _planted_through_the_block(cleaned):
    """The planted pulse of planted_case's shape on the header's own delay table: 70 pixels, +150 for 2 integrations along trial 2,
    the top of the band at integration 33 = sample seq0 + 33 acc_len."""
    npix, seq0 = 70, 4096
    rng = np.random.default_rng(1)
    x = _noise(rng, 64, npix)
    t = table()
    plant(x, t[2], 33, 2, 33)
    w = [1.0, 1.0, 0.0, 2.0, 1.0]
    span = NGROUP * 4 * npix * 4
    hdr = image_header(npix=npix, seq0=seq0)
    data = x
    if cleaned:                                 # (UpchanClean's span: the residual at the front, components and stats behind it)
        comp = 4 * 32 * NGROUP
        span_bytes = span + comp + 16 * NGROUP
        hdr.update(cleaned=True, niter=4, comp_offset=span, stats_offset=span + comp, span_bytes=span_bytes)
        data = np.full((64, span_bytes // 4), np.nan, np.float32)
        data[:, :span // 4] = x.reshape(64, -1)
        span = span_bytes
    got = []
    be = ImsearchBackend()
    blk = _block(Ring("im-output"), Ring("is-output"), be, npix=npix, nwidth=3, nstat=16, threshold=8.0, weights=w, on_candidates=got.extend)
    sink = Sink(blk.oring, npix * 8)
    run_blocks([blk], Source(blk.iring, [(hdr, data, span)]), [sink])
    (_, _, planes), = sink.sequences
    ref = imsearch(x, t, np.array(w, np.float32), 16, 3, np.float32)
    assert len(planes) == 64
    for k, o in enumerate(planes):
        assert o.tobytes() == records(ref, k).tobytes(), k
    best = max(got, key=lambda c: c['snr'])
    assert (best['pixel'], best['idm'], best['dm'], best['width'], best['window']) == (33, 2, DMS[2], 2, 33 + 12 + 1)
    assert best['sample'] == seq0 + 33 * ACC_LEN and best['snr'] > 15 and best['members'] == [33]
    assert all(c['pixel'] == 33 for c in got if c['snr'] > 12)


@pytest.mark.parametrize("cleaned", [False, True])
def test_block_sample_is_the_planted_sample(cleaned):
    """The brightest candidate is the planted pixel, trial, width and sample -- from UpchanImage's spans and from UpchanClean's, whose
    size comes from the header's span_bytes and whose front alone is read (what lies behind it is NaN here)."""
    _planted_through_the_block(cleaned)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(lmn=np.zeros((4, 2))), dict(dms=[]), dict(dms=[0.0, -1.0]), dict(dms=[float('nan')]), dict(nwidth=0), dict(nwidth=7),
                                dict(nstat=1), dict(nstat=(1 << 20) + 1), dict(nwidth=6, nstat=31), dict(threshold=float('nan')), dict(threshold="8"),
                                dict(radius=-1.0), dict(max_delay=-1), dict(max_above=0), dict(on_candidates=3), dict(weights=[0.0, 0.0]),
                                dict(weights=[1.0, float('inf')])])
def test_constructor_refuses_bad_arguments(kw):
    be = ImsearchBackend()
    with pytest.raises(ValueError, match="UPCHAN_IMAGE_SEARCH"):
        _block(Ring("a"), Ring("b"), be, **kw)
    assert be.ctx is None


class _FakeOut:
    name, space = "device-output", "cuda"


def test_constructor_refuses_a_device_output_ring():
    with pytest.raises(ValueError, match="UPCHAN_IMAGE_SEARCH"):
        _block(Ring("a"), _FakeOut(), ImsearchBackend())


@pytest.mark.parametrize("bad", [dict(npix=NPIX + 1), dict(npix=None), dict(nprod=1), dict(nfavg=3), dict(nfine=None), dict(bw_hz=None), dict(nchan=None),
                                 dict(bw_hz=0.0), dict(image_sfreq=None), dict(image_bw_hz=0.0), dict(complex=True),
                                 dict(cleaned=True, stats_offset=16)])
def test_block_refuses_what_is_not_images_of_this_list(bad):
    """Another pixel count, other products, an nfavg that does not divide nfine, no bw_hz or nchan (no integration length in
    seconds), no group frequencies, a cleaned span that ends inside the image: ValueError before any run."""
    be = ImsearchBackend()
    hdr = image_header()
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NGROUP, 4, NPIX), np.float32)
    blk = _block(_FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), be)
    with pytest.raises(ValueError, match="UPCHAN_IMAGE_SEARCH|image_search"):
        blk.main()
    assert 'run' not in be.calls


def test_block_refuses_a_sweep_longer_than_max_delay_and_other_weights():
    x = np.zeros((NGROUP, 4, NPIX), np.float32)
    for kw in (dict(max_delay=11), dict(weights=[1.0, 1.0, 1.0])):
        be = ImsearchBackend()
        blk = _block(_FakeRing([_FakeSeq(image_header(), [(0, x)], x.nbytes)]), Ring("b"), be, **kw)
        with pytest.raises(ValueError, match="UPCHAN_IMAGE_SEARCH"):
            blk.main()
        assert be.ctx is None


# ---------------------------------------------------------------- the C entry points
NAMES = ("xengImsearchInitialize", "xengImsearchSetDelays", "xengImsearchSetWeights", "xengImsearchRun", "xengImsearchReset", "xengImsearchGetInfo",
         "xengImsearchGetBaseline", "xengImsearchCheckGuards", "xengImsearchMark", "xengImsearchWait", "xengImsearchTicketDone", "xengImsearchSync",
         "xengImsearchDestroy")


def test_backend_forwards_every_call_the_block_makes():
    """HipBackend has a method for each imsearch_* call of the block (and the fake backend above has the same ones)."""
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("imsearch_initialize", "imsearch_set_delays", "imsearch_set_weights", "imsearch_run", "imsearch_reset", "imsearch_info",
              "imsearch_baseline", "imsearch_guards_intact", "imsearch_mark", "imsearch_wait", "imsearch_ticket_done", "imsearch_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("imsearch_initialize", "imsearch_set_delays", "imsearch_set_weights", "imsearch_run", "imsearch_reset", "imsearch_mark", "imsearch_wait",
              "imsearch_sync"):
        assert callable(getattr(ImsearchBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are not.
    Initialize refuses bad sizes, too many pixels or trials, nwidth, nstat, a boxcar longer than a block and too much state before it
    touches a device; the setters and Run refuse null and misaligned pointers, GetInfo / GetBaseline / CheckGuards / Mark /
    TicketDone null results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengImsearchRun", "xengImsearchReset", "xengImsearchMark", "xengImsearchTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengImsearchInitialize", "xengImsearchSetDelays", "xengImsearchSetWeights", "xengImsearchGetBaseline", "xengImsearchWait",
                 "xengImsearchSync", "xengImsearchCheckGuards", "xengImsearchGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, npix, ngroup, ndm, max_delay, nwidth, nstat)
    for args in ((0, 0, 24, 64, 128, 5, 64), (0, 65536, 0, 64, 128, 5, 64), (0, 65536, 24, 0, 128, 5, 64), (0, 65536, 24, 64, -1, 5, 64),
                 (0, (1 << 24) + 1, 24, 64, 128, 5, 64), (0, 65536, 24, 1025, 128, 5, 64), (0, 65536, 24, 64, 128, 0, 64), (0, 65536, 24, 64, 128, 7, 64),
                 (0, 65536, 24, 64, 128, 5, 1), (0, 65536, 24, 64, 128, 5, (1 << 20) + 1), (0, 65536, 24, 64, 128, 5, 15), (0, 65536, 24, 64, 1024, 5, 64),
                 (0, 1 << 24, 24, 64, 0, 5, 64)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImsearchInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    f = np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n, s, i = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
    t = ctypes.c_ulonglong()
    for name, args in (("xengImsearchSetDelays", (None,)), ("xengImsearchSetWeights", (None,)), ("xengImsearchRun", (None, 16)), ("xengImsearchRun", (16, None)),
                       ("xengImsearchRun", (20, 16)), ("xengImsearchRun", (16, 24)), ("xengImsearchGetInfo", (None, ctypes.byref(s))),
                       ("xengImsearchGetInfo", (ctypes.byref(n), None)), ("xengImsearchGetBaseline", (None, f, f)), ("xengImsearchGetBaseline", (f, f, None)),
                       ("xengImsearchCheckGuards", (None,)), ("xengImsearchMark", (None,)), ("xengImsearchTicketDone", (1, None))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    d = np.zeros(4, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    for name, args in (("xengImsearchSetDelays", (d,)), ("xengImsearchSetWeights", (f,)), ("xengImsearchRun", (16, 32)), ("xengImsearchReset", ()),
                       ("xengImsearchGetInfo", (ctypes.byref(n), ctypes.byref(s))), ("xengImsearchGetBaseline", (f, f, f)),
                       ("xengImsearchCheckGuards", (ctypes.byref(i),)), ("xengImsearchMark", (ctypes.byref(t),)), ("xengImsearchWait", (1,)),
                       ("xengImsearchTicketDone", (1, ctypes.byref(i))), ("xengImsearchSync", ())):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, (name, args)
    assert ffi.lib().xengImsearchDestroy() == 0
