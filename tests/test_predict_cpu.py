"""UpchanPredict without a GPU: the restatement (tests/predict_ref.py) against the host helper component_visibilities; the identity
that makes the block the major cycle of a Cotton-Schwab CLEAN -- the image of V - M is the dirty image minus the components' point-
spread functions -- in float64 on the CPU; the block on CPU rings with a backend that serves predict_* from the float32 restatement."""
import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ring
from caltech_bifrost_dsp_amd.blocks import UpchanPredict, component_visibilities
from caltech_bifrost_dsp_amd.blocks.imaging import CLEAN_COMPONENT, psf
from caltech_bifrost_dsp_amd.ring import Ring
from tests import clean_ref, image_ref
from tests.calapply_ref import hermitian_bits
from tests.fake_backend import OracleBackend
from tests.image_ref import random_array
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.predict_ref import MODEL, SUBTRACT, case, float_gap, model64, predict, records, scale, word_error
from tests.test_calapply_cpu import ACC_LEN, vis_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

NSTAND, NFINE, NFAVG, NDIR, NCOMP = 6, 4, 2, 7, 5
NGROUP = NFINE // NFAVG
SPAN = NFINE * (2 * NSTAND) ** 2 * 8


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


# ---------------------------------------------------------------- the restatement and the host helper
@pytest.mark.parametrize("nstand,ncomp,nfine,nfavg", [(22, 1, 2, 1), (35, 3, 4, 2), (40, 17, 2, 1)])
def test_restatement_is_the_host_helper(nstand, ncomp, nfine, nfavg):
    """model64 (steering from tests/gaincal_ref.py, one einsum per product) and component_visibilities (its own exponentials) agree to
    rounding, with and without the cross hands; M is Hermitian; the float32 restatement in the kernel's order lies within 1e-6 of
    the scale; an empty record and trailing empties change nothing."""
    tau, freq, comps, V = case(nstand, ncomp, nfine, nfavg)
    n = 2 * nstand
    for cross in (True, False):
        M = component_visibilities(freq, tau, comps, nfavg, cross)
        R = model64(freq, tau, comps, nfavg, cross)
        sc = scale(None, comps, nfavg)
        assert np.abs(M - R).max() <= 1e-13 * sc.max()
        A = M.reshape(nfine, n, n)
        assert np.abs(A - np.conj(A.transpose(0, 2, 1))).max() <= 1e-13 * sc.max()
        if not cross:
            assert not M[:, :, 0, :, 1].any() and not M[:, :, 1, :, 0].any()
        assert float_gap(V, freq, tau, comps, nfavg, cross, MODEL) < 1e-6
    wide = records(nfine // nfavg, ncomp + 3)
    wide[:, :ncomp] = comps
    assert np.array_equal(component_visibilities(freq, tau, wide, nfavg), component_visibilities(freq, tau, comps, nfavg))
    assert predict(V, freq, tau, wide, nfavg, dtype=np.complex64).tobytes() == predict(V, freq, tau, comps, nfavg, dtype=np.complex64).tobytes()
    out = predict(V, freq, tau, comps, nfavg, dtype=np.complex64)
    assert hermitian_bits(out) and out.dtype == np.complex64


def test_host_helper_refuses_what_is_not_a_component_list():
    tau, freq, comps, V = case(22, 3, 4, 2)
    for bad in (dict(nfavg=3), dict(nfavg=0), dict(components=comps[:1]), dict(components=np.zeros((2, 3))), dict(tau=tau[0])):
        args = dict(freq=freq, tau=tau, components=comps, nfavg=2)
        args.update(bad)
        with pytest.raises(ValueError, match="component_visibilities"):
            component_visibilities(**args)
    for field, value in (('pixel', tau.shape[0]), ('pixel', -2), ('C', np.nan)):
        bad = comps.copy()
        bad[field][0, 0] = value
        with pytest.raises(ValueError, match="component_visibilities"):
            component_visibilities(freq, tau, bad, 2)


# ---------------------------------------------------------------- the major cycle's identity
@pytest.mark.parametrize("autos", [False, True])
@pytest.mark.parametrize("nfavg", [1, 3])
def test_image_of_the_subtracted_visibilities_is_the_dirty_image_minus_the_components_psfs(autos, nfavg):
    """image(V - M(components)) = dirty - sum_k C_k psf(., x_k) in float64, in all four words: 22 stands (one of weight 0, one of 0.5),
    40 pixels, 6 channels; components of either sign on all four words, a repeated pixel and an empty record; and with the records of a
    float64 CLEAN of the dirty image, the right-hand side is that run's residual."""
    nstand, npix, nfine = 22, 40, 6
    c = clean_ref.case(nstand, npix, nfine, nfavg, autos)
    V, freq, tau, w = c['V'], c['freq'], c['tau'], c['w']
    ngroup = nfine // nfavg
    rng = np.random.default_rng(5)
    comps = records(ngroup, 6)
    comps['pixel'][:, :5] = rng.integers(0, npix, (ngroup, 5))
    comps['pixel'][:, 3] = comps['pixel'][:, 0]
    comps['pixel'][:, 1] = -1
    comps['C'] = rng.uniform(-2, 3, (ngroup, 6, 4))
    dirty = image_ref.image(V, freq, tau, w, autos, nfavg)
    second = image_ref.image(V - component_visibilities(freq, tau, comps, nfavg), freq, tau, w, autos, nfavg)
    exp = dirty.copy()
    for g in range(ngroup):
        for rec in comps[g]:
            if rec['pixel'] >= 0:
                exp[g] -= rec['C'].astype(np.float64)[:, None] * psf(freq, tau, w, autos, nfavg, rec['pixel'])[g][None]
    sc = np.abs(dirty).max() + np.abs(comps['C']).sum()
    assert np.abs(second - exp).max() <= 1e-12 * sc
    assert np.abs(second - dirty).max() > 1e-3 * sc
    res, rcomps, rstats, _ = clean_ref.clean(c['dirty'], freq, tau, w, autos, nfavg, c['mask'], 5, 0.5)
    again = image_ref.image(V - component_visibilities(freq, tau, rcomps, nfavg), freq, tau, w, autos, nfavg)
    # (clean_ref.clean starts from the dirty image rounded to float32 and subtracts its components before it rounds them into their
    # float32 records: those two roundings are the difference, |psf| <= 1)
    assert np.abs(again - res).max() <= 1e-12 * sc + np.abs(c['dirty'] - dirty).max() + 2.0 ** -24 * np.abs(rcomps['C']).sum(axis=1).max()


# ---------------------------------------------------------------- the block on CPU rings
class PredictBackend(OracleBackend):
    """The oracle backend plus xengPredict* served by the float32 restatement in the kernel's order, with the context's state."""

    def __init__(self):
        super().__init__()
        self.pr, self.calls = None, []
        self.tau = self.freq = self.comps = None
        self.mode = SUBTRACT

    def predict_initialize(self, gpu, nstand, nfine, nfavg, ndir, ncomp_max, cross):
        if nfine % nfavg or not 1 <= ncomp_max <= 4096 or nstand > 512:
            return 1
        self.pr = dict(nstand=nstand, nfine=nfine, nfavg=nfavg, ndir=ndir, ncomp_max=ncomp_max, cross=bool(cross))
        self.tau = self.freq = None
        self.comps, self.mode = records(nfine // nfavg, ncomp_max), SUBTRACT
        self.calls.append('init')
        return 0

    def predict_set_geometry(self, tau, freq):
        u = self.pr
        self.tau, self.freq = np.array(tau, np.float64).reshape(u['ndir'], u['nstand']), np.array(freq, np.float64).reshape(u['nfine'])
        self.calls.append('geometry')
        return 0

    def predict_set_components(self, recs):
        u = self.pr
        assert recs.dtype == CLEAN_COMPONENT and recs.shape == (u['nfine'] // u['nfavg'], u['ncomp_max']) and recs.flags['C_CONTIGUOUS']
        if ((recs['pixel'] < -1) | (recs['pixel'] >= u['ndir'])).any():
            return 1
        self.comps = recs.copy()
        self.calls.append('components')
        return 0

    def predict_set_mode(self, mode):
        if mode not in (SUBTRACT, MODEL):
            return 1
        self.mode = mode
        self.calls.append(('mode', mode))
        return 0

    def predict_run(self, vis_arr, out_arr):
        u = self.pr
        if self.tau is None:
            return 2
        V = vis_arr.numpy().reshape(-1).view(np.uint8).view(np.complex64).reshape(u['nfine'], u['nstand'], 2, u['nstand'], 2)
        y = expect(V, self.freq, self.tau, self.comps, u['nfavg'], u['cross'], self.mode)
        out_arr.numpy().reshape(-1).view(np.uint8)[:y.nbytes] = y.reshape(-1).view(np.uint8)
        self.calls.append('run')
        return 0

    def predict_mark(self):
        return self.beam_mark()

    def predict_wait(self, ticket):
        self.beam_wait(ticket)

    def predict_sync(self):
        pass


def expect(V, freq, tau, comps, nfavg=NFAVG, cross=True, mode=SUBTRACT):
    return np.ascontiguousarray(predict(V, freq, tau, comps, nfavg, cross, mode, np.complex64))


def _setup(seed):
    rng = np.random.default_rng(seed)
    pos, lmn = random_array(rng, NSTAND, 300.0, 3.0), clean_ref.sky(rng, NDIR)
    return rng, pos, lmn


def _comps(rng, n=NCOMP, ngroup=NGROUP):
    r = records(ngroup, n)
    r['pixel'] = rng.integers(0, NDIR, (ngroup, n))
    r['C'] = rng.uniform(-2, 3, (ngroup, n, 4))
    if n > 2:
        r['pixel'][:, 1] = -1
    return r


def _data(rng, n):
    return np.stack([image_ref.hermitian_uneven(rng, NFINE, NSTAND, 0.5, 5.0) for _ in range(n)])


def _vis(span):
    return np.asarray(span).view(np.uint8).reshape(-1).view(np.complex64).reshape(NFINE, NSTAND, 2, NSTAND, 2)


def _freq(hdr):
    return hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(NFINE)


def _filled(c):
    return int((c['pixel'] >= 0).sum(axis=1).max())


def test_block_one_span_per_span_and_header(ring_impl):
    """Source -> UpchanPredict -> Sink, two sequences of three integrations, the second already calibrated with 2 sources subtracted:
    every output span is the restatement of its input span at the sequence's frequencies; the header is the input's plus ncomponents,
    nsubtracted and predict_mode; an image header is not accepted as input."""
    from caltech_bifrost_dsp_amd.blocks import steering_delays
    rng, pos, lmn = _setup(13)
    comps = _comps(rng)
    hdrs = [vis_header(nstand=NSTAND, nfine=NFINE, seq0=1000, fine_sfreq=50e6),
            vis_header(nstand=NSTAND, nfine=NFINE, seq0=5000, fine_sfreq=62e6, calibrated=True, nsubtracted=2)]
    Vs = [_data(rng, 3) for _ in range(2)]
    r0, r1 = Ring("corr-output"), Ring("predict-output")
    be = PredictBackend()
    pr = UpchanPredict(LOG, r0, r1, pos, lmn, nfavg=NFAVG, ncomp_max=NCOMP + 3, components=comps, backend=be)
    sink = Sink(r1, SPAN)
    run_blocks([pr], Source(r0, [(hdrs[s], Vs[s].reshape(-1).view(np.uint8), SPAN) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    tau = steering_delays(pos, lmn)
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert len(spans) == 3 and tag == hd['seq0'] == hdrs[s]['seq0']
        for k in range(3):
            assert _vis(spans[k]).tobytes() == expect(Vs[s][k], _freq(hdrs[s]), tau, comps).tobytes()
        assert (hd['ncomponents'], hd['nsubtracted'], hd['predict_mode']) == (NCOMP - 1, (0, 2)[s] + NCOMP - 1, 'subtract') and hd.get('calibrated') == (None, True)[s]
        assert all(hd[k] == hdrs[s][k] for k in ('nfine', 'fine_sfreq', 'fine_bw_hz', 'nstand', 'npol', 'acc_len', 'nupchan'))
    assert be.calls == ['init', 'components', ('mode', SUBTRACT), 'geometry', 'run', 'run', 'run', 'geometry', 'run', 'run', 'run']
    assert be.comps.shape == (NGROUP, NCOMP + 3) and (be.comps['pixel'][:, NCOMP:] == -1).all()
    assert pr.stats['npredict'] == 6 and pr.stats['ngap'] == 0
    bad = dict(hdrs[0], npix=9)
    with pytest.raises(ValueError, match="UPCHAN_PREDICT"):
        pr._check_header(bad)


def test_block_components_and_mode_at_the_next_integration_and_a_gap_opens_a_new_sequence(ring_impl):
    """Integrations 0..6 of a sequence, 3 never read, no components at first (a copy).  set_components before 1 and before 5, set_mode
    'model' before 2 and back before 6: each begins a sequence of its own whose header names the count and the mode.  The gap ends
    its sequence; 4 opens one whose header starts there.  What is not a component list for this block is refused and changes
    nothing."""
    from caltech_bifrost_dsp_amd.blocks import steering_delays
    rng, pos, lmn = _setup(17)
    hdr = vis_header(nstand=NSTAND, nfine=NFINE, seq0=960)
    V = _data(rng, 7)
    c1, c2 = _comps(rng, 3), _comps(rng, NCOMP)
    box = {}

    def spans():
        for k in (0, 1, 2, 4, 5, 6):
            pr = box['pr']
            if k == 1:
                pr.set_components(c1)
                bad_pixel, bad_word, empty_nan = c1.copy(), c1.copy(), c1.copy()
                bad_pixel['pixel'][0, 0] = NDIR
                bad_word['C'][1, 2, 3] = np.inf
                empty_nan['C'][:, 1] = np.nan           # (record 1 is empty: its words are not looked at)
                for bad in (bad_pixel, bad_word, c1[:1], _comps(rng, NCOMP + 1), np.zeros((NGROUP, 3)), None):
                    with pytest.raises(ValueError, match="UPCHAN_PREDICT"):
                        pr.set_components(bad)
                pr._checked_components(empty_nan)
                with pytest.raises(ValueError, match="UPCHAN_PREDICT"):
                    pr.set_mode('add')
            if k == 2:
                pr.set_mode('model')
            if k == 5:
                pr.set_components(c2)
            if k == 6:
                pr.set_mode('subtract')
            yield k, V[k]

    be = PredictBackend()
    r1 = Ring("predict-output")
    pr = box['pr'] = UpchanPredict(LOG, _FakeRing([_FakeSeq(hdr, spans(), SPAN)]), r1, pos, lmn, nfavg=NFAVG, ncomp_max=NCOMP, backend=be)
    sink = Sink(r1, SPAN)
    sink.start()
    pr.main()
    sink.join(20)
    seqs = sink.sequences
    t = [960 + k * ACC_LEN for k in range(7)]
    assert [(h['seq0'], tag, len(s)) for h, tag, s in seqs] == [(t[0], t[0], 1), (t[1], t[1], 1), (t[2], t[2], 1), (t[4], t[4], 1), (t[5], t[5], 1), (t[6], t[6], 1)]
    n1, n2 = _filled(c1), _filled(c2)
    assert [(h['ncomponents'], h['nsubtracted'], h['predict_mode']) for h, _, _ in seqs] == [(0, 0, 'subtract'), (n1, n1, 'subtract'), (n1, n1, 'model'), (n1, n1, 'model'),
                                                                                             (n2, n2, 'model'), (n2, n2, 'subtract')]
    tau, freq, none = steering_delays(pos, lmn), _freq(hdr), records(NGROUP, 1)
    chain = [(V[0], none, SUBTRACT), (V[1], c1, SUBTRACT), (V[2], c1, MODEL), (V[4], c1, MODEL), (V[5], c2, MODEL), (V[6], c2, SUBTRACT)]
    for k, sp in enumerate([sp for _, _, s in seqs for sp in s]):
        Vk, ck, mk = chain[k]
        assert _vis(sp).tobytes() == expect(Vk, freq, tau, ck, mode=mk).tobytes(), k
    low = np.tril(np.ones((2 * NSTAND, 2 * NSTAND), bool), -1)
    assert _vis(seqs[0][2][0]).reshape(NFINE, 2 * NSTAND, 2 * NSTAND)[:, low].tobytes() == V[0].reshape(NFINE, 2 * NSTAND, 2 * NSTAND)[:, low].tobytes()
    assert be.calls == ['init', 'components', ('mode', SUBTRACT), 'geometry', 'run', 'components', 'run', ('mode', MODEL), 'run', 'run', 'components', 'run',
                        ('mode', SUBTRACT), 'run']
    assert pr.stats['ngap'] == 1 and pr.stats['npredict'] == 6


@pytest.mark.parametrize("kw", [dict(nfavg=0), dict(nfavg=1.5), dict(ncomp_max=0), dict(ncomp_max=4097), dict(mode='add'), dict(components=np.zeros((2, 3))),
                                dict(positions=np.zeros((513, 3))), dict(positions=np.zeros((6, 2))), dict(lmn=np.full((7, 3), np.nan))])
def test_constructor_refuses_bad_arguments(kw):
    rng, pos, lmn = _setup(3)
    be = PredictBackend()
    args = dict(positions=pos, lmn=lmn, nfavg=NFAVG, ncomp_max=NCOMP)
    args.update(kw)
    with pytest.raises(ValueError, match="UPCHAN_PREDICT"):
        UpchanPredict(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.pr is None
    UpchanPredict(LOG, Ring("a"), Ring("b"), pos, lmn, nfavg=NFAVG, ncomp_max=4096, components=_comps(rng), mode='model', cross=False, backend=be)


@pytest.mark.parametrize("bad", [dict(npol=1), dict(nstand=7), dict(nfine=None), dict(nfine=0), dict(nfine=5), dict(nbit=8), dict(complex=False), dict(npix=7), dict(nsrc=2),
                                 dict(acc_len=0), dict(nsubtracted=-1)])
def test_block_refuses_what_is_not_its_visibilities(bad):
    """npol != 2, a stand count that differs from the block's, a channel count nfavg does not divide, and headers that are not
    visibilities: refused at the sequence, before anything is run."""
    rng, pos, lmn = _setup(3)
    be = PredictBackend()
    hdr = vis_header(nstand=NSTAND, nfine=NFINE)
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NFINE, NSTAND, 2, NSTAND, 2), np.complex64)
    pr = UpchanPredict(LOG, _FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), pos, lmn, nfavg=NFAVG, ncomp_max=NCOMP, backend=be)
    with pytest.raises(ValueError, match="UPCHAN_PREDICT"):
        pr.main()
    assert 'run' not in be.calls
