"""UpchanClean without a GPU: the point-spread function of blocks/imaging.py against the image of a point source and against the
restatement (tests/clean_ref.py); the restatement's own loop (what it subtracts, its ties, its stops); restore; the round trip
image -> components -> sky model -> tests/calapply_ref.apply -> image; the block on CPU rings (both implementations) with a backend
that serves clean_* from the float32 restatement -- header keys, one output span per input span, the set_* calls and the commands at
the next integration, a gap, the refusals -- and the C entry points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import (UpchanClean, clean_components, clean_layout, components_to_model, image_norm, psf, restore, steering_delays,
                                            stokes_i)
from caltech_bifrost_dsp_amd.blocks.imaging import CLEAN_COMPONENT, CLEAN_STATS
from caltech_bifrost_dsp_amd.ring import Ring
from tests import calapply_ref, clean_ref
from tests.clean_ref import CleanBackend, case, clean, fractions, pack_span, sky
from tests.image_ref import image, point_source, random_array
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
NSTAND, NFINE, NFAVG, NPIX, ACC_LEN, NITER = 5, 4, 2, 9, 96, 3
NGROUP = NFINE // NFAVG
FINE_BW = 23925.78125 / 2
SHAPES = [(22, 49), (35, 81), (35, 324)]


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


# ---------------------------------------------------------------- the point-spread function
@pytest.mark.parametrize("nstand,npix", SHAPES)
@pytest.mark.parametrize("autos", [False, True])
@pytest.mark.parametrize("nfavg", [1, 3])
def test_psf_is_the_image_of_a_point_source(nstand, npix, autos, nfavg):
    """psf(x0) against tests/image_ref.image of point_source at x0, weights 0 and 0.5 among the stands: XX, YY and Re XY are the PSF and
    Im XY nothing, to 1e-8 (the complex64 rounding of the test source: 3e-9 measured); PSF(x0, x0) = 1; the restatement's float64 form is
    the same function and its float32 form agrees to 1e-5 of a unit source."""
    c = case(nstand, npix, 6, nfavg, autos)
    x0 = int(c['src'][0])
    P = psf(c['freq'], c['tau'], c['w'], autos, nfavg, x0)
    I = image(point_source(c['freq'], c['tau'][x0]), c['freq'], c['tau'], c['w'], autos, nfavg)
    assert P.shape == (6 // nfavg, npix) and np.abs(P[:, x0] - 1).max() < 1e-12
    assert np.abs(I[:, :3] - P[:, None]).max() < 1e-8 and np.abs(I[:, 3]).max() < 1e-8
    fr = fractions(c['freq'], c['tau'])
    assert np.abs(clean_ref.psf(fr, c['w'], autos, nfavg, x0) - P).max() < 1e-12
    P32 = clean_ref.psf(fr, c['w'], autos, nfavg, x0, np.float32)
    assert P32.dtype == np.float32 and np.abs(P32 - P).max() < 1e-5
    with pytest.raises(ValueError):
        psf(c['freq'], c['tau'], c['w'], autos, nfavg, npix)
    with pytest.raises(ValueError):
        psf(c['freq'], c['tau'], c['w'][:-1], autos, nfavg, 0)


def test_a_stand_of_weight_zero_is_the_stand_deleted():
    c = case(22, 49, 4, 2, False)
    keep = c['w'] != 0
    assert not keep.all()
    bad = c['tau'].copy()
    bad[:, ~keep] = 1e3                           # (never turned into a phase)
    a = psf(c['freq'], bad, c['w'], False, 2, 5)
    b = psf(c['freq'], c['tau'][:, keep], c['w'][keep], False, 2, 5)
    assert np.abs(a - b).max() < 1e-13
    fr = fractions(c['freq'], bad)
    assert np.array_equal(clean_ref.psf(fr, c['w'], False, 2, 5, np.float32), clean_ref.psf(fractions(c['freq'], c['tau'][:, keep]), c['w'][keep], False, 2, 5, np.float32))


# ---------------------------------------------------------------- the restatement's loop
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_subtracts_gain_times_the_peak_and_records_it(dtype):
    """The residual is the dirty image minus sum_k C_k PSF(x_k); every C_k is gain times the residual before it at x_k, every x_k the
    window's brightest pixel then; ncomp = niter, reason 0, and the reported peak is the residual's; the records past ncomp hold -1."""
    c = case(22, 49, 4, 2, False)
    R, comps, stats, gaps = clean(c['dirty'], c['freq'], c['tau'], c['w'], False, 2, c['mask'], 5, 0.5, dtype=dtype)
    tol = 1e-12 if dtype == np.float64 else 2e-6
    for g in range(2):
        acc = c['dirty'][g].astype(np.float64)
        for k in range(5):
            x = comps['pixel'][g, k]
            a = np.where(c['mask'] != 0, np.abs(acc[0] + acc[1]), -1)
            assert x == np.argmax(a) and c['mask'][x]
            assert np.abs(comps['C'][g, k] - 0.5 * acc[:, x]).max() < 1e-5 and abs(comps['I'][g, k] - (acc[0, x] + acc[1, x])) < 1e-5
            acc = acc - (0.5 * acc[:, x])[:, None] * psf(c['freq'], c['tau'], c['w'], False, 2, x)[g][None]
        assert np.abs(acc - R[g]).max() < tol * np.abs(c['dirty'][g]).max()
        assert stats['peak'][g] == np.float32(np.abs(np.where(c['mask'] != 0, R[g, 0] + R[g, 1], 0)).max())
    assert (stats['ncomp'] == 5).all() and (stats['reason'] == 0).all() and len(gaps[0]) == 5
    short = clean(c['dirty'], c['freq'], c['tau'], c['w'], False, 2, c['mask'], 5, 0.5, threshold=float(stats['peak'].max()) * 1.0001, dtype=dtype)
    assert (short[2]['reason'] == 1).all() and (short[2]['ncomp'] <= 5).all() and (short[2]['ncomp'] > 0).all()
    for g in range(2):
        n = short[2]['ncomp'][g]
        assert short[1][g, :n].tobytes() == comps[g, :n].tobytes() and (short[1]['pixel'][g, n:] == -1).all() and not short[1]['C'][g, n:].any()


def test_restatement_ties_non_finite_pixels_and_the_empty_window():
    """Two equal peaks: the lower pixel wins.  A NaN or Inf pixel never wins and stays as it is.  No window, or nothing finite in it:
    reason 2, ncomp 0, peak 0, the residual the input."""
    c = case(22, 49, 2, 2, False)
    d = np.zeros((1, 4, 49), np.float32)
    d[0, :2, 30] = d[0, :2, 12] = 2.0
    d[0, 0, 20] = np.inf
    d[0, 1, 21] = np.nan
    mask = np.ones(49, np.uint8)
    R, comps, stats, _ = clean(d, c['freq'], c['tau'], c['w'], False, 2, mask, 1, 0.5)
    assert comps['pixel'][0, 0] == 12 and comps['I'][0, 0] == 4.0 and np.isinf(R[0, 0, 20]) and np.isnan(R[0, 1, 21])
    for m, img in ((np.zeros(49, np.uint8), c['dirty'][:1]), (mask, np.full((1, 4, 49), np.nan, np.float32))):
        R, comps, stats, _ = clean(img, c['freq'], c['tau'], c['w'], False, 2, m, 3, 0.5, dtype=np.float32)
        assert R.tobytes() == img.tobytes() and stats[0].tolist()[:3] == (0, 2, 0.0) and (comps['pixel'] == -1).all()


# ---------------------------------------------------------------- the host functions
def test_clean_components_takes_a_span_apart_without_a_copy():
    rng = np.random.default_rng(3)
    res = rng.standard_normal((NGROUP, 4, NPIX)).astype(np.float32)
    comps = np.zeros((NGROUP, NITER), CLEAN_COMPONENT)
    comps['pixel'], comps['I'], comps['C'] = rng.integers(-1, NPIX, (NGROUP, NITER)), 1.5, rng.standard_normal((NGROUP, NITER, 4))
    stats = np.zeros(NGROUP, CLEAN_STATS)
    stats['ncomp'], stats['reason'], stats['peak'] = (3, 1), (0, 1), (0.25, 0.5)
    span = np.concatenate([pack_span(res, comps, stats), np.zeros(7, np.uint8)])
    assert CLEAN_COMPONENT.itemsize == 32 and CLEAN_STATS.itemsize == 16
    assert clean_layout(NGROUP, NITER, NPIX) == (16 * NGROUP * NPIX, 16 * NGROUP * NPIX + 32 * NGROUP * NITER, span.size - 7)
    c, s, r = clean_components(span, NGROUP, NITER, NPIX)
    assert c.tobytes() == comps.tobytes() and s.tobytes() == stats.tobytes() and r.tobytes() == res.tobytes()
    assert np.shares_memory(r, span) and np.shares_memory(c, span)
    with pytest.raises(ValueError):
        clean_components(span[:-8], NGROUP, NITER, NPIX)


def test_restore_adds_a_gaussian_of_the_given_width_per_component():
    """Pixel 0 at the zenith, pixels 1..3 at 1, 2 and 90 degrees from it; one component of (2, 1, 0.5, -0.25) at pixel 0 and a beam of 2
    degrees: the component itself at pixel 0, half of it at one degree (half the width away), 1/16 at two, nothing at the horizon; an
    unfilled record adds nothing; the second group, without components, is its residual."""
    ang = np.radians([0.0, 1.0, 2.0, 90.0])
    lmn = np.stack([np.sin(ang), np.zeros(4), np.cos(ang)], axis=-1)
    res = np.arange(2 * 4 * 4, dtype=np.float32).reshape(2, 4, 4)
    comps = np.zeros((2, 2), CLEAN_COMPONENT)
    comps['pixel'] = -1
    comps[0, 0] = (0, 3.0, (2, 1, 0.5, -0.25), 0)
    out = restore(res, comps, lmn, np.radians(2.0))
    C = np.array([2, 1, 0.5, -0.25])
    assert out.dtype == np.float64 and np.array_equal(out[1], res[1])
    assert np.allclose(out[0] - res[0], C[:, None] * np.array([1, 0.5, 1 / 16.0, 0])[None], rtol=1e-12, atol=1e-300)
    both = comps.copy()
    both[0, 1] = (2, 1.0, (1, 1, 0, 0), 0)
    assert np.allclose(restore(res, both, lmn, np.radians(2.0))[0, 0] - out[0, 0], [1 / 16.0, 0.5, 1, 0], rtol=1e-12, atol=1e-300)
    for bad in (dict(fwhm_rad=0.0), dict(fwhm_rad=np.nan), dict(lmn=lmn[:3])):
        with pytest.raises(ValueError):
            restore(res, comps, **dict(dict(lmn=lmn, fwhm_rad=0.1), **bad))


def test_components_to_model_merges_ranks_and_repeats():
    lmn = sky(np.random.default_rng(5), 6)
    comps = np.zeros((2, 4), CLEAN_COMPONENT)
    comps['pixel'] = -1
    comps[0, 0], comps[0, 1], comps[0, 2] = (4, 0, (2, 1, 9, 9), 0), (1, 0, (0.5, 0.5, 0, 0), 0), (4, 0, (1, 1, 0, 0), 0)
    comps[1, 0], comps[1, 1] = (1, 0, (0.25, 0.25, 0, 0), 0), (2, 0, (-1, -2, 0, 0), 0)
    src, flux = components_to_model(comps, lmn, 3)
    assert src.dtype == np.float64 and flux.dtype == np.float32 and flux.flags['C_CONTIGUOUS'] and src.flags['C_CONTIGUOUS']
    assert np.array_equal(src, lmn[[4, 2, 1]])                  # summed |flux|: 2.5, 1.5, 0.75
    assert np.array_equal(flux, np.repeat(np.array([[2.5, 0, 0.5], [0, 0, 0.25]], np.float32), 3, axis=0))      # (a negative flux is 0)
    src, flux = components_to_model(comps, lmn, 1, nsrc_max=2)
    assert np.array_equal(src, lmn[[4, 2]]) and flux.shape == (2, 2)
    src, flux = components_to_model(comps[:, 3:], lmn, 2)
    assert src.shape == (0, 3) and flux.shape == (4, 0)
    for bad in (dict(nfavg=0), dict(nsrc_max=0)):
        with pytest.raises(ValueError):
            components_to_model(comps, lmn, **dict(dict(nfavg=1), **bad))


@pytest.mark.parametrize("autos", [False, True])
def test_model_round_trip_through_calapply_removes_what_clean_found(autos):
    """Sources of 3 and 1.5 without noise (XX = YY, so the model's (C_XX + C_YY) / 2 is both), gain 0.5, 8 iterations: the components'
    model handed to tests/calapply_ref.apply with unit factors takes the sources out of the visibilities, and their image is the
    restatement's residual in XX and YY -- so the peak of I drops by the factor the restatement reports (0.1 at the most here).  The
    bar: the float32 roundings between the two routes -- the dirty image (2^-24 max|dirty|), the records' C and the model's flux
    (2^-24 sum|C| each) -- so 4 * 2^-24 of max|dirty| + sum|C| per word."""
    nstand, npix, nfine, nfavg, niter = 22, 49, 4, 2, 8
    c = case(nstand, npix, nfine, nfavg, autos, noise=0.0)
    R, comps, stats, _ = clean(c['dirty'], c['freq'], c['tau'], c['w'], autos, nfavg, c['mask'], niter, 0.5)
    assert set(comps['pixel'].reshape(-1)) == set(c['src'])
    src_lmn, flux = components_to_model(comps, c['lmn'], nfavg)
    assert src_lmn.shape == (2, 3) and flux.shape == (nfine, 2) and np.array_equal(src_lmn[0], c['lmn'][c['src'][0]])
    V2 = calapply_ref.apply(c['V'], np.ones((nfine, 2, nstand), np.complex64), c['freq'], steering_delays(c['pos'], src_lmn), flux)
    again = image(V2, c['freq'], c['tau'], c['w'], autos, nfavg)
    sc = clean_ref.scale(c['dirty'], comps)
    assert (np.abs(again[:, :2] - R[:, :2]) <= 4 * 2.0 ** -24 * sc[:, :2]).all()
    before, after = np.abs(stokes_i(c['dirty'])[:, c['mask'] != 0]).max(axis=1), np.abs(stokes_i(again)[:, c['mask'] != 0]).max(axis=1)
    assert (np.abs(after - stats['peak']) <= 4 * 2.0 ** -24 * (sc[:, 0, 0] + sc[:, 1, 0])).all() and (after < 0.1 * before).all()


# ---------------------------------------------------------------- the block on CPU rings
def image_header(nstand=NSTAND, nfine=NFINE, seq0=0, fine_sfreq=50e6, **extra):
    """The sequence header UpchanImage writes (upchan_image_block.py output_header)."""
    hdr = source_header(nfine // 2, nstand, 2, seq0=seq0, sfreq=fine_sfreq + FINE_BW)
    hdr.update(nupchan=2, fine_lo=0, nfine=nfine, fine_bw_hz=FINE_BW, fine_sfreq=fine_sfreq, nframe_per_integration=ACC_LEN // 2, acc_len=ACC_LEN,
               npix=NPIX, nfavg=NFAVG, nprod=4, autos=False, nbit=32, complex=False, image_sfreq=fine_sfreq + FINE_BW / 2, image_bw_hz=2 * FINE_BW)
    hdr.update(extra)
    return hdr


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _geometry(seed=11):
    rng = np.random.default_rng(seed)
    return random_array(rng, NSTAND), sky(rng, NPIX)


def _block(iring, oring, be, **kw):
    pos, lmn = _geometry()
    args = dict(positions=pos, lmn=lmn, niter=NITER, gain=0.5)
    args.update(kw)
    return UpchanClean(LOG, iring, oring, backend=be, **args)


def _images(rng, n):
    d = rng.standard_normal((n, NGROUP, 4, NPIX)).astype(np.float32)
    d[:, :, :2] += 3
    return d


def _expect(dirty, freq, w=None, autos=False, mask=None, niter=NITER, gain=0.5, threshold=0.0, fraction=0.0):
    tau = steering_delays(*_geometry())
    R, comps, stats, _ = clean(dirty, freq, tau, np.ones(NSTAND, np.float32) if w is None else w, autos, NFAVG, mask, niter, gain, threshold, fraction, np.float32)
    return pack_span(R, comps, stats)


SPAN = clean_layout(NGROUP, NITER, NPIX)[2]
IMG = NGROUP * 4 * NPIX * 4


def test_block_one_span_per_span_and_header(ring_impl):
    """Source -> UpchanClean -> Sink, two sequences of three images (the second with autos): every output span is the float32
    restatement of its input span with the sequence's own frequencies and autos; the header is the input's plus cleaned, niter, gain,
    threshold, fraction, comp_offset, stats_offset; the geometry and the weights are set once per sequence."""
    rng = np.random.default_rng(13)
    imgs = [_images(rng, 3) for _ in range(2)]
    hdrs = [image_header(seq0=1000, fine_sfreq=50e6), image_header(seq0=5000, fine_sfreq=62e6, autos=True)]
    r0, r1 = Ring("image-output"), Ring("clean-output")
    be = CleanBackend()
    cb = _block(r0, r1, be, threshold=0.125, fraction=0.25)
    sink = Sink(r1, SPAN)
    run_blocks([cb], Source(r0, [(hdrs[s], imgs[s].reshape(-1).view(np.uint8), IMG) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    co, so, n = clean_layout(NGROUP, NITER, NPIX)
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        freq = hdrs[s]['fine_sfreq'] + FINE_BW * np.arange(NFINE)
        assert len(spans) == 3
        for k in range(3):
            assert spans[k].tobytes() == _expect(imgs[s][k], freq, autos=bool(s), threshold=0.125, fraction=0.25).tobytes()
        assert tag == hd['seq0'] == hdrs[s]['seq0']
        assert (hd['cleaned'], hd['niter'], hd['gain'], hd['threshold'], hd['fraction'], hd['comp_offset'], hd['stats_offset'], hd['span_bytes']) == \
            (True, NITER, 0.5, 0.125, 0.25, co, so, n)
        assert all(hd[k] == hdrs[s][k] for k in hdrs[s] if k != 'seq0')
    assert be.calls == ['init', 'window', ('control', NITER, 0.5, 0.125, 0.25), 'weights', 'geometry', 'run', 'run', 'run', 'weights', 'geometry', 'run', 'run', 'run']
    assert cb.stats['nclean'] == 6 and cb.stats['ngap'] == 0


def test_block_cleans_a_cleaned_span_deeper(ring_impl):
    """UpchanClean -> UpchanClean: the second reads the first's spans (its header carries `cleaned`), takes the residual at their front
    and writes niter = 2 more: residual and records of the float32 restatement run on the first one's residual."""
    rng = np.random.default_rng(15)
    imgs = _images(rng, 2)
    hdr = image_header(seq0=960)
    r0, r1, r2 = Ring("image-output"), Ring("clean-output"), Ring("deeper-output")
    be1, be2 = CleanBackend(), CleanBackend()
    a, b = _block(r0, r1, be1), _block(r1, r2, be2, niter=2)
    n2 = clean_layout(NGROUP, 2, NPIX)[2]
    sink = Sink(r2, n2)
    run_blocks([a, b], Source(r0, [(hdr, imgs.reshape(-1).view(np.uint8), IMG)]), [sink])
    (hd, tag, spans), = sink.sequences
    freq = hdr['fine_sfreq'] + FINE_BW * np.arange(NFINE)
    assert len(spans) == 2 and hd['niter'] == 2 and hd['stats_offset'] == clean_layout(NGROUP, 2, NPIX)[1]
    for k in range(2):
        first = clean_components(_expect(imgs[k], freq), NGROUP, NITER, NPIX)[2]
        assert spans[k].tobytes() == _expect(first, freq, niter=2).tobytes()


def test_block_changes_take_effect_at_the_next_integration_and_a_gap_restarts_the_sequence(ring_impl):
    """Images 0..6 of a sequence, 3 never read.  set_weights and set_window before image 1, a `niter` and `gain` command before image 2, a
    `weights` and `threshold` command before image 5, set_control(fraction) before image 6.  Each span carries what was set before it; a
    change of the control starts a new output sequence whose header says so, as the gap does; spans keep the size of the constructor's
    niter.  What the contract refuses is refused and changes nothing."""
    rng = np.random.default_rng(17)
    imgs = _images(rng, 7)
    hdr = image_header(seq0=960)
    w1, w2 = np.array([2, 0, 1, 1, 3], np.float32), [1.0, 1.0, 0.0, 2.0, 0.5]
    m1 = np.arange(NPIX) % 2 == 0
    box = {}

    def spans():
        for k in (0, 1, 2, 4, 5, 6):
            cb = box['cb']
            if k == 1:
                cb.set_weights(w1)
                cb.set_window(m1)
                for bad in ([1.0] * 4, [1, 1, 1, 1, -1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, np.nan]):
                    with pytest.raises(ValueError, match="UPCHAN_CLEAN"):
                        cb.set_weights(bad)
                for bad in (np.ones(NPIX - 1, bool), np.ones(NPIX), "all"):
                    with pytest.raises(ValueError, match="UPCHAN_CLEAN"):
                        cb.set_window(bad)
                for bad in (dict(niter=NITER + 1), dict(niter=-1), dict(gain=0.0), dict(gain=1.5), dict(threshold=-1.0), dict(fraction=np.inf), dict(niter=1.5)):
                    with pytest.raises(ValueError, match="UPCHAN_CLEAN"):
                        cb.set_control(**bad)
            if k == 2:
                cb.process_command_strings(_cmd(niter=2, gain=1))
                assert cb.last_response['val']['status'] == 'normal'
                for n, bad in enumerate(({'niter': NITER + 1}, {'niter': 1.0}, {'gain': 0}, {'gain': 2.0}, {'threshold': -0.5}, {'weights': [1.0]}, {'weights': [0.0] * 5},
                                         {'fraction': 0.5})):
                    cb.process_command_strings(_cmd(str(2 + n), **bad))
                    assert cb.last_response['val']['status'] == 'error', bad
            if k == 5:
                cb.process_command_strings(_cmd("20", weights=w2, threshold=0.5))
                assert cb.last_response['val']['status'] == 'normal'
            if k == 6:
                cb.set_control(fraction=0.75)
            yield k, imgs[k]

    be = CleanBackend()
    r1 = Ring("clean-output")
    cb = box['cb'] = _block(_FakeRing([_FakeSeq(hdr, spans(), IMG)]), r1, be)
    sink = Sink(r1, SPAN)
    sink.start()
    cb.main()
    sink.join(20)
    seqs = sink.sequences
    assert [(h['seq0'], t, len(s)) for h, t, s in seqs] == [(960 + k * ACC_LEN, 960 + k * ACC_LEN, n) for k, n in ((0, 2), (2, 1), (4, 1), (5, 1), (6, 1))]
    assert [(h['niter'], h['gain'], h['threshold'], h['fraction']) for h, _, _ in seqs] == [(NITER, 0.5, 0, 0), (2, 1, 0, 0), (2, 1, 0, 0), (2, 1, 0.5, 0), (2, 1, 0.5, 0.75)]
    assert [h['stats_offset'] for h, _, _ in seqs] == [clean_layout(NGROUP, n, NPIX)[1] for n in (NITER, 2, 2, 2, 2)]
    freq = hdr['fine_sfreq'] + FINE_BW * np.arange(NFINE)
    got = [s for _, _, ss in seqs for s in ss]
    ones = np.ones(NSTAND, np.float32)
    setups = [(0, ones, None, NITER, 0.5, 0, 0), (1, w1, m1, NITER, 0.5, 0, 0), (2, w1, m1, 2, 1, 0, 0), (4, w1, m1, 2, 1, 0, 0), (5, w2, m1, 2, 1, 0.5, 0),
              (6, w2, m1, 2, 1, 0.5, 0.75)]
    for span, (k, w, m, niter, gain, th, fr) in zip(got, setups):
        exp = _expect(imgs[k], freq, w=np.asarray(w, np.float32), mask=m, niter=niter, gain=gain, threshold=th, fraction=fr)
        assert span.size == SPAN and span[:exp.size].tobytes() == exp.tobytes(), k
    assert be.calls == ['init', 'window', ('control', NITER, 0.5, 0.0, 0.0), 'weights', 'geometry', 'run', 'weights', 'window', 'run', ('control', 2, 1.0, 0.0, 0.0),
                        'run', 'run', 'weights', ('control', 2, 1.0, 0.5, 0.0), 'run', ('control', 2, 1.0, 0.5, 0.75), 'run']
    assert cb.stats['ngap'] == 1 and cb.stats['nclean'] == 6


@pytest.mark.parametrize("kw", [dict(niter=0), dict(niter=4097), dict(niter=1.5), dict(gain=0), dict(gain=1.01), dict(threshold=-1), dict(fraction=np.nan),
                                dict(weights=[1.0] * 4), dict(weights=[1, 1, 1, 1, -1.0]), dict(weights=[1, 0, 0, 0, 0.0]), dict(window=[1, 0]),
                                dict(window=np.ones(NPIX)), dict(lmn=[[0, 0]]), dict(positions=np.zeros((5, 2))), dict(lmn=[[0, 0, np.inf]])])
def test_constructor_refuses_bad_arguments(kw):
    be = CleanBackend()
    with pytest.raises(ValueError, match="UPCHAN_CLEAN"):
        _block(Ring("a"), Ring("b"), be, **kw)
    assert be.cl is None


@pytest.mark.parametrize("bad", [dict(npix=8), dict(npix=None), dict(nprod=3), dict(nstand=6), dict(nfine=None), dict(nfavg=3), dict(nfavg=None), dict(nbit=8),
                                 dict(complex=True), dict(autos=None), dict(fine_sfreq=None), dict(fine_bw_hz=0.0), dict(acc_len=0),
                                 dict(cleaned=True, stats_offset=8)])
def test_block_refuses_what_is_not_an_image_of_its_list(bad):
    """A pixel count that differs from the list's, fewer than four words, another stand count, an nfavg that does not divide nfine, and
    headers that are not UpchanImage's: refused at the sequence, before anything is run."""
    be = CleanBackend()
    hdr = image_header()
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NGROUP, 4, NPIX), np.float32)
    cb = _block(_FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), be)
    with pytest.raises(ValueError, match="UPCHAN_CLEAN"):
        cb.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengCleanInitialize", "xengCleanGetInfo", "xengCleanSetGeometry", "xengCleanSetWeights", "xengCleanSetWindow", "xengCleanSetControl", "xengCleanRun",
         "xengCleanCheckGuards", "xengCleanMark", "xengCleanWait", "xengCleanTicketDone", "xengCleanSync", "xengCleanDestroy")


def test_backend_forwards_every_call_the_block_makes():
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("clean_initialize", "clean_set_geometry", "clean_set_weights", "clean_set_window", "clean_set_control", "clean_run", "clean_info",
              "clean_guards_intact", "clean_mark", "clean_wait", "clean_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("clean_initialize", "clean_set_geometry", "clean_set_weights", "clean_set_window", "clean_set_control", "clean_run", "clean_mark", "clean_wait",
              "clean_sync"):
        assert callable(getattr(CleanBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Mark and TicketDone are enqueue-only, the calls that wait are not.  Initialize
    refuses every size outside the contract before it touches a device; Run refuses null and misaligned pointers, the getters null
    results, SetGeometry and SetWeights null tables, SetControl a gain, threshold or fraction outside the contract, before looking
    for a context; without one, INVALID_STATE."""
    lib = ffi.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in ffi.SYMBOLS, name
    for name in ("xengCleanRun", "xengCleanMark", "xengCleanTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengCleanInitialize", "xengCleanSetGeometry", "xengCleanSetWeights", "xengCleanSetWindow", "xengCleanSetControl", "xengCleanWait", "xengCleanSync",
                 "xengCleanCheckGuards", "xengCleanGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, nstand, nfine, nfavg, npix, niter_max)
    good = (0, 352, 192, 8, 4096, 100)
    for i, v in ((1, 0), (1, -3), (1, 2049), (2, 0), (3, 0), (3, 5), (3, 384), (4, 0), (4, (1 << 24) + 1), (4, 1 << 20), (5, 0), (5, -1), (5, 4097)):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCleanInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengCleanInitialize", 0, 4, 70000, 1, 16, 1)                      # (more channel groups than a launch takes)
    assert ei.value.status == INVALID_ARGUMENT
    s, d, ll = ctypes.c_int(), ctypes.c_double(), ctypes.c_longlong()
    f64 = np.zeros(4, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f32 = np.ones(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    info = [ctypes.byref(s), ctypes.byref(s), ctypes.byref(ll), ctypes.byref(ll), ctypes.byref(ll), ctypes.byref(d)]
    cases = [("xengCleanRun", (None, 4096)), ("xengCleanRun", (4096, None)), ("xengCleanRun", (4104, 4096)), ("xengCleanRun", (4096, 4104)),
             ("xengCleanSetGeometry", (None, f64)), ("xengCleanSetGeometry", (f64, None)), ("xengCleanSetWeights", (None, 0)),
             ("xengCleanSetControl", (1, 0.0, 0.0, 0.0)), ("xengCleanSetControl", (1, 1.5, 0.0, 0.0)), ("xengCleanSetControl", (1, np.nan, 0.0, 0.0)),
             ("xengCleanSetControl", (1, 0.5, -1.0, 0.0)), ("xengCleanSetControl", (1, 0.5, np.inf, 0.0)), ("xengCleanSetControl", (1, 0.5, 0.0, -1.0)),
             ("xengCleanSetControl", (1, 0.5, 0.0, np.nan)),
             ("xengCleanMark", (None,)), ("xengCleanTicketDone", (1, None)), ("xengCleanCheckGuards", (None,))]
    for i in range(6):
        cases.append(("xengCleanGetInfo", tuple(None if j == i else a for j, a in enumerate(info))))
    for name, args in cases:
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_clean_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengCleanRun", (4096, 4096)), ("xengCleanSetGeometry", (f64, f64)), ("xengCleanSetWeights", (f32, 1)), ("xengCleanSetWindow", (None,)),
                       ("xengCleanSetControl", (1, 0.5, 0.0, 0.0)), ("xengCleanGetInfo", tuple(info)),
                       ("xengCleanMark", (ctypes.byref(t),)), ("xengCleanWait", (1,)), ("xengCleanTicketDone", (1, ctypes.byref(s))),
                       ("xengCleanSync", ()), ("xengCleanCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCleanDestroy")        # (nothing to destroy: success)
