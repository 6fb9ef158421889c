"""UpchanImage without a GPU: the delays and grids of blocks/imaging.py (an east-west baseline's analytic fringe, the zenith, the
horizon mask, patches), the restatement (tests/image_ref.py) on a point source, on the autos, on a flagged stand that holds NaN; the
block on CPU rings (both implementations) with a backend that serves image_* from the restatement -- header keys, one output span
per input span, set_weights and a `weights` command at the next integration, a gap, the refusals -- and the C entry points'
argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanImage, image_norm, patch, pixel_grid, steering_delays, stokes_i
from caltech_bifrost_dsp_amd.blocks.imaging import C_M_S, direction_list
from caltech_bifrost_dsp_amd.ring import Ring
from tests.image_ref import ImageBackend, hermitian_uneven, image, masked, point_source, random_array, steering
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
NSTAND, NFINE, NFAVG, ACC_LEN = 5, 4, 2, 96
FINE_BW = 23925.78125 / 2


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def vis_header(nstand=NSTAND, nfine=NFINE, seq0=0, fine_sfreq=50e6, **extra):
    """The sequence header UpchanCorr writes (upchan_corr_block.py output_header)."""
    hdr = source_header(nfine // 2, nstand, 2, seq0=seq0, sfreq=fine_sfreq + FINE_BW)
    hdr.update(nupchan=2, fine_lo=0, nfine=nfine, fine_bw_hz=FINE_BW, fine_sfreq=fine_sfreq, nframe_per_integration=ACC_LEN // 2, acc_len=ACC_LEN,
               complex=True, nbit=32)
    hdr.update(extra)
    return hdr


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _sky(rng, n):
    """n directions above the horizon, the first the zenith: float64 [n][3]"""
    lm = rng.uniform(-0.6, 0.6, (n, 2))
    lm[0] = 0
    return np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)


# ---------------------------------------------------------------- delays and grids
def test_east_west_baseline_gives_the_analytic_fringe_and_the_zenith_no_delay():
    """Two stands d = 30 m apart east-west, coplanar, a unit source at the zenith (V = 1 everywhere), no autos: the image along
    the l axis is cos(2 pi f d l / c) in both polarisations; tau is 0 at the zenith for any array, and the w-term (n - 1) z / c
    away from it."""
    d, f = 30.0, 60e6
    pos = np.array([[-d / 2, 0, 0], [d / 2, 0, 0]])
    l = np.linspace(-0.9, 0.9, 37)
    lmn = np.stack([l, 0 * l, np.sqrt(1 - l * l)], axis=-1)
    tau = steering_delays(pos, lmn)
    assert tau.shape == (37, 2) and tau.dtype == np.float64 and tau.flags['C_CONTIGUOUS']
    assert np.allclose(tau[:, 1] - tau[:, 0], d * l / C_M_S, rtol=0, atol=1e-22)
    V = np.ones((1, 2, 2, 2, 2), np.complex128)
    I = image(V, [f], tau, np.ones(2), False, 1)
    fringe = np.cos(2 * np.pi * f * d * l / C_M_S)
    assert np.max(np.abs(I[0, 0] - fringe)) < 1e-12 and np.max(np.abs(I[0, 1] - fringe)) < 1e-12 and np.max(np.abs(I[0, 3])) < 1e-12
    rng = np.random.default_rng(1)
    arr = random_array(rng, 7)
    t = steering_delays(arr, [[0, 0, 1], [0.3, -0.2, np.sqrt(1 - 0.13)]])
    assert (t[0] == 0).all()
    assert np.allclose(t[1], (0.3 * arr[:, 0] - 0.2 * arr[:, 1] + (np.sqrt(0.87) - 1) * arr[:, 2]) / C_M_S, rtol=0, atol=1e-22)
    for bad in (dict(positions_enu_m=arr[:, :2]), dict(lmn=[[0, 0]]), dict(lmn=[[0, 0, np.nan]]), dict(positions_enu_m=np.zeros((0, 3)))):
        kw = dict(positions_enu_m=arr, lmn=[[0, 0, 1]])
        kw.update(bad)
        with pytest.raises(ValueError, match="steering_delays"):
            steering_delays(**kw)


@pytest.mark.parametrize("side,fov", [(16, 180.0), (9, 180.0), (33, 120.0), (8, 20.0)])
def test_pixel_grid_masks_exactly_the_pixels_at_or_below_the_horizon(side, fov):
    l, m, n, mask = pixel_grid(side, fov)
    assert l.shape == m.shape == n.shape == mask.shape == (side, side) and l.dtype == np.float64
    assert np.array_equal(mask, l * l + m * m < 1.0) and np.array_equal(~mask, l * l + m * m >= 1.0)
    assert np.allclose(n[mask] ** 2 + l[mask] ** 2 + m[mask] ** 2, 1.0, rtol=0, atol=1e-15) and (n[~mask] == 0).all()
    half = np.sin(np.radians(fov) / 2)
    assert np.allclose(l[0], half * (2 * np.arange(side) + 1 - side) / side) and np.array_equal(l, m.T) and (np.diff(l[0]) > 0).all()
    assert mask.all() == (fov < 90) and (side % 2 == 0 or (l[side // 2, side // 2], m[side // 2, side // 2], n[side // 2, side // 2]) == (0, 0, 1))
    d = direction_list(l, m, n, mask)
    assert d.shape == (int(mask.sum()), 3) and np.array_equal(d[:, 0], l[mask])
    with pytest.raises(ValueError, match="pixel_grid"):
        pixel_grid(0)
    with pytest.raises(ValueError, match="pixel_grid"):
        pixel_grid(8, 200.0)


def test_patch_is_centred_on_its_direction_and_masked_alike():
    l, m, n, mask = patch(0.3, -0.4, 5, 0.01)
    assert (l[2, 2], m[2, 2]) == (0.3, -0.4) and np.allclose(np.diff(l[0]), 0.01) and np.allclose(np.diff(m[:, 0]), 0.01) and mask.all()
    assert np.allclose(n, np.sqrt(1 - l * l - m * m))
    l, m, n, mask = patch(0.99, 0.0, 4, 0.02)
    assert np.array_equal(mask, l * l + m * m < 1.0) and not mask.all() and mask.any()
    with pytest.raises(ValueError, match="patch"):
        patch(0.0, 0.0, 4, 0.0)


def test_image_norm_and_stokes_i():
    w = np.array([1.0, 2.0, 0.0, 0.5])
    assert image_norm(w, True, 1) == 1 / 3.5 ** 2 and image_norm(w, False, 4) == 1 / (4 * (3.5 ** 2 - 5.25))
    for bad in (dict(w=[0.0, 0.0]), dict(w=[1.0], autos=False), dict(w=[1.0, -1.0]), dict(w=[1.0, np.inf]), dict(nfavg=0), dict(w=[])):
        kw = dict(w=w, autos=False, nfavg=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="image_norm"):
            image_norm(**kw)
    assert image_norm([1.0], True, 1) == 1.0
    img = np.arange(2 * 4 * 3, dtype=np.float32).reshape(2, 4, 3)
    assert np.array_equal(stokes_i(img), img[:, 0] + img[:, 1])


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("autos", [False, True])
def test_point_source_images_to_one_at_its_pixel_and_no_more_elsewhere(autos):
    """V = a a^H of a unit source at list pixel 11, uneven weights (one of them 0), two channel groups: XX and YY read 1.0 at
    that pixel and at most 1 anywhere, XY the same (equal polarisations), within 1e-12 in float64."""
    rng = np.random.default_rng(3)
    nstand, x0 = 12, 11
    pos, lmn = random_array(rng, nstand), _sky(rng, 40)
    tau = steering_delays(pos, lmn)
    freq = 50e6 + FINE_BW * np.arange(4)
    w = rng.uniform(0.5, 2.0, nstand)
    w[4] = 0
    assert point_source(freq, tau[x0]).shape == (4, nstand, 2, nstand, 2)
    turns = freq[:, None] * tau[x0][None]
    a = np.repeat(np.exp(-2j * np.pi * turns), 2, axis=1)
    V = (a[:, :, None] * np.conj(a[:, None, :])).reshape(4, nstand, 2, nstand, 2)      # (float64, not the generator's complex64)
    I = image(V, freq, tau, w, autos, 2)
    assert I.shape == (2, 4, 40)
    assert np.max(np.abs(I[:, :3, x0] - 1.0)) < 1e-12 and np.max(np.abs(I[:, 3, x0])) < 1e-12
    assert (I[:, :3] <= 1.0 + 1e-12).all() and np.argmax(I[0, 0]) == x0 and np.max(np.abs(I[:, 0] - I[:, 1])) < 1e-12
    assert np.max(np.abs(stokes_i(I) - 2 * I[:, 0])) < 1e-12


def test_autos_off_removes_exactly_the_diagonal_blocks():
    """norm_with * I_with / ... : the un-normalised image with autos minus the one without is sum_s w_s^2 V[s p][s q] at every
    pixel (the steering factors cancel on the diagonal blocks): I_off = (I_on / norm_on - sum_c sum_s w_s^2 V[c][s p][s q]) * norm_off."""
    rng = np.random.default_rng(5)
    nstand = 9
    tau = steering_delays(random_array(rng, nstand), _sky(rng, 17))
    freq = 61e6 + FINE_BW * np.arange(4)
    w = rng.uniform(0.0, 2.0, nstand)
    V = hermitian_uneven(rng, 4, nstand).astype(np.complex128)
    on, off = image(V, freq, tau, w, True, 2), image(V, freq, tau, w, False, 2)
    D = np.einsum('s,cspsq->cpq', w * w, V).reshape(2, 2, 2, 2).sum(axis=1)              # per group
    diag = np.stack([D[:, 0, 0].real, D[:, 1, 1].real, D[:, 0, 1].real, D[:, 0, 1].imag], axis=1)[:, :, None]
    n_on, n_off = image_norm(w, True, 2), image_norm(w, False, 2)
    exp = (on / n_on - diag) * n_off
    assert np.max(np.abs(off - exp)) < 1e-12 * np.max(np.abs(exp)) and np.max(np.abs(diag)) > 0


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_flagged_stand_holding_nan_is_the_stand_deleted(dtype):
    """w_3 = 0 and NaN / Inf all over stand 3's rows and columns: the image is finite and equals, bit for bit, the image of the
    array without stand 3."""
    rng = np.random.default_rng(7)
    nstand = 8
    pos, lmn = random_array(rng, nstand), _sky(rng, 13)
    tau = steering_delays(pos, lmn)
    freq = 47e6 + FINE_BW * np.arange(2)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[3] = 0
    V = hermitian_uneven(rng, 2, nstand)
    bad = V.copy()
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    got = image(bad, freq, tau, w, False, 1, dtype)
    keep = np.arange(nstand) != 3
    exp = image(V[:, keep][:, :, :, keep], freq, tau[:, keep], w[keep], False, 1, dtype)
    assert np.isfinite(got).all() and np.array_equal(got, exp)
    assert np.isfinite(masked(bad, w, False)).all() and (steering(freq, tau, w)[:, :, 3] == 0).all()


# ---------------------------------------------------------------- the block on CPU rings
def _geometry(seed=11, nstand=NSTAND, npix=7):
    rng = np.random.default_rng(seed)
    return random_array(rng, nstand), _sky(rng, npix)


def _block(iring, oring, be, **kw):
    pos, lmn = _geometry()
    args = dict(positions=pos, lmn=lmn, nfavg=NFAVG)
    args.update(kw)
    return UpchanImage(LOG, iring, oring, backend=be, **args)


def _images(spans, npix=7, ngroup=NFINE // NFAVG):
    return np.array([s.view(np.float32).reshape(ngroup, 4, npix) for s in spans])


def test_block_one_span_per_integration_and_header(ring_impl):
    """Source -> UpchanImage -> Sink, two sequences of three integrations: every output span is the complex64 restatement of its
    input span with the sequence's own frequencies; the header is the input's plus npix, nfavg, nprod, autos, the group centres,
    nbit 32 and complex False; the geometry is set once per sequence."""
    rng = np.random.default_rng(13)
    pos, lmn = _geometry()
    tau = steering_delays(pos, lmn)
    Vs = [hermitian_uneven(rng, 3 * NFINE, NSTAND).reshape(3, NFINE, NSTAND, 2, NSTAND, 2) for _ in range(2)]
    hdrs = [vis_header(seq0=1000, fine_sfreq=50e6), vis_header(seq0=5000, fine_sfreq=62e6)]
    span = NFINE * (2 * NSTAND) ** 2 * 8
    r0, r1 = Ring("uc-output"), Ring("image-output")
    be = ImageBackend()
    im = _block(r0, r1, be)
    sink = Sink(r1, (NFINE // NFAVG) * 4 * 7 * 4)
    run_blocks([im], Source(r0, [(hdrs[s], Vs[s].reshape(-1).view(np.uint8), span) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        freq = hdrs[s]['fine_sfreq'] + FINE_BW * np.arange(NFINE)
        exp = np.array([image(Vs[s][k], freq, tau, np.ones(NSTAND), False, NFAVG, np.complex64) for k in range(3)], np.float32)
        assert len(spans) == 3 and _images(spans).tobytes() == exp.tobytes()
        assert tag == hd['seq0'] == hdrs[s]['seq0']
        assert (hd['npix'], hd['nfavg'], hd['nprod'], hd['autos'], hd['nbit'], hd['complex']) == (7, NFAVG, 4, False, 32, False)
        assert hd['image_sfreq'] == hdrs[s]['fine_sfreq'] + FINE_BW / 2 and hd['image_bw_hz'] == 2 * FINE_BW
        assert all(hd[k] == hdrs[s][k] for k in ('nfine', 'fine_sfreq', 'fine_bw_hz', 'nstand', 'npol', 'acc_len', 'nupchan'))
    assert be.calls == ['init', 'weights', 'geometry', 'run', 'run', 'run', 'geometry', 'run', 'run', 'run']
    assert im.stats['nimage'] == 6 and im.stats['ngap'] == 0


def test_block_weights_take_effect_at_the_next_integration_and_a_gap_restarts_the_sequence(ring_impl):
    """Integrations 0..5 of a sequence, 3 never read.  set_weights before integration 1 and a `weights` command before integration
    4 (flagging stand 2, whose visibilities are NaN from then on): integration 0 carries the constructor's weights, 1 and 2 the
    first change, 4 and 5 the second and are finite.  The gap ends the output sequence; the next one's seq0 is integration 4's.
    What is not nstand finite numbers >= 0 with a pair left is refused and changes nothing."""
    rng = np.random.default_rng(17)
    pos, lmn = _geometry()
    tau = steering_delays(pos, lmn)
    V = hermitian_uneven(rng, 6 * NFINE, NSTAND).reshape(6, NFINE, NSTAND, 2, NSTAND, 2)
    V[4:, :, 2] = np.nan
    V[4:, :, :, :, 2] = np.nan
    hdr = vis_header(seq0=960)
    w0 = np.array([1, 2, 1, 0.5, 1], np.float32)
    w1 = np.array([2, 0, 1, 1, 3], np.float32)
    w2 = [1.0, 1.0, 0.0, 2.0, 0.5]
    box = {}

    def spans():
        for k in (0, 1, 2, 4, 5):
            if k == 1:
                box['im'].set_weights(w1)
                for bad in ([1.0] * 4, [1, 1, 1, 1, -1], [0, 0, 0, 0, 0], [1, 1, 1, 1, np.nan]):
                    with pytest.raises(ValueError, match="UPCHAN_IMAGE"):
                        box['im'].set_weights(bad)
            if k == 4:
                box['im'].process_command_strings(_cmd(weights=w2))
                assert box['im'].last_response['val']['status'] == 'normal'
                for n, bad in enumerate(({'weights': [1.0]}, {'weights': [0.0] * 5}, {'weights': "none"}, {'weights': [1, 1, 1, 1, -2.0]})):
                    box['im'].process_command_strings(_cmd(str(2 + n), **bad))
                    assert box['im'].last_response['val']['status'] == 'error', bad
            yield k, V[k]

    be = ImageBackend()
    r1 = Ring("image-output")
    im = box['im'] = _block(_FakeRing([_FakeSeq(hdr, spans(), NFINE * (2 * NSTAND) ** 2 * 8)]), r1, be, weights=w0, autos=True)
    sink = Sink(r1, (NFINE // NFAVG) * 4 * 7 * 4)
    sink.start()
    im.main()
    sink.join(20)
    (h0, t0, a), (h1, t1, b) = sink.sequences
    assert (h0['seq0'], t0, h1['seq0'], t1) == (960, 960, 960 + 4 * ACC_LEN, 960 + 4 * ACC_LEN) and h0['autos'] is True
    freq = hdr['fine_sfreq'] + FINE_BW * np.arange(NFINE)
    exp = [image(V[k], freq, tau, w, True, NFAVG, np.complex64).astype(np.float32) for k, w in ((0, w0), (1, w1), (2, w1), (4, w2), (5, w2))]
    assert len(a) == 3 and len(b) == 2 and np.concatenate([_images(a), _images(b)]).tobytes() == np.array(exp).tobytes()
    assert np.isfinite(_images(b)).all()
    assert be.calls == ['init', 'weights', 'geometry', 'run', 'weights', 'run', 'run', 'weights', 'run', 'run']
    assert im.stats['ngap'] == 1 and im.stats['nimage'] == 5


@pytest.mark.parametrize("kw", [dict(nfavg=0), dict(nfavg=1.5), dict(weights=[1.0] * 4), dict(weights=[1, 1, 1, 1, -1.0]), dict(weights=[0.0] * 5),
                                dict(weights=[1, 0, 0, 0, 0.0]), dict(lmn=[[0, 0]]), dict(positions=np.zeros((5, 2))), dict(lmn=[[0, 0, np.inf]])])
def test_constructor_refuses_bad_arguments(kw):
    be = ImageBackend()
    with pytest.raises(ValueError, match="UPCHAN_IMAGE"):
        _block(Ring("a"), Ring("b"), be, **kw)
    assert be.im is None
    _block(Ring("a"), Ring("b"), be, weights=[1, 0, 0, 0, 0.0], autos=True)       # (one stand with its autos is an image)


@pytest.mark.parametrize("bad", [dict(npol=1), dict(nstand=6), dict(nfine=3), dict(nfine=None), dict(nbit=8), dict(complex=False), dict(fine_sfreq=None),
                                 dict(fine_bw_hz=0.0), dict(npix=7), dict(acc_len=0)])
def test_block_refuses_what_is_not_its_visibilities(bad):
    """npol != 2, a stand count that differs from the positions', an nfine that nfavg does not divide, and headers that are not
    UpchanCorr's: refused at the sequence, before anything is run."""
    be = ImageBackend()
    hdr = vis_header()
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NFINE, NSTAND, 2, NSTAND, 2), np.complex64)
    im = _block(_FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), be)
    with pytest.raises(ValueError, match="UPCHAN_IMAGE"):
        im.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengImageInitialize", "xengImageGetInfo", "xengImageSetGeometry", "xengImageSetWeights", "xengImageRun", "xengImageCheckGuards",
         "xengImageMark", "xengImageWait", "xengImageTicketDone", "xengImageSync", "xengImageDestroy")


def test_backend_forwards_every_call_the_block_makes():
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("image_initialize", "image_set_geometry", "image_set_weights", "image_run", "image_info", "image_guards_intact", "image_mark",
              "image_wait", "image_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("image_initialize", "image_set_geometry", "image_set_weights", "image_run", "image_mark", "image_wait", "image_sync"):
        assert callable(getattr(ImageBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Mark and TicketDone are enqueue-only, the calls that wait are not.  Initialize
    refuses every size outside the contract before it touches a device; Run refuses null and misaligned pointers, the getters null
    results, SetGeometry and SetWeights null tables, before looking for a context; without one, INVALID_STATE."""
    lib = ffi.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in ffi.SYMBOLS, name
    for name in ("xengImageRun", "xengImageMark", "xengImageTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengImageInitialize", "xengImageSetGeometry", "xengImageSetWeights", "xengImageWait", "xengImageSync", "xengImageCheckGuards", "xengImageGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, nstand, nfine, nfavg, npix)
    good = (0, 352, 192, 8, 4096)
    for i, v in ((1, 0), (1, -3), (1, 513), (2, 0), (3, 0), (3, 5), (3, 384), (4, 0), (4, (1 << 24) + 1), (4, 1 << 20)):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImageInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengImageInitialize", 0, 4, 70000, 1, 16)                         # (more channel groups than a launch takes)
    assert ei.value.status == INVALID_ARGUMENT
    s, d = ctypes.c_int(), ctypes.c_double()
    f64 = np.zeros(4, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f32 = np.ones(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name, args in (("xengImageRun", (None, 4096)), ("xengImageRun", (4096, None)), ("xengImageRun", (4104, 4096)), ("xengImageRun", (4096, 4104)),
                       ("xengImageGetInfo", (None, ctypes.byref(s), ctypes.byref(s), ctypes.byref(d))),
                       ("xengImageGetInfo", (ctypes.byref(s), None, ctypes.byref(s), ctypes.byref(d))),
                       ("xengImageGetInfo", (ctypes.byref(s), ctypes.byref(s), None, ctypes.byref(d))),
                       ("xengImageGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(s), None)),
                       ("xengImageSetGeometry", (None, f64)), ("xengImageSetGeometry", (f64, None)), ("xengImageSetWeights", (None, 0)),
                       ("xengImageMark", (None,)), ("xengImageTicketDone", (1, None)), ("xengImageCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_image_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengImageRun", (4096, 4096)), ("xengImageSetGeometry", (f64, f64)), ("xengImageSetWeights", (f32, 1)),
                       ("xengImageGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(s), ctypes.byref(d))),
                       ("xengImageMark", (ctypes.byref(t),)), ("xengImageWait", (1,)), ("xengImageTicketDone", (1, ctypes.byref(s))),
                       ("xengImageSync", ()), ("xengImageCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengImageDestroy")        # (nothing to destroy: success)
