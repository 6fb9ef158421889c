"""UpchanClean on the MI355X: xengClean* against the restatement (tests/clean_ref.py).  Parity with the float64 restatement on images
of point sources in noise; the point-spread function against xengImageRun's own response to a point source; exact bookkeeping (prefix,
gain times the residual, a Run split in two); bit identity of a sub-list of the pixels, of a fresh context and beside an X-engine
contraction and xengBeamformRun; the controls and the window; a NaN that stays in its channel group; the ABI with a context;
Source -> UpchanCorr -> UpchanImage -> UpchanClean on device rings.  The output sits between two poisoned 64 KiB guard bands that are
checked after every call, the state's guards at every close.  No wall-clock assertions.

The bar of the float tests is not a constant: it is five times the worst gap between the float32 and the float64 evaluation of the
restatement ON THE TEST'S OWN INPUTS, both taking the float64 run's component pixels (tests/clean_ref.py float_gap), per word as
|got - ref| / (max_x |dirty| + sum_k |C_k|) of the word's (group, word).  Every float test first asserts that the float64 run chose
each of its peaks by a margin of at least 100 float gaps (peak_margin) and that the kernel's pixel sequence is the float64 run's: a
near-tie fails loudly.  Measured here on the CPU with numpy 2.2 on the parity test's inputs: gaps of 9.7e-8 (22 stands, 37 pixels),
1.3e-7 (35 stands, 300 pixels) and 7.7e-8 (64 stands, 64 pixels), margins of 2.6e-3, 3.8e-4 and 5.2e-3.  Measured on the MI355X: see
MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import UpchanClean, UpchanCorr, UpchanImage, clean_components, clean_layout, image_norm, steering_delays  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import image_ref  # noqa: E402
from tests.clean_ref import case, clean, component_error, float_gap, peak_margin, scale, sky, word_error  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.image_ref import point_source, random_array  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
GAIN = 0.5
# worst word error / bar over test_parity_with_the_float64_restatement on the MI355X, per case (nstand, npix)
MEASURED = {(22, 37): 0.20, (35, 300): 0.20, (64, 64): 0.20}       # (worst errors 9.7e-8, 1.26e-7, 7.75e-8: the float32 restatement's own;
#                                                                    the PSF test's worst residual 1.2e-7 to 2.4e-7 against bars of 1.5e-6 to 2.1e-6)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _info():
    g, t, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    c, s, b = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengCleanGetInfo", ctypes.byref(g), ctypes.byref(t), ctypes.byref(c), ctypes.byref(s), ctypes.byref(b), ctypes.byref(n))
    return g.value, t.value, c.value, s.value, b.value, n.value


class CL:
    """The xengClean context (one per process), an input buffer and the output of one call between two poisoned guard bands."""

    def __init__(self, c, niter_max, tau=None, mask=None, geometry=True, gpu_state=True):
        tau = c['tau'] if tau is None else tau
        mask = c['mask'] if mask is None else mask
        self.npix, self.nstand = tau.shape
        self.nfine, self.nfavg, self.niter_max = len(c['freq']), c['nfavg'], niter_max
        self.ngroup = self.nfine // self.nfavg
        ffi.call("xengCleanInitialize", 0, self.nstand, self.nfine, self.nfavg, self.npix, niter_max)
        if geometry:
            ffi.call("xengCleanSetGeometry", _dp(np.ascontiguousarray(tau, np.float64)), _dp(np.ascontiguousarray(c['freq'], np.float64)))
        if gpu_state:
            ffi.call("xengCleanSetWeights", _fp(np.ascontiguousarray(c['w'], np.float32)), int(c['autos']))
            self.set_window(mask)
        self.din = ffi.DeviceBuffer(self.ngroup * 4 * self.npix * 4)
        self.nmax = clean_layout(self.ngroup, niter_max, self.npix)[2]
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nmax)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        self.niter = niter_max

    def set_window(self, mask):
        ffi.call("xengCleanSetWindow", None if mask is None else np.ascontiguousarray(mask, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def control(self, niter, gain=GAIN, threshold=0.0, fraction=0.0):
        ffi.call("xengCleanSetControl", niter, gain, threshold, fraction)
        self.niter = niter

    def upload(self, dirty):
        assert dirty.shape == (self.ngroup, 4, self.npix) and dirty.dtype == np.float32
        self.din.upload(np.ascontiguousarray(dirty))

    def enqueue(self):
        ffi.call("xengCleanRun", self.din.ptr, self.dout.ptr + GUARD)

    def result(self):
        """After a sync: (residual, components, stats) of the span (the poison is put back); every byte before it and past it must
        still be poison."""
        comp, stats, n = clean_layout(self.ngroup, self.niter, self.npix)
        assert _info()[2:5] == (comp, stats, n)
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + n:] == POISON).all(), "bytes past the output were written"
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        comps, st, res = clean_components(raw[GUARD:GUARD + n].copy(), self.ngroup, self.niter, self.npix)
        return res, comps, st

    def run(self, dirty, niter, gain=GAIN, threshold=0.0, fraction=0.0):
        self.control(niter, gain, threshold, fraction)
        self.upload(dirty)
        self.enqueue()
        ffi.call("xengCleanSync")
        return self.result()

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengCleanCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengCleanDestroy")
        self.din.free()
        self.dout.free()


def _reference(c, niter, gain=GAIN, **kw):
    """The float64 run of a case, its scale, its float gap; asserts the margin of its peaks."""
    ref, rcomps, rstats, gaps = clean(c['dirty'], c['freq'], c['tau'], c['w'], c['autos'], c['nfavg'], kw.pop('mask', c['mask']), niter, gain, **kw)
    sc = scale(c['dirty'], rcomps)
    gap = float_gap(c['dirty'], c['freq'], c['tau'], c['w'], c['autos'], c['nfavg'], ref, rcomps, rstats, gain)
    assert peak_margin(gaps, sc) >= 100 * gap, (peak_margin(gaps, sc), gap)
    return ref, rcomps, rstats, sc, gap


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. parity with float64
@pytest.mark.parametrize("nstand,npix,nfine,nfavg,autos,niter", [(22, 37, 4, 1, False, 6), (35, 300, 6, 3, True, 8), (64, 64, 2, 2, False, 4)])
def test_parity_with_the_float64_restatement(nstand, npix, nfine, nfavg, autos, niter):
    """One ragged tile; two tiles, the second ragged, an odd stand count and groups of three channels; an exact quarter of a tile.
    Sources of 3 and 1.5 in noise, gain 0.5; one stand of weight 0 and one of 0.5; every seventh pixel outside the window.  The
    components' pixels are the float64 run's; their values and every residual word within five float gaps of it."""
    c = case(nstand, npix, nfine, nfavg, autos)
    ref, rcomps, rstats, sc, gap = _reference(c, niter)
    cl = CL(c, niter)
    res, comps, stats = cl.run(c['dirty'], niter)
    assert abs(_info()[5] - image_norm(c['w'], autos, nfavg)) <= 1e-15 * image_norm(c['w'], autos, nfavg)
    cl.close()
    assert np.array_equal(comps['pixel'], rcomps['pixel']) and np.array_equal(stats['ncomp'], rstats['ncomp']) and np.array_equal(stats['reason'], rstats['reason'])
    err = max(word_error(res, ref, sc).max(), component_error(comps, rcomps, sc).max())
    print("clean parity %d stands %d pixels: float gap %.3g, worst error %.3g = %.2f of the bar" % (nstand, npix, gap, err, err / (5 * gap)))
    assert np.isfinite(res).all() and err <= 5 * gap, (err, 5 * gap)
    assert (comps['pad'] == 0).all() and (stats['pad'] == 0).all()
    I = res[:, 0] + res[:, 1]
    assert np.array_equal(stats['peak'], np.abs(np.where(c['mask'] != 0, I, 0)).max(axis=1))
    assert set(c['src']) >= set(comps['pixel'][:, :2].reshape(-1))       # (the first two components of every group: the sources)


# ---------------------------------------------------------------- 2. the PSF is the imager's own response
@pytest.mark.parametrize("autos,nfavg", [(False, 1), (True, 1), (False, 3), (True, 3)])
def test_psf_is_the_response_of_xeng_image_run_to_a_point_source(autos, nfavg):
    """xengImageRun on a unit point source at window pixel 41 of 70 (30 stands, the case's weights), its output handed on the device
    to xengCleanRun with gain 1 and niter 1: the component is (I, XX, YY, Re, Im) = (2, 1, 1, 1, 0) and every residual word is the
    float64 image minus the float64 component times the float64 PSF -- nothing, up to the source's own complex64 rounding -- within
    the image test's bar (five image float gaps, tests/image_ref.py) plus this test's."""
    nstand, npix, nfine, x0 = 30, 70, 6, 41
    c = case(nstand, npix, nfine, nfavg, autos, seed=77)
    assert c['mask'][x0]
    V = point_source(c['freq'], c['tau'][x0])
    img64 = image_ref.image(V, c['freq'], c['tau'], c['w'], autos, nfavg)
    igap = image_ref.float_gap(V, c['freq'], c['tau'], c['w'], autos, nfavg)
    isc = image_ref.scale(V, c['w'], autos, nfavg)
    c['dirty'] = img64.astype(np.float32)
    ref, rcomps, rstats, sc, gap = _reference(c, 1, gain=1.0)
    assert (rcomps['pixel'][:, 0] == x0).all()
    cl = CL(c, 1)
    ffi.call("xengImageInitialize", 0, nstand, nfine, nfavg, npix)
    ffi.call("xengImageSetGeometry", _dp(np.ascontiguousarray(c['tau'])), _dp(np.ascontiguousarray(c['freq'])))
    ffi.call("xengImageSetWeights", _fp(c['w']), int(autos))
    dvis = ffi.DeviceBuffer(V.nbytes).upload(V)
    ffi.call("xengImageRun", dvis.ptr, cl.din.ptr)
    cl.control(1, 1.0)
    cl.enqueue()                                    # (the same stream: the image is there)
    ffi.call("xengCleanSync")
    res, comps, stats = cl.result()
    cl.close()
    ffi.call("xengImageDestroy")
    dvis.free()
    bar = 5 * igap * isc + 5 * gap * sc
    assert (comps['pixel'][:, 0] == x0).all() and (stats['ncomp'] == 1).all() and (stats['reason'] == 0).all()
    exp = np.array([1, 1, 1, 0.0])
    assert (np.abs(comps['C'][:, 0].astype(np.float64) - exp) <= bar[:, :, 0]).all() and (np.abs(comps['I'][:, 0] - 2.0) <= bar[:, 0, 0] + bar[:, 1, 0]).all()
    print("PSF against the imager: worst residual %.3g, bar %.3g" % (np.abs(res).max(), bar.min()))
    assert (np.abs(res.astype(np.float64) - ref) <= bar).all() and np.abs(ref).max() < 1e-7


# ---------------------------------------------------------------- 3. exact bookkeeping
def test_prefix_gain_times_residual_and_a_run_split_in_two_bit_for_bit():
    """35 stands, 300 pixels, groups of three channels.  The records of niter = 4 are the first four of niter = 5; record 4's C_j is
    gain times the niter = 4 residual's word at that pixel, its I the sum of the first two; niter = 2 followed by a Run on its residual
    with niter = 3 gives the residual and the records of niter = 5."""
    c = case(35, 300, 6, 3, True)
    cl = CL(c, 5)
    r4, r5 = cl.run(c['dirty'], 4), cl.run(c['dirty'], 5)
    ra = cl.run(c['dirty'], 2)
    rb = cl.run(ra[0], 3)
    cl.close()
    assert r4[1].tobytes() == np.ascontiguousarray(r5[1][:, :4]).tobytes() and (r5[2]['ncomp'] == 5).all()
    for g in range(2):
        x = r5[1]['pixel'][g, 4]
        assert x >= 0 and np.array_equal(r5[1]['C'][g, 4], np.float32(GAIN) * r4[0][g, :, x]) and r5[1]['I'][g, 4] == r4[0][g, 0, x] + r4[0][g, 1, x]
        assert r4[2]['peak'][g] == abs(r5[1]['I'][g, 4])
    assert rb[0].tobytes() == r5[0].tobytes() and np.concatenate([ra[1], rb[1]], axis=1).tobytes() == r5[1].tobytes()
    assert rb[2]['peak'].tobytes() == r5[2]['peak'].tobytes()


# ---------------------------------------------------------------- 4. bit identity
def test_sub_list_fresh_context_and_other_kernels_change_no_bit():
    """35 stands, 300 pixels.  A sub-list in the same order that holds the whole window and about half of the other pixels, so that the
    tiles fall elsewhere: the same residual words and the same records (the pixels mapped).  The same Run in a fresh context, and in a
    fresh context while X-engine contractions run on their streams and xengBeamformRun on this one."""
    nstand, npix, nfine, nfavg, niter = 35, 300, 6, 3, 5
    c = case(nstand, npix, nfine, nfavg, False)
    mask = c['mask'].copy()
    mask[:120:3] = 0                                # (more pixels outside the window: the sub-list drops half of them)
    cl = CL(c, niter, mask=mask)
    full = cl.run(c['dirty'], niter)
    cl.close()
    assert not np.isnan(full[0]).any() and (full[2]['ncomp'] == niter).all()
    out = np.flatnonzero(mask == 0)
    keep = np.sort(np.concatenate([np.flatnonzero(mask), out[::2]]))
    assert len(keep) < npix - 20 and (keep[:100] != np.arange(100)).any()
    cl = CL(c, niter, tau=np.ascontiguousarray(c['tau'][keep]), mask=mask[keep])
    sub = cl.run(np.ascontiguousarray(c['dirty'][:, :, keep]), niter)
    cl.close()
    assert sub[0].tobytes() == np.ascontiguousarray(full[0][:, :, keep]).tobytes()
    assert np.array_equal(keep[sub[1]['pixel']], full[1]['pixel']) and sub[1]['C'].tobytes() == full[1]['C'].tobytes() and sub[1]['I'].tobytes() == full[1]['I'].tobytes()
    assert sub[2].tobytes() == full[2].tobytes()
    cl = CL(c, niter, mask=mask)
    again = cl.run(c['dirty'], niter)
    cl.close()
    assert _same(again, full)
    bstand, bchan, btime, nbeam = 96, 8, 96, 4
    rng = np.random.default_rng(3)
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, bstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * bstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    cl = CL(c, niter, mask=mask)
    cl.control(niter)
    cl.upload(c['dirty'])
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(3):
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            cl.enqueue()
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengCleanSync")
            got.append(cl.result())
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    cl.close()
    ffi.call("xengBeamformDestroy")
    assert all(_same(g, full) for g in got)


# ---------------------------------------------------------------- 5. the controls and the window
def test_niter_zero_threshold_fraction_window_and_an_empty_window():
    """niter = 0 and a threshold above the peak copy the input bit for bit with no component (reasons 0 and 1, the peak reported);
    `fraction` stops where the float64 restatement does (and where its float32 form does); with the brighter source's pixel outside
    the window that pixel is never a component but is subtracted from, within the bar; an empty window is reason 2 with peak +0."""
    nstand, npix, nfine, nfavg, niter = 35, 300, 6, 3, 8
    c = case(nstand, npix, nfine, nfavg, True)
    dirty = c['dirty']
    top = np.abs(np.where(c['mask'] != 0, dirty[:, 0] + dirty[:, 1], 0)).max(axis=1)
    cl = CL(c, niter)
    for kw, reason in ((dict(niter=0), 0), (dict(niter=niter, threshold=float(top.max()) * 1.5), 1)):
        res, comps, stats = cl.run(dirty, **kw)
        assert res.tobytes() == dirty.tobytes() and (stats['ncomp'] == 0).all() and (stats['reason'] == reason).all() and (comps['pixel'] == -1).all()
        assert np.array_equal(stats['peak'], top) and not comps['C'].view(np.uint32).any() and not comps['I'].view(np.uint32).any()
    # threshold exactly at the peak of group 0: <= stops it; just below lets it go on
    res, comps, stats = cl.run(dirty, niter, threshold=float(top[0]))
    assert stats['ncomp'][0] == 0 and stats['reason'][0] == 1
    fraction = 0.55
    ref, rcomps, rstats, sc, gap = _reference(c, niter, fraction=fraction)
    r32 = clean(dirty, c['freq'], c['tau'], c['w'], True, nfavg, c['mask'], niter, GAIN, fraction=fraction, dtype=np.float32)
    assert (rstats['reason'] == 1).all() and (0 < rstats['ncomp']).all() and (rstats['ncomp'] < niter).all() and np.array_equal(r32[2]['ncomp'], rstats['ncomp'])
    res, comps, stats = cl.run(dirty, niter, fraction=fraction)
    assert np.array_equal(stats['ncomp'], rstats['ncomp']) and np.array_equal(stats['reason'], rstats['reason']) and np.array_equal(comps['pixel'], rcomps['pixel'])
    assert max(word_error(res, ref, sc).max(), component_error(comps, rcomps, sc).max()) <= 5 * gap
    assert (np.abs(stats['peak'].astype(np.float64) - rstats['peak']) <= 5 * gap * (sc[:, 0, 0] + sc[:, 1, 0])).all()
    bright = int(c['src'][0])
    mask = c['mask'].copy()
    mask[bright] = 0
    ref, rcomps, rstats, sc, gap = _reference(c, 4, mask=mask)
    cl.set_window(mask)
    res, comps, stats = cl.run(dirty, 4)
    assert np.array_equal(comps['pixel'], rcomps['pixel']) and not (comps['pixel'] == bright).any()
    assert (res[:, :2, bright] != dirty[:, :2, bright]).all() and word_error(res, ref, sc).max() <= 5 * gap
    cl.set_window(np.zeros(npix, np.uint8))
    res, comps, stats = cl.run(dirty, 4)
    assert res.tobytes() == dirty.tobytes() and (stats['ncomp'] == 0).all() and (stats['reason'] == 2).all() and not stats['peak'].view(np.uint32).any()
    cl.set_window(None)                              # (every pixel again: the brightest pixel of the list wins)
    res, comps, stats = cl.run(dirty, 1)
    assert np.array_equal(comps['pixel'][:, 0], np.argmax(np.abs(dirty[:, 0] + dirty[:, 1]), axis=1))
    cl.close()


# ---------------------------------------------------------------- 6. a NaN stays in its group
def test_nan_stays_within_its_channel_group():
    """Three groups.  XX of group 1 all NaN: that group stops with reason 2, no component, and its residual is its input bit for bit;
    the other groups are those of the clean run bit for bit.  One NaN pixel (in the window) of group 1: it is never a component, it
    stays NaN, and the group goes on around it; Im XY of group 2 all NaN (an image whose group held a NaN visibility): I is finite, so
    the group is cleaned, its Im XY words stay NaN and its other words are the clean run's."""
    c = case(22, 37, 6, 2, False)
    dirty = c['dirty']
    cl = CL(c, 4)
    good = cl.run(dirty, 4)
    bad = dirty.copy()
    bad[1, 0] = np.nan
    res, comps, stats = cl.run(bad, 4)
    assert (stats['ncomp'][1], stats['reason'][1]) == (0, 2) and res[1].tobytes() == bad[1].tobytes() and (comps['pixel'][1] == -1).all()
    for g in (0, 2):
        assert res[g].tobytes() == good[0][g].tobytes() and comps[g].tobytes() == good[1][g].tobytes() and stats[g].tobytes() == good[2][g].tobytes()
    x = int(good[1]['pixel'][1, 0])
    bad = dirty.copy()
    bad[1, 1, x] = np.nan
    bad[2, 3] = np.nan
    res, comps, stats = cl.run(bad, 4)
    cl.close()
    assert stats['ncomp'][1] == 4 and not (comps['pixel'][1] == x).any() and np.isnan(res[1, 1, x]) and np.isfinite(np.delete(res[1], x, axis=1)).all()
    assert res[0].tobytes() == good[0][0].tobytes()
    assert np.isnan(res[2, 3]).all() and res[2, :3].tobytes() == good[0][2, :3].tobytes() and np.array_equal(comps['pixel'][2], good[1]['pixel'][2])
    assert np.isnan(comps['C'][2, :, 3]).all() and comps['C'][2, :, :3].tobytes() == good[1]['C'][2, :, :3].tobytes()


# ---------------------------------------------------------------- 7. the ABI
def test_info_tickets_and_argument_checks_with_and_without_a_context():
    """GetInfo follows SetControl's niter; Run before SetGeometry is INVALID_STATE and launches nothing; SetWeights, SetGeometry and
    SetControl refuse what the contract lists and change nothing; tickets count from 1 after Initialize and every one is done after
    Sync; every INVALID_ARGUMENT of Initialize leaves a live context alone; after Destroy every call that needs a context is
    INVALID_STATE."""
    nstand, npix, nfine, nfavg, niter = 6, 5, 4, 2, 3
    c = case(nstand, npix, nfine, nfavg, False)
    tau, freq, w = np.ascontiguousarray(c['tau']), np.ascontiguousarray(c['freq']), c['w']
    cl = CL(c, niter, geometry=False, gpu_state=False)
    assert _info() == (2, 256, 16 * 2 * 5, 16 * 2 * 5 + 32 * 2 * 3, 16 * 2 * 5 + 32 * 2 * 3 + 32, image_norm(np.ones(nstand), False, nfavg))
    cl.upload(c['dirty'])
    with pytest.raises(ffi.XengError) as ei:
        cl.enqueue()
    assert ei.value.status == INVALID_STATE
    ffi.call("xengCleanSync")
    raw = cl.dout.download(np.uint8)
    assert (raw == POISON).all()                    # (nothing was written)
    ffi.call("xengCleanSetGeometry", _dp(tau), _dp(freq))
    for bad_tau, bad_freq in ((np.where(np.arange(tau.size).reshape(tau.shape) == 7, np.nan, tau), freq), (tau, np.where(np.arange(nfine) == 1, np.inf, freq))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCleanSetGeometry", _dp(np.ascontiguousarray(bad_tau)), _dp(np.ascontiguousarray(bad_freq)))
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengCleanSetWeights", _fp(w), 0)
    cl.set_window(c['mask'])
    first = cl.run(c['dirty'], niter)
    for bad, autos in (([1, 1, 1, 1, 1, -1], 1), ([1, 1, 1, 1, 1, np.nan], 1), ([1, 1, 1, 1, 1, np.inf], 0), ([0] * 6, 1), ([0, 0, 3, 0, 0, 0], 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCleanSetWeights", _fp(np.array(bad, np.float32)), autos)
        assert ei.value.status == INVALID_ARGUMENT, bad
    for args in ((-1, 0.5, 0, 0), (niter + 1, 0.5, 0, 0), (1, 0.0, 0, 0), (1, 1.5, 0, 0), (1, np.nan, 0, 0), (1, 0.5, -1.0, 0), (1, 0.5, np.inf, 0),
                 (1, 0.5, 0, -0.5), (1, 0.5, 0, np.nan)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCleanSetControl", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert abs(_info()[5] / image_norm(w, False, nfavg) - 1) < 1e-15
    cl.upload(c['dirty'])
    cl.enqueue()
    ffi.call("xengCleanSync")
    assert _same(cl.result(), first)                 # (the refused calls changed nothing: still niter, GAIN, 0, 0)
    cl.control(1)
    assert _info()[2:5] == clean_layout(2, 1, npix)
    cl.control(niter, 1.0)                           # (a gain of 1 is allowed)
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    ffi.call("xengCleanMark", ctypes.byref(t))
    t0 = t.value
    cl.enqueue()
    ffi.call("xengCleanMark", ctypes.byref(t))
    assert t.value == t0 + 1
    ffi.call("xengCleanWait", t.value)
    ffi.call("xengCleanSync")
    cl.result()
    for k in (t0, t0 + 1):
        ffi.call("xengCleanTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, t0 + 2):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCleanWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, nfine, nfavg, npix, niter), (0, nstand, nfine, 3, npix, niter), (0, 2049, nfine, nfavg, npix, niter), (0, nstand, nfine, nfavg, 0, niter),
                 (0, nstand, nfine, nfavg, npix, 0), (0, nstand, nfine, nfavg, npix, 4097)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCleanInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info()[0] == 2
    for args in ((None, cl.dout.ptr + GUARD), (cl.din.ptr, None), (cl.din.ptr + 8, cl.dout.ptr + GUARD), (cl.din.ptr, cl.dout.ptr + GUARD + 8)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCleanRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengCleanSync")
    assert (cl.dout.download(np.uint8) == POISON).all()
    cl.close()
    s, n, ll = ctypes.c_int(), ctypes.c_double(), ctypes.c_longlong()
    for name, args in (("xengCleanRun", (4096, 4096)), ("xengCleanSetGeometry", (_dp(tau), _dp(freq))), ("xengCleanSetWeights", (_fp(w), 0)),
                       ("xengCleanSetWindow", (None,)), ("xengCleanSetControl", (1, 0.5, 0.0, 0.0)),
                       ("xengCleanGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(ll), ctypes.byref(ll), ctypes.byref(ll), ctypes.byref(n))),
                       ("xengCleanMark", (ctypes.byref(t),)), ("xengCleanWait", (1,)), ("xengCleanTicketDone", (1, ctypes.byref(d))), ("xengCleanSync", ()),
                       ("xengCleanCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCleanDestroy")


# ---------------------------------------------------------------- 8. the chain on device rings
def _encode(x):
    """complex -> the F-engine's byte: 4-bit two's-complement real part in the high nibble, imaginary part in the low one"""
    re = np.clip(np.rint(x.real), -7, 7).astype(np.int16) & 0xF
    im = np.clip(np.rint(x.imag), -7, 7).astype(np.int16) & 0xF
    return ((re << 4) | im).astype(np.uint8)


def test_source_to_upchan_corr_to_upchan_image_to_upchan_clean_on_device_rings():
    """Source -> UpchanCorr (44 inputs, 2 coarse channels, nupchan 2, one gulp of 256 samples per integration) -> UpchanImage (60
    pixels, groups of two fine channels) -> UpchanClean (niter 4, gain 0.5) on device rings, two integrations of voltages that hold two
    noise-like sources at list pixels (amplitudes 4 and 2.5 on every input with their delays, an array of 100 m, plus receiver
    noise): in every group the first component sits on the brighter source's pixel and every component on one of the two; each span
    is the float64 restatement of CLEAN on the image span UpchanImage wrote, pixels exact, words within five float gaps; the header
    says what was done."""
    nstand, nchan, g, N, npix, nfavg, seq0, sfreq, niter = 22, 2, 256, 2, 60, 2, 6400, 55e6, 4
    ninput, nfine = 2 * nstand, nchan * N
    rng = np.random.default_rng(91)
    pos, lmn = random_array(rng, nstand, 100.0, 3.0), sky(rng, npix)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[6] = 0
    window = np.ones(npix, bool)
    window[5::9] = False
    src = (17, 40)
    assert window[list(src)].all()
    tau = steering_delays(pos, lmn)
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=sfreq)
    fc = sfreq + hdr['bw_hz'] / nchan * np.arange(nchan)                 # the coarse channels' centres
    x = 1.2 * (rng.standard_normal((2 * g, nchan, ninput)) + 1j * rng.standard_normal((2 * g, nchan, ninput)))
    for px, amp in zip(src, (4.0, 2.5)):
        s = amp * (rng.standard_normal((2 * g, nchan, 1)) + 1j * rng.standard_normal((2 * g, nchan, 1))) / np.sqrt(2)
        x = x + s * np.repeat(np.exp(-2j * np.pi * fc[:, None] * tau[px][None, :]), 2, axis=1)[None]
    vin = _encode(x)
    r0, r1, r2, r3 = Ring("f-engine", space="cuda"), Ring("uc-output", space="cuda"), Ring("image-output", space="cuda"), Ring("clean-output", space="cuda")
    uc = UpchanCorr(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=g // N, gpu=0)
    im = UpchanImage(LOG, r1, r2, pos, lmn, nfavg=nfavg, weights=w, autos=False, gpu=0)
    cb = UpchanClean(LOG, r2, r3, pos, lmn, niter, gain=GAIN, window=window, weights=w, gpu=0)
    ngroup = nfine // nfavg
    nimg, (co, so, nspan) = ngroup * 4 * npix * 4, clean_layout(ngroup, niter, npix)
    mid, sink = Sink(r2, nimg), Sink(r3, nspan)
    run_blocks([uc, im, cb], Source(r0, [(hdr, vin.reshape(-1), g * nchan * ninput)]), [mid, sink])
    ok = ctypes.c_int()
    ffi.call("xengCleanCheckGuards", ctypes.byref(ok))
    for name in ("xengCleanDestroy", "xengImageDestroy", "xengUpchanCorrDestroy"):
        ffi.call(name)
    assert ok.value == 1
    (ih, _, ispans), = mid.sequences
    (ch, ctag, cspans), = sink.sequences
    assert len(ispans) == len(cspans) == 2 and ctag == ch['seq0'] == seq0 and cb.stats['nclean'] == 2
    assert (ch['cleaned'], ch['niter'], ch['gain'], ch['threshold'], ch['fraction'], ch['comp_offset'], ch['stats_offset']) == (True, niter, GAIN, 0.0, 0.0, co, so)
    assert all(ch[k] == ih[k] for k in ('npix', 'nfavg', 'nprod', 'autos', 'nfine', 'fine_sfreq', 'fine_bw_hz', 'image_sfreq'))
    freq = ih['fine_sfreq'] + ih['fine_bw_hz'] * np.arange(nfine)
    for k in range(2):
        dirty = ispans[k].view(np.float32).reshape(ngroup, 4, npix)
        c = dict(dirty=dirty, freq=freq, tau=tau, w=w, autos=False, nfavg=nfavg, mask=window.astype(np.uint8))
        ref, rcomps, rstats, sc, gap = _reference(c, niter)
        comps, stats, res = clean_components(cspans[k], ngroup, niter, npix)
        assert np.array_equal(comps['pixel'], rcomps['pixel']) and (stats['ncomp'] == niter).all() and (stats['reason'] == 0).all()
        assert (comps['pixel'][:, 0] == src[0]).all() and np.isin(comps['pixel'], src).all()
        assert max(word_error(res, ref, sc).max(), component_error(comps, rcomps, sc).max()) <= 5 * gap
