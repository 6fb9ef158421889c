"""UpchanImage on the MI355X: xengImage* against the restatement (tests/image_ref.py).  Parity with the float64 restatement on
Hermitian matrices of uneven rows; exact cases on small integers; a point source; bit identity of sub-lists of pixels, after
SetWeights back and forth, in a fresh context and beside an X-engine contraction and xengBeamformRun; a flagged stand that holds
NaN; a NaN in a stand that is read; the ABI with a context; Source -> UpchanCorr -> UpchanImage on device rings.  The output sits
between two poisoned 64 KiB guard bands that are checked after every call, the state's guards at every close.  No wall-clock
assertions.

The bar of the float tests is not a constant: it is five times the worst gap between the complex64 and the float64 evaluation of
the restatement ON THE TEST'S OWN INPUTS (tests/image_ref.py float_gap), per word as |I - I_ref| / (norm * sum_c sum_{s,t} w_s w_t
|V[c][s p][t q]|), so a faint pixel is not allowed a bright sky's error by another route.  Measured here on the CPU with numpy 2.2
on the parity test's inputs (arrays of 1.2 km, so phases of hundreds of turns; rows of scales 0.5 to 50): gaps of 2.0e-7 (22
stands, 37 pixels), 1.0e-7 (35 stands, 1 pixel) and 1.1e-7 (64 stands, 64 pixels), so bars of 5e-7 to 1.0e-6.  Measured on the
MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import UpchanCorr, UpchanImage, image_norm, steering_delays  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.image_ref import float_gap, hermitian_uneven, image, masked, point_source, random_array, scale, word_error  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.upchan_corr_ref import fine_freqs, upchan_corr, upchan_corr_scale  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
FINE_BW = 23925.78125 / 2
# worst word error / bar over test_parity_with_the_float64_restatement on the MI355X, per case
MEASURED = {(22, 37): 0.07, (35, 1): 0.02, (64, 64): 0.03}       # (worst errors 7.3e-8, 1.0e-8, 1.8e-8; the point source reads 1 to 6.0e-8)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _info():
    g, t, l, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    ffi.call("xengImageGetInfo", ctypes.byref(g), ctypes.byref(t), ctypes.byref(l), ctypes.byref(n))
    return g.value, t.value, l.value, n.value


def _sky(rng, n):
    """n directions above the horizon, the first the zenith where there is more than one: float64 [n][3]"""
    lm = rng.uniform(-0.65, 0.65, (n, 2))
    if n > 1:
        lm[0] = 0
    return np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)


def _setup(seed, nstand, npix, nfine, f0=50e6, flagged=(), extent=1200.0):
    """(rng, tau [npix][nstand], freq [nfine], w f32 [nstand] between 0.5 and 2 with the `flagged` stands at 0)"""
    rng = np.random.default_rng(seed)
    tau = steering_delays(random_array(rng, nstand, extent, 5.0), _sky(rng, npix))
    freq = f0 + FINE_BW * np.arange(nfine)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[list(flagged)] = 0
    return rng, tau, freq, w


class IM:
    """The xengImage context (one per process), an input buffer and the output of one call between two poisoned guard bands."""

    def __init__(self, tau, freq, nfavg, geometry=True):
        self.npix, self.nstand = tau.shape
        self.nfine, self.nfavg = len(freq), nfavg
        ffi.call("xengImageInitialize", 0, self.nstand, self.nfine, nfavg, self.npix)
        if geometry:
            ffi.call("xengImageSetGeometry", _dp(np.ascontiguousarray(tau, np.float64)), _dp(np.ascontiguousarray(freq, np.float64)))
        self.din = ffi.DeviceBuffer(self.nfine * (2 * self.nstand) ** 2 * 8)
        self.nout = (self.nfine // nfavg) * 4 * self.npix * 4
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nout)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def set_weights(self, w, autos):
        ffi.call("xengImageSetWeights", _fp(np.ascontiguousarray(w, np.float32)), int(autos))

    def upload(self, V):
        assert V.shape == (self.nfine, self.nstand, 2, self.nstand, 2) and V.dtype == np.complex64
        self.din.upload(np.ascontiguousarray(V))

    def enqueue(self):
        ffi.call("xengImageRun", self.din.ptr, self.dout.ptr + GUARD)

    def result(self):
        """After a sync: the image (the poison is put back); every byte before it and past it must still be poison."""
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.nout:] == POISON).all(), "bytes past the output were written"
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + self.nout].copy().view(np.float32).reshape(self.nfine // self.nfavg, 4, self.npix)

    def run(self, V):
        self.upload(V)
        self.enqueue()
        ffi.call("xengImageSync")
        return self.result()

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengImageCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengImageDestroy")
        self.din.free()
        self.dout.free()


# ---------------------------------------------------------------- 1. parity with float64
@pytest.mark.parametrize("nstand,npix,nfine,nfavg,autos", [(22, 37, 4, 1, False), (35, 1, 4, 2, True), (64, 64, 2, 2, False)])
def test_parity_with_the_float64_restatement(nstand, npix, nfine, nfavg, autos):
    """A partial column tile and a ragged second pixel tile; an odd stand count over two column tiles and a single pixel; an exact
    fit of two column tiles and two pixel tiles.  One stand flagged.  Every word within five float gaps of the float64
    restatement, the error measured against norm * sum w_s w_t |V|."""
    rng, tau, freq, w = _setup(100 + nstand, nstand, npix, nfine, flagged=(3,))
    V = hermitian_uneven(rng, nfine, nstand)
    gap = float_gap(V, freq, tau, w, autos, nfavg)
    im = IM(tau, freq, nfavg)
    im.set_weights(w, autos)
    got = im.run(V)
    assert abs(_info()[3] - image_norm(w, autos, nfavg)) <= 1e-15 * image_norm(w, autos, nfavg)
    im.close()
    err = word_error(got, V, freq, tau, w, autos, nfavg)
    print("image parity %d stands %d pixels: float gap %.3g, worst error %.3g = %.2f of the bar" % (nstand, npix, gap, err.max(), err.max() / (5 * gap)))
    assert np.isfinite(got).all() and (err <= 5 * gap).all(), (err.max(), 5 * gap)


# ---------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("autos", [False, True])
def test_small_integers_with_unit_steering_equal_the_int64_restatement(autos):
    """tau = 0: every steering factor is w_s exactly.  V small Gaussian integers, w in {0, 1, 2}: every partial sum is an integer
    below 2^24, so the image is float32(S) * float32(norm) with S = sum_c sum_{s,t} w_s w_t V[c][s p][t q] in int64, bit for bit
    -- 35 stands (two column tiles, an odd k count), 33 pixels (two tiles), groups of two channels."""
    nstand, npix, nfine, nfavg = 35, 33, 4, 2
    rng = np.random.default_rng(211 + autos)
    w = rng.integers(0, 3, nstand)
    w[:3] = (1, 2, 0)
    re = rng.integers(-7, 8, (nfine, nstand, 2, nstand, 2))
    iv = rng.integers(-7, 8, (nfine, nstand, 2, nstand, 2))
    keep = (w != 0)[:, None] & (w != 0)[None, :] & (autos | ~np.eye(nstand, dtype=bool))
    S = np.zeros((nfine, 4), np.int64)
    for k, (part, p, q) in enumerate(((re, 0, 0), (re, 1, 1), (re, 0, 1), (iv, 0, 1))):
        S[:, k] = np.einsum('s,cst,t->c', w, np.where(keep[None], part[:, :, p, :, q], 0), w)
    S = S.reshape(nfine // nfavg, nfavg, 4).sum(axis=1)
    assert 0 < np.abs(S).max() < 2 ** 24
    exp = S.astype(np.float32) * np.float32(image_norm(w, autos, nfavg))
    im = IM(np.zeros((npix, nstand)), 50e6 + FINE_BW * np.arange(nfine), nfavg)
    im.set_weights(w.astype(np.float32), autos)
    got = im.run((re + 1j * iv).astype(np.complex64))
    im.close()
    assert np.array_equal(got, np.broadcast_to(exp[:, :, None], got.shape))


# ---------------------------------------------------------------- 3. a point source
def test_point_source_peaks_at_its_pixel_and_reads_one():
    """A unit source at list pixel 21 of 40 (the second pixel tile), 30 stands, two groups of two channels: the largest XX and YY
    of each group are at that pixel, |I - 1| there is within the bar (the scale of the error measure is 1 for |V| = 1), and XX
    and YY are equal bit for bit (equal polarisations take the same sums)."""
    nstand, npix, nfine, nfavg, x0 = 30, 40, 4, 2, 21
    rng, tau, freq, w = _setup(31, nstand, npix, nfine, flagged=(7,))
    V = point_source(freq, tau[x0])
    gap = float_gap(V, freq, tau, w, False, nfavg)
    im = IM(tau, freq, nfavg)
    im.set_weights(w, False)
    got = im.run(V)
    im.close()
    sc = scale(V, w, False, nfavg)
    assert np.max(np.abs(sc - 1)) < 1e-6
    assert (np.argmax(got[:, 0], axis=1) == x0).all() and (np.argmax(got[:, 1], axis=1) == x0).all()
    print("point source: float gap %.3g, |I - 1| %.3g" % (gap, np.abs(got[:, :3, x0].astype(np.float64) - 1).max()))
    assert (np.abs(got[:, :3, x0].astype(np.float64) - 1) <= 5 * gap * sc[:, :3, 0]).all() and (np.abs(got[:, 3, x0]) <= 5 * gap * sc[:, 3, 0]).all()
    assert got[:, 0].tobytes() == got[:, 1].tobytes()
    assert (word_error(got, V, freq, tau, w, False, nfavg) <= 5 * gap).all()


# ---------------------------------------------------------------- 4. bit identity
def test_sub_lists_weights_back_and_forth_fresh_context_and_other_kernels_change_no_bit():
    """37 pixels, 22 stands.  Every third pixel, and the last one alone, in contexts of their own: the corresponding words of the
    full image.  The same call after SetWeights to other weights (which changes the image) and back; in a fresh context; and in a
    fresh context while X-engine contractions run on their streams and xengBeamformRun on this one."""
    nstand, npix, nfine, nfavg = 22, 37, 4, 2
    rng, tau, freq, w = _setup(41, nstand, npix, nfine, flagged=(5,))
    V = hermitian_uneven(rng, nfine, nstand)
    w1 = np.roll(w, 3)
    im = IM(tau, freq, nfavg)
    im.set_weights(w, False)
    full = im.run(V)
    im.set_weights(w1, True)
    other = im.run(V)
    im.set_weights(w, False)
    again = im.run(V)
    im.close()
    assert again.tobytes() == full.tobytes() and other.tobytes() != full.tobytes() and not np.isnan(full).any()
    for sel in (slice(None, None, 3), slice(npix - 1, None)):
        im = IM(np.ascontiguousarray(tau[sel]), freq, nfavg)
        im.set_weights(w, False)
        sub = im.run(V)
        im.close()
        assert sub.tobytes() == np.ascontiguousarray(full[:, :, sel]).tobytes()
    bstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, bstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * bstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    im = IM(tau, freq, nfavg)
    im.set_weights(w, False)
    im.upload(V)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(3):
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            im.enqueue()
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengImageSync")
            got.append(im.result())
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    im.close()
    ffi.call("xengBeamformDestroy")
    assert all(g.tobytes() == full.tobytes() for g in got)


# ---------------------------------------------------------------- 5., 6. non-finite visibilities
def test_flagged_stand_holding_nan_is_the_stand_holding_zeros():
    """w_9 = 0 and w_32 = 0 (one in each column tile), NaN and Inf all over their rows and columns: bit-identical to the same
    matrix with zeros there, and finite."""
    nstand, npix, nfine, nfavg = 35, 33, 2, 1
    rng, tau, freq, w = _setup(51, nstand, npix, nfine, flagged=(9, 32))
    V = hermitian_uneven(rng, nfine, nstand)
    zeros, bad = V.copy(), V.copy()
    for s in (9, 32):
        zeros[:, s] = 0
        zeros[:, :, :, s] = 0
        bad[:, s] = np.nan
        bad[:, :, :, s] = np.inf
    im = IM(tau, freq, nfavg)
    im.set_weights(w, True)
    a, b = im.run(zeros), im.run(bad)
    im.close()
    assert np.isfinite(a).all() and a.tobytes() == b.tobytes() and a.any()


def test_nan_in_a_read_stand_stays_within_its_channel_group():
    """A NaN in V[c = 2][4 0][11 1] (group 1 of three groups of two channels): every other group is bit-identical to the clean
    run; group 1's XY words are NaN at every pixel."""
    nstand, npix, nfine, nfavg = 22, 37, 6, 2
    rng, tau, freq, w = _setup(61, nstand, npix, nfine)
    V = hermitian_uneven(rng, nfine, nstand)
    bad = V.copy()
    bad[2, 4, 0, 11, 1] = np.nan
    im = IM(tau, freq, nfavg)
    im.set_weights(w, False)
    clean, got = im.run(V), im.run(bad)
    im.close()
    assert np.isfinite(clean).all() and got[[0, 2]].tobytes() == clean[[0, 2]].tobytes()
    assert np.isnan(got[1, 2:]).all() and got[1, :2].tobytes() == clean[1, :2].tobytes()


# ---------------------------------------------------------------- 7. the ABI
def test_info_tickets_and_argument_checks_with_and_without_a_context():
    """GetInfo; Run before SetGeometry is INVALID_STATE and launches nothing; SetWeights refuses negative, non-finite and all-zero
    weights and, without autos, a single live stand, and changes nothing; tickets count from 1 after Initialize and every one is
    done after Sync; every INVALID_ARGUMENT of Initialize leaves a live context alone; after Destroy every call that needs a
    context is INVALID_STATE."""
    nstand, npix, nfine, nfavg = 6, 5, 4, 2
    rng, tau, freq, w = _setup(71, nstand, npix, nfine)
    V = hermitian_uneven(rng, nfine, nstand)
    im = IM(tau, freq, nfavg, geometry=False)
    ones = np.ones(nstand)
    assert _info()[:3] == (2, 32, 32 * 33 * 8 + 32 * 4 + 4 * 4 * 32 * 4) and _info()[3] == image_norm(ones, False, nfavg)
    im.upload(V)
    with pytest.raises(ffi.XengError) as ei:
        im.enqueue()
    assert ei.value.status == INVALID_STATE
    ffi.call("xengImageSync")
    im.result()                                 # (nothing was written)
    ffi.call("xengImageSetGeometry", _dp(tau), _dp(freq))
    for bad_tau, bad_freq in ((np.where(np.arange(tau.size).reshape(tau.shape) == 7, np.nan, tau), freq), (tau, np.where(np.arange(nfine) == 1, np.inf, freq))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImageSetGeometry", _dp(np.ascontiguousarray(bad_tau)), _dp(np.ascontiguousarray(bad_freq)))
        assert ei.value.status == INVALID_ARGUMENT
    im.set_weights(w, False)
    first = im.run(V)
    for bad, autos in (([1, 1, 1, 1, 1, -1], 1), ([1, 1, 1, 1, 1, np.nan], 1), ([1, 1, 1, 1, 1, np.inf], 0), ([0] * 6, 1), ([0, 0, 3, 0, 0, 0], 0)):
        with pytest.raises(ffi.XengError) as ei:
            im.set_weights(np.array(bad, np.float32), autos)
        assert ei.value.status == INVALID_ARGUMENT, bad
    assert abs(_info()[3] / image_norm(w, False, nfavg) - 1) < 1e-15 and im.run(V).tobytes() == first.tobytes()
    im.set_weights(np.array([0, 0, 3, 0, 0, 0], np.float32), True)       # (one stand with its autos is an image)
    one = im.run(V)
    exp = np.stack([V[:, 2, 0, 2, 0].real, V[:, 2, 1, 2, 1].real, V[:, 2, 0, 2, 1].real, V[:, 2, 0, 2, 1].imag], axis=1).reshape(2, 2, 4).mean(axis=1)
    assert np.allclose(one, np.broadcast_to(exp[:, :, None], one.shape), rtol=1e-6, atol=1e-6 * np.abs(exp).max())
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    ffi.call("xengImageMark", ctypes.byref(t))
    assert t.value == 1
    im.enqueue()
    ffi.call("xengImageMark", ctypes.byref(t))
    assert t.value == 2
    ffi.call("xengImageWait", 2)
    ffi.call("xengImageSync")
    im.result()
    for k in (1, 2):
        ffi.call("xengImageTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, 3):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImageWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, nfine, nfavg, npix), (0, nstand, nfine, 3, npix), (0, 513, nfine, nfavg, npix), (0, nstand, nfine, nfavg, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImageInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info()[0] == 2
    for args in ((None, im.dout.ptr + GUARD), (im.din.ptr, None), (im.din.ptr + 8, im.dout.ptr + GUARD), (im.din.ptr, im.dout.ptr + GUARD + 8)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengImageRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengImageSync")
    im.result()
    im.close()
    s, n = ctypes.c_int(), ctypes.c_double()
    for name, args in (("xengImageRun", (4096, 4096)), ("xengImageSetGeometry", (_dp(tau), _dp(freq))), ("xengImageSetWeights", (_fp(w), 0)),
                       ("xengImageGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(s), ctypes.byref(n))), ("xengImageMark", (ctypes.byref(t),)),
                       ("xengImageWait", (1,)), ("xengImageTicketDone", (1, ctypes.byref(d))), ("xengImageSync", ()),
                       ("xengImageCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengImageDestroy")


# ---------------------------------------------------------------- 8. the chain on device rings
def test_source_to_upchan_corr_to_upchan_image_on_device_rings():
    """Source -> UpchanCorr (44 inputs, 2 coarse channels, nupchan 2, one gulp of 64 samples per integration) -> UpchanImage (37
    pixels, groups of two fine channels, one stand flagged) on device rings, two integrations: each image against the float64
    restatement applied to the float64 restatement of the visibilities (tests/upchan_corr_ref.py), within the image's bar (five
    float gaps on those visibilities) plus the visibilities' own bar, 1e-6 sum_f |X_i||X_j| per element, carried through
    norm * sum w_s w_t; the header says what was imaged."""
    nstand, nchan, g, N, npix, nfavg, seq0, sfreq = 22, 2, 64, 2, 37, 2, 6400, 55e6
    ninput, nfine = 2 * nstand, nchan * N
    rng = np.random.default_rng(81)
    pos, lmn = random_array(rng, nstand, 1200.0, 5.0), _sky(rng, npix)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[6] = 0
    vin = rng.integers(0, 256, (2 * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=sfreq)
    r0, r1, r2 = Ring("f-engine", space="cuda"), Ring("uc-output", space="cuda"), Ring("image-output", space="cuda")
    uc = UpchanCorr(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=g // N, gpu=0)
    im = UpchanImage(LOG, r1, r2, pos, lmn, nfavg=nfavg, weights=w, autos=False, gpu=0)
    mid, sink = Sink(r1, nfine * ninput * ninput * 8), Sink(r2, (nfine // nfavg) * 4 * npix * 4)
    run_blocks([uc, im], Source(r0, [(hdr, vin.reshape(-1), g * nchan * ninput)]), [mid, sink])
    ok = ctypes.c_int()
    ffi.call("xengImageCheckGuards", ctypes.byref(ok))
    ffi.call("xengImageDestroy")
    ffi.call("xengUpchanCorrDestroy")
    assert ok.value == 1
    (vh, _, vspans), = mid.sequences
    (ih, itag, ispans), = sink.sequences
    assert len(vspans) == len(ispans) == 2 and itag == ih['seq0'] == seq0 and im.stats['nimage'] == 2
    assert (ih['npix'], ih['nfavg'], ih['nprod'], ih['autos'], ih['nbit'], ih['complex'], ih['nfine']) == (npix, nfavg, 4, False, 32, False, nfine)
    freq = fine_freqs(sfreq, hdr['bw_hz'], nchan, N)
    assert np.allclose(freq, vh['fine_sfreq'] + vh['fine_bw_hz'] * np.arange(nfine), rtol=0, atol=1e-6)
    assert ih['image_sfreq'] == vh['fine_sfreq'] + vh['fine_bw_hz'] / 2 and ih['image_bw_hz'] == 2 * vh['fine_bw_hz']
    tau = steering_delays(pos, lmn)
    norm = image_norm(w, False, nfavg)
    for k in range(2):
        part = vin[k * g:(k + 1) * g]
        V = upchan_corr(part, N).reshape(nfine, nstand, 2, nstand, 2)
        ref = image(V, freq, tau, w, False, nfavg)
        got = ispans[k].view(np.float32).reshape(nfine // nfavg, 4, npix)
        sc = scale(V, w, False, nfavg)
        vbar = 1e-6 * upchan_corr_scale(part, N).reshape(nfine, nstand, 2, nstand, 2)
        A = masked(vbar, w, False)
        carried = np.einsum('s,cspt,t->cp', w.astype(np.float64), A[:, :, [0, 1, 0, 0], :, [0, 1, 1, 1]].transpose(1, 2, 0, 3), w.astype(np.float64))
        carried = carried.reshape(nfine // nfavg, nfavg, 4).sum(axis=1)[:, :, None] * norm
        bar = 5 * float_gap(V.astype(np.complex64), freq, tau, w, False, nfavg) * sc + carried
        assert (np.abs(got.astype(np.float64) - ref) <= bar).all()
