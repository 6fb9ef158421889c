"""The contract of xengClean* (include/xeng.h, "Hogbom CLEAN of the dirty images") restated in numpy: float64 by default, float32
step for step with a dtype argument (the gap between the two on a test's own inputs, given the same component pixels, is a fifth of
that test's bar), the error measure, the margin by which each peak was chosen, a fake backend that serves the clean_* calls
UpchanClean makes from the float32 restatement, and a generator of cases."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks.imaging import CLEAN_COMPONENT, CLEAN_STATS, image_norm, steering_delays
from tests.fake_backend import OracleBackend
from tests.image_ref import hermitian_uneven, image, point_source, random_array


def fractions(freq, tau):
    """fr_c(x, s): freq[c] tau[x][s] minus its nearest integer, float64 [nfine][npix][nstand]"""
    turns = np.asarray(freq, np.float64)[:, None, None] * np.asarray(tau, np.float64)[None]
    return turns - np.rint(turns)


def _fma32(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def psf(fr, w, autos, nfavg, x0, dtype=np.float64):
    """PSF_g(x, x0) [ngroup][npix] from the fractions `fr` [nfine][npix][nstand].  float64: the formula; float32: the kernel's steps
    (the difference of the fractions float64, then float32: fma chains over the live stands in ascending order, fma(Re, Re, Im Im)
    - D, the channels added in ascending order, one multiply by norm)."""
    nfine, npix, nstand = fr.shape
    w = np.asarray(w, np.float32)
    d = fr - fr[:, x0:x0 + 1, :]
    w64 = w.astype(np.float64)
    dsum = 0.0 if autos else float((w64 * w64).sum())
    norm = image_norm(w, autos, nfavg)
    if np.dtype(dtype) == np.float64:
        S = (w64 * np.exp(2j * np.pi * d)).sum(axis=2)
        p = (S.real ** 2 + S.imag ** 2 - dsum).reshape(nfine // nfavg, nfavg, npix)
        acc = np.zeros((nfine // nfavg, npix))
        for c in range(nfavg):
            acc = acc + p[:, c]
        return norm * acc
    ang = np.float32(2.0 * np.pi) * d.astype(np.float32)
    cs, sn = np.cos(ang), np.sin(ang)
    assert cs.dtype == np.float32
    sr, si = np.zeros((nfine, npix), np.float32), np.zeros((nfine, npix), np.float32)
    for s in range(nstand):
        if w[s] != 0:
            sr, si = _fma32(w[s], cs[:, :, s], sr), _fma32(w[s], sn[:, :, s], si)
    p = (_fma32(sr, sr, si * si) - np.float32(dsum)).reshape(nfine // nfavg, nfavg, npix)
    acc = np.zeros((nfine // nfavg, npix), np.float32)
    for c in range(nfavg):
        acc = acc + p[:, c]
    assert acc.dtype == np.float32
    return np.float32(norm) * acc


def clean(dirty, freq, tau, w, autos, nfavg, mask, niter, gain, threshold=0.0, fraction=0.0, dtype=np.float64, pixels=None):
    """The loop of the contract on dirty f32 [ngroup][4][npix].  Returns (residual `dtype` [ngroup][4][npix], components CLEAN_COMPONENT
    [ngroup][niter], stats CLEAN_STATS [ngroup], gaps): gaps[g] is the list, per recorded component, of best |I| minus second-best |I| in
    the window (inf with one candidate).  With `pixels` (a list of pixel lists, one per group) nothing is searched and nothing
    stops: those components are taken in that order -- what float_gap compares."""
    real = np.dtype(dtype).type
    dirty = np.asarray(dirty, np.float32)
    ngroup, _, npix = dirty.shape
    fr = fractions(freq, tau)
    win = np.ones(npix, bool) if mask is None else np.asarray(mask) != 0
    R = dirty.astype(real)
    comps = np.zeros((ngroup, niter), CLEAN_COMPONENT)
    comps['pixel'] = -1
    stats = np.zeros(ngroup, CLEAN_STATS)
    gaps = [[] for _ in range(ngroup)]
    gain, threshold, fraction = real(gain), real(threshold), real(fraction)
    cache = {}
    for g in range(ngroup):
        k, peak0 = 0, None
        while True:
            with np.errstate(invalid='ignore'):
                I = R[g, 0] + R[g, 1]
            a = np.where(win & np.isfinite(I), np.abs(I), -1)
            if pixels is not None:
                if k == len(pixels[g]):
                    stats[g] = (k, 0, 0, 0)
                    break
                xk = int(pixels[g][k])
            else:
                xk = int(np.argmax(a))                                  # (the first of equals: the lowest index)
                if a[xk] < 0:
                    stats[g] = (k, 2, 0, 0)
                    break
                if peak0 is None:
                    peak0 = a[xk]
                if a[xk] <= max(threshold, fraction * peak0):
                    stats[g] = (k, 1, a[xk], 0)
                    break
                if k == niter:
                    stats[g] = (k, 0, a[xk], 0)
                    break
                second = np.sort(a)[-2] if npix > 1 else -1
                gaps[g].append(float(a[xk] - second) if second >= 0 else np.inf)
            C = gain * R[g, :, xk]
            comps[g, k] = (xk, I[xk], C, 0)
            if (real, xk) not in cache:
                cache[real, xk] = psf(fr, w, autos, nfavg, xk, real)
            P = cache[real, xk][g]
            with np.errstate(invalid='ignore'):
                R[g] = _fma32(-C[:, None], P[None], R[g]) if real is np.float32 else R[g] - C[:, None] * P[None]
            k += 1
    assert R.dtype == real
    return R, comps, stats, gaps


def scale(dirty, comps):
    """max_x |dirty| + sum_k |C_k| per (group, word): f64 [ngroup][4][1], what an error is measured against"""
    dirty = np.asarray(dirty, np.float64)
    with np.errstate(invalid='ignore'):
        top = np.nanmax(np.abs(np.where(np.isfinite(dirty), dirty, np.nan)), axis=2)
    return (top + np.abs(comps['C'].astype(np.float64)).sum(axis=1))[:, :, None]


def word_error(got, ref, sc):
    """|got - ref| / scale per word; 0 where both the difference and the scale are 0"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    sc = np.broadcast_to(sc, d.shape)
    return np.where(sc > 0, d / np.where(sc > 0, sc, 1), np.where(d > 0, np.inf, 0.0))


def float_gap(dirty, freq, tau, w, autos, nfavg, ref, comps, stats, gain):
    """The worst word_error, over the residual and the components' values, of the float32 restatement against the float64 run `ref`
    (its residual), both taking the float64 run's component pixels: a fifth of the float bar."""
    pixels = [list(comps['pixel'][g, :stats['ncomp'][g]]) for g in range(len(stats))]
    r32, c32, _, _ = clean(dirty, freq, tau, w, autos, nfavg, None, comps.shape[1], gain, dtype=np.float32, pixels=pixels)
    sc = scale(dirty, comps)
    return float(max(word_error(r32, ref, sc).max(), component_error(c32, comps, sc).max()))


def component_error(got, ref, sc):
    """word_error of the components' four words [ngroup][niter][4] against the words' scales"""
    return word_error(got['C'].transpose(0, 2, 1), ref['C'].transpose(0, 2, 1), sc)


def peak_margin(gaps, sc):
    """The smallest gap between the best and the second-best |I| over all iterations of a run, over the scale of I (the scales of XX
    and YY added: I is their sum, so an error of `float_gap` per word moves |I| by float_gap times that at the most)."""
    out = np.inf
    for g, gg in enumerate(gaps):
        if gg:
            out = min(out, min(gg) / float(sc[g, 0, 0] + sc[g, 1, 0]))
    return out


def sky(rng, n):
    """n directions above the horizon: float64 [n][3]"""
    lm = rng.uniform(-0.65, 0.65, (n, 2))
    return np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)


FINE_BW = 23925.78125 / 2


def case(nstand, npix, nfine, nfavg, autos, seed=None, fluxes=(3.0, 1.5), extent=1200.0, noise=0.02):
    """A dirty image with point sources of `fluxes` on window pixels plus noise * hermitian_uneven, imaged by tests/image_ref.image:
    one stand of weight 0 and one of weight 0.5 (where there are more than three), a window that leaves out every seventh pixel.
    Returns a dict: pos, lmn, tau, freq, w, mask u8, src (the sources' pixels), V complex64, dirty f32 [ngroup][4][npix]."""
    rng = np.random.default_rng(1000 + nstand if seed is None else seed)
    pos, lmn = random_array(rng, nstand, extent, 5.0), sky(rng, npix)
    tau = steering_delays(pos, lmn)
    freq = 50e6 + FINE_BW * np.arange(nfine)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    if nstand > 3:
        w[3], w[1] = 0, 0.5
    mask = np.ones(npix, np.uint8)
    mask[3::7] = 0
    src = rng.choice(np.flatnonzero(mask), size=min(len(fluxes), int(mask.sum())), replace=False)
    V = noise * hermitian_uneven(rng, nfine, nstand)
    for x, f in zip(src, fluxes):
        V = V + np.float32(f) * point_source(freq, tau[x])
    V = np.ascontiguousarray(V.astype(np.complex64))
    dirty = np.ascontiguousarray(image(V, freq, tau, w, autos, nfavg), np.float32)
    return dict(pos=pos, lmn=lmn, tau=tau, freq=freq, w=w, mask=mask, src=src, V=V, dirty=dirty, autos=autos, nfavg=nfavg)


def pack_span(residual, comps, stats):
    """The span of one Run as bytes: the residual f32, the records, the stats"""
    return np.concatenate([np.ascontiguousarray(residual, np.float32).reshape(-1).view(np.uint8), np.ascontiguousarray(comps).reshape(-1).view(np.uint8),
                           np.ascontiguousarray(stats).reshape(-1).view(np.uint8)])


class CleanBackend(OracleBackend):
    """The oracle backend plus xengClean* served by the float32 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.cl, self.calls = None, []
        self.tau = self.freq = self.w = self.mask = None
        self.control = None

    def clean_initialize(self, gpu, nstand, nfine, nfavg, npix, niter_max):
        if nfine % nfavg or not 1 <= niter_max <= 4096:
            return 1
        self.cl = dict(nstand=nstand, nfine=nfine, nfavg=nfavg, npix=npix, niter_max=niter_max)
        self.tau = self.freq = self.mask = None
        self.w, self.autos = np.ones(nstand, np.float32), False
        self.control = (niter_max, 0.1, 0.0, 0.0)
        self.calls.append('init')
        return 0

    def clean_set_geometry(self, tau, freq):
        u = self.cl
        self.tau = np.array(tau, np.float64).reshape(u['npix'], u['nstand'])
        self.freq = np.array(freq, np.float64).reshape(u['nfine'])
        self.calls.append('geometry')
        return 0

    def clean_set_weights(self, weights, autos):
        self.w, self.autos = np.array(weights, np.float32).reshape(self.cl['nstand']), bool(autos)
        self.calls.append('weights')
        return 0

    def clean_set_window(self, mask):
        self.mask = None if mask is None else np.array(mask, np.uint8).reshape(self.cl['npix'])
        self.calls.append('window')
        return 0

    def clean_set_control(self, niter, gain, threshold, fraction):
        if not (0 <= niter <= self.cl['niter_max'] and 0 < gain <= 1 and threshold >= 0 and fraction >= 0):
            return 1
        self.control = (int(niter), float(gain), float(threshold), float(fraction))
        self.calls.append(('control',) + self.control)
        return 0

    def clean_info(self):
        u = self.cl
        ngroup = u['nfine'] // u['nfavg']
        co = ngroup * 4 * u['npix'] * 4
        so = co + ngroup * self.control[0] * 32
        return ngroup, 256, co, so, so + ngroup * 16, image_norm(self.w, self.autos, u['nfavg'])

    def clean_run(self, image_arr, out_arr):
        u = self.cl
        if self.tau is None:
            return 2
        ngroup = u['nfine'] // u['nfavg']
        n = ngroup * 4 * u['npix']
        dirty = image_arr.numpy().reshape(-1).view(np.uint8)[:4 * n].view(np.float32).reshape(ngroup, 4, u['npix'])
        niter, gain, threshold, fraction = self.control
        R, comps, stats, _ = clean(dirty, self.freq, self.tau, self.w, self.autos, u['nfavg'], self.mask, niter, gain, threshold, fraction, np.float32)
        y = pack_span(R, comps, stats)
        out_arr.numpy().reshape(-1).view(np.uint8)[:y.nbytes] = y
        self.calls.append('run')
        return 0

    def clean_mark(self):
        return self.beam_mark()

    def clean_wait(self, ticket):
        self.beam_wait(ticket)

    def clean_sync(self):
        pass
