"""The contract of xengCalapply* (include/xeng.h, "Calibrated, source-subtracted visibilities") restated in numpy: float64 by default,
complex64 with a dtype argument (the gap between the two on a test's own inputs is a fifth of that test's bar); the error measure;
the bitwise Hermitian check; generators of cases (on tests/gaincal_ref.py's arrays, skies and gains)."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks.calibration import inverse_gains, model_flux
from tests.gaincal_ref import corrupt, model, noisy, setup, steering


def factors(g):
    """The apply factors of gains g [nfine][2][nstand]: inverse_gains in float64, rounded once; complex64 [nfine][2][nstand]"""
    g = np.asarray(g)
    inv = inverse_gains(g).reshape(g.shape[0], g.shape[2], 2)
    return np.ascontiguousarray(inv.transpose(0, 2, 1)).astype(np.complex64)


def per_input(h):
    """h [nfine][2][nstand] as [nfine][2 nstand] with input i = 2 s + p"""
    h = np.asarray(h)
    return np.ascontiguousarray(h.transpose(0, 2, 1)).reshape(h.shape[0], -1)


def model_tile(freq, tau, flux, dtype=np.complex128):
    """M [nfine][nstand][nstand] = sum_k (F_k a_ks) conj(a_kt), every step after the fraction of a turn in `dtype`'s precision"""
    dtype = np.dtype(dtype)
    real = np.float32 if dtype == np.complex64 else np.float64
    a = steering(freq, tau, dtype)
    F = model_flux(flux, len(freq), np.shape(tau)[0]).astype(real)
    M = np.einsum('cks,ckt->cst', (F[:, :, None] * a).astype(dtype), np.conj(a))
    assert M.dtype == dtype
    return M


def apply(V, h, freq=None, tau=None, flux=None, dtype=np.complex128):
    """The output of a Run: complex `dtype` [nfine][nstand][2][nstand][2].  Only the words i >= j of V are looked at; a word whose
    h_i or h_j is 0 is not looked at either (a select) and comes out as 0; the upper triangle is the conjugate of the lower, the
    diagonal real.  No model where tau is None or has no rows."""
    dtype = np.dtype(dtype)
    V = np.asarray(V)
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    hi = per_input(h).astype(dtype)
    live = hi != 0
    keep = live[:, :, None] & live[:, None, :]
    low = np.tril(np.ones((n, n), bool))
    A = np.where(keep & low[None], V.reshape(nfine, n, n), 0).astype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        Y = (hi[:, :, None] * np.conj(hi)[:, None, :]) * A
        if tau is not None and np.shape(tau)[0] > 0:
            M = model_tile(freq, tau, flux, dtype)
            Y5 = Y.reshape(nfine, nstand, 2, nstand, 2)
            for p in range(2):
                Y5[:, :, p, :, p] -= M
    assert Y.dtype == dtype
    Y = np.where(keep, Y, 0)
    L = np.where(np.tril(np.ones((n, n), bool), -1)[None], Y, 0)
    D = np.einsum('cii->ci', Y).real
    out = L + np.conj(L.transpose(0, 2, 1))
    out[:, np.arange(n), np.arange(n)] = D
    return out.reshape(nfine, nstand, 2, nstand, 2)


def scale(V, h, flux=None):
    """|h_i||h_j| max|V| + sum_k F_k per word, f64 [nfine][n][n]: what an error is measured against.  max|V| is over the finite
    words of the lower triangle of the whole input."""
    V = np.asarray(V)
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    A = np.abs(np.where(np.tril(np.ones((n, n), bool))[None], V.reshape(nfine, n, n), 0).astype(np.complex128))
    vmax = A[np.isfinite(A)].max()
    ah = np.abs(per_input(h).astype(np.complex128))
    fs = 0.0 if flux is None or not np.size(flux) else np.broadcast_to(np.asarray(flux, np.float64), (nfine, np.shape(flux)[-1])).sum(axis=1)
    return ah[:, :, None] * ah[:, None, :] * vmax + np.broadcast_to(fs, (nfine,))[:, None, None]


def word_error(got, ref, sc):
    """|got - ref| / scale per word; 0 where both the difference and the scale are 0."""
    n = sc.shape[-1]
    d = np.abs(np.asarray(got, np.complex128).reshape(-1, n, n) - np.asarray(ref, np.complex128).reshape(-1, n, n))
    return np.where(sc > 0, d / np.where(sc > 0, sc, 1), np.where(d > 0, np.inf, 0.0))


def float_gap(V, h, freq, tau, flux, ref=None):
    """The worst word_error of the complex64 evaluation against the float64 one: a fifth of the float bar."""
    ref = apply(V, h, freq, tau, flux) if ref is None else ref
    return float(word_error(apply(V, h, freq, tau, flux, np.complex64), ref, scale(V, h, flux)).max())


def hermitian_bits(out):
    """True if out (complex64, vis's layout) is Hermitian bit for bit: out[j][i] has out[i][j]'s real word and its imaginary word
    with the sign turned -- or both are +0 + 0i, a word that was left out -- and the diagonal's imaginary words are +0."""
    out = np.ascontiguousarray(out, np.complex64)
    nfine, nstand = out.shape[:2]
    n = 2 * nstand
    A = out.reshape(nfine, n, n)
    U = np.ascontiguousarray(A.transpose(0, 2, 1))
    re, im = np.ascontiguousarray(A.real).view(np.uint32), np.ascontiguousarray(A.imag).view(np.uint32)
    ure, uim = np.ascontiguousarray(U.real).view(np.uint32), np.ascontiguousarray(U.imag).view(np.uint32)
    nim = np.ascontiguousarray(-A.imag).view(np.uint32)
    zero = (re == 0) & (im == 0) & (ure == 0) & (uim == 0)
    off = ~np.eye(n, dtype=bool)[None]
    ok = np.where(off, ((ure == re) & (uim == nim)) | zero, im == 0)
    return bool(ok.all())


def case(nstand, nsrc, nfine, noise=0.05, seed=None, flagged=(3,), half_flagged=((5, 1),)):
    """(tau [nsrc][nstand], freq, flux f32 [nfine][nsrc], h c64 [nfine][2][nstand], V c64): tests/gaincal_ref.py's array of 1.2 km, its
    sky and its gains of modulus 0.5 to 2 and any phase; V = g g^H o M plus Hermitian noise of uneven rows, the cross hands
    included; h = 1 / g, 0 at the `flagged` stands and at the (stand, pol) of `half_flagged`.  With nsrc = 0 the sky that made V has
    one source and tau has no rows."""
    rng, tau, freq, flux, w, g = setup(200 + nstand if seed is None else seed, nstand, max(nsrc, 1), nfine)
    V = noisy(rng, corrupt(model(freq, tau, flux), g), noise)
    g = g.copy()
    for s in flagged:
        g[:, :, s] = 0
    for s, p in half_flagged:
        g[:, p, s] = 0
    if nsrc == 0:
        tau, flux = tau[:0], flux[:, :0]
    return tau, freq, np.ascontiguousarray(flux), factors(g), V
