"""The contract of xengGaincal* (include/xeng.h, "Per-stand gains from the fine-channel visibilities") restated in numpy, by the
contract's own route (N by the contraction over the sources' steering rows, D from the K x K Gram matrix minus the t = s term):
float64 by default, complex64 with a dtype argument (the gap between the two on a test's own inputs is a fifth of that test's
bar); a textbook dense StEFCal to compare it with; the error measure; generators of arrays, skies, gains and visibilities."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks.calibration import model_flux, model_visibilities
from caltech_bifrost_dsp_amd.blocks.imaging import steering_delays
from tests.image_ref import hermitian_uneven, random_array

FINE_BW = 23925.78125 / 2


def steering(freq, tau, dtype=np.complex128):
    """a[c][k][s] = exp(-2 pi i frac(freq[c] tau[k][s])): the product and its fraction of a turn in float64 whatever `dtype`; with
    complex64 the sine and the cosine are single precision."""
    turns = np.asarray(freq, np.float64)[:, None, None] * np.asarray(tau, np.float64)[None]
    fr = turns - np.rint(turns)
    if np.dtype(dtype) == np.complex64:
        ang = np.float32(2.0 * np.pi) * fr.astype(np.float32)
        return (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex64)
    return np.exp(-2j * np.pi * fr)


def read_block(V, w, c, p):
    """What the kernel loads of channel c, polarisation p: X[s][t] = conj(V[c][t p][s p]) with the rows and columns of the stands of
    weight 0 and the diagonal replaced by zeros -- a select, so NaN there does not get through."""
    live = np.asarray(w) != 0
    keep = live[:, None] & live[None, :] & ~np.eye(len(live), dtype=bool)
    return np.where(keep, np.conj(V[c, :, p, :, p]).T, 0)


def solve(V, freq, tau, flux, w, refant, niter, tol, dtype=np.complex128, start=None, average=True, trace=None):
    """(gains [nfine][2][nstand], stats f64 [nfine][2][4], keep): the contract, every step in `dtype`'s precision.  `start` is the
    `keep` of an earlier call, (unreferenced gains [nfine][2][nstand], converged and finite [nfine][2]): the warm start.
    average = False leaves the averaging step of the even iterations out (to show that it matters); a list `trace` receives
    (c, p, iteration, delta) of every delta formed."""
    dtype = np.dtype(dtype)
    real = np.float32 if dtype == np.complex64 else np.float64
    nfine, nstand = V.shape[:2]
    F = model_flux(flux, nfine, np.shape(tau)[0]).astype(real)
    w = np.asarray(w).astype(real)
    live = w != 0
    a_all = steering(freq, tau, dtype)
    gains = np.zeros((nfine, 2, nstand), dtype)
    stats = np.zeros((nfine, 2, 4))
    keep_g = np.zeros((nfine, 2, nstand), dtype) if start is None else np.array(start[0], dtype)
    keep_ok = np.zeros((nfine, 2), bool) if start is None else np.array(start[1], bool)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for c in range(nfine):
            a = np.where(live[None], a_all[c], 0).astype(dtype)                      # [k][s]
            z = F[c][:, None] * a                                                    # F_k a_ks
            fsum2 = real(F[c].sum(dtype=real)) ** 2
            for p in range(2):
                X = read_block(V, w, c, p).astype(dtype)
                g = np.where(live, keep_g[c, p] if start is not None and keep_ok[c, p] else 1, 0).astype(dtype)
                it, conv, delta = 0, False, -1.0
                while it < niter and not conv:
                    U = (w * g * a) @ X.T                                            # U[k][s] = sum_t h_kt X[s][t]
                    N = (np.conj(z) * U).sum(axis=0)
                    q = w * (g.real ** 2 + g.imag ** 2)
                    G = (q * np.conj(a)) @ a.T                                       # G[k][k'] = sum_t q_t conj(a_kt) a_k't
                    D = (z * (G @ np.conj(z))).sum(axis=0).real - q * fsum2
                    assert U.dtype == dtype and D.dtype == real
                    new = np.where(live & (D > 0), N / np.where(D > 0, D, 1), 0).astype(dtype)
                    it += 1
                    if it % 2 == 0:
                        delta = float(np.sqrt((np.abs(new - g)[live] ** 2).sum(dtype=real) / (np.abs(new)[live] ** 2).sum(dtype=real)))
                        if trace is not None:
                            trace.append((c, p, it, delta))
                        if tol > 0 and delta <= real(tol):
                            conv = True
                        elif average:
                            new = ((new + g) * real(0.5)).astype(dtype)
                    g = new
                mag = np.abs(g[refant])
                gains[c, p] = g * (np.conj(g[refant]) / mag if mag > 0 else 1)
                stats[c, p] = (it, delta, np.count_nonzero(live & (g != 0)), conv)
                if niter > 0:
                    keep_g[c, p], keep_ok[c, p] = g, conv and bool(np.all(np.isfinite(g)))
    return gains, stats, (keep_g, keep_ok)


def textbook_stefcal(V, M, w, refant, niter):
    """Dense StEFCal in float64 on the model matrix M [nfine][nstand][nstand] (blocks/calibration.py model_visibilities), `niter`
    iterations with the average on the even ones and no exit: g_s = sum_{t != s} w_t X[s][t] g_t M[t][s] / sum_{t != s} w_t |g_t
    M[t][s]|^2.  Gains [nfine][2][nstand], phase referenced."""
    nfine, nstand = V.shape[:2]
    w = np.asarray(w, np.float64)
    live = w != 0
    out = np.zeros((nfine, 2, nstand), np.complex128)
    for c in range(nfine):
        for p in range(2):
            X = read_block(V, w, c, p).astype(np.complex128)
            g = np.where(live, 1.0 + 0j, 0)
            for it in range(1, niter + 1):
                Z = (w * g)[:, None] * M[c]                                          # Z[t][s] = w_t g_t M[t][s]
                N = np.einsum('st,ts->s', X, Z)
                D = np.einsum('t,ts->s', w * np.abs(g) ** 2, np.abs(M[c]) ** 2 * ~np.eye(nstand, dtype=bool))
                new = np.where(live & (D > 0), N / np.where(D > 0, D, 1), 0)
                g = (new + g) / 2 if it % 2 == 0 else new
            out[c, p] = g * np.conj(g[refant]) / np.abs(g[refant])
    return out


def gain_error(got, ref):
    """max_s |g - g_ref| / rms_s |g_ref| per (channel, pol): f64 [nfine][2]"""
    ref = np.asarray(ref, np.complex128)
    return np.abs(np.asarray(got, np.complex128) - ref).max(axis=-1) / np.sqrt((np.abs(ref) ** 2).mean(axis=-1))


def float_gap(V, freq, tau, flux, w, refant, niter, tol=0.0, ref=None):
    """The worst gain_error of the complex64 evaluation against the float64 one: a fifth of the float bar."""
    ref = solve(V, freq, tau, flux, w, refant, niter, tol)[0] if ref is None else ref
    return float(np.max(gain_error(solve(V, freq, tau, flux, w, refant, niter, tol, np.complex64)[0], ref)))


def sky(rng, n):
    """n directions above the horizon: float64 [n][3]"""
    lm = rng.uniform(-0.65, 0.65, (n, 2))
    return np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)


def setup(seed, nstand, nsrc, nfine, flagged=(3,), f0=50e6, extent=1200.0):
    """(rng, tau [nsrc][nstand], freq [nfine], flux f32 [nfine][nsrc] between 1 and 10 falling with the source's number, w f32
    [nstand] between 0.5 and 2 with the `flagged` stands at 0, true gains complex128 [nfine][2][nstand] of amplitude 0.5 to 2 and
    any phase): an array of `extent` metres, so that phases reach hundreds of turns."""
    rng = np.random.default_rng(seed)
    tau = steering_delays(random_array(rng, nstand, extent, 5.0), sky(rng, nsrc))
    freq = f0 + FINE_BW * np.arange(nfine)
    flux = (rng.uniform(1.0, 10.0, (nfine, nsrc)) / (1 + np.arange(nsrc))).astype(np.float32)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[list(flagged)] = 0
    g = rng.uniform(0.5, 2.0, (nfine, 2, nstand)) * np.exp(2j * np.pi * rng.uniform(size=(nfine, 2, nstand)))
    return rng, tau, freq, flux, w, g


def corrupt(M, g):
    """V = g g^H o M on both polarisations and zeros in the cross-hands: complex64 [nfine][nstand][2][nstand][2], Hermitian bit for
    bit (the upper triangle is the conjugate of the lower)."""
    nfine, nstand = M.shape[:2]
    V = np.zeros((nfine, nstand, 2, nstand, 2), np.complex64)
    low = np.tril(np.ones((nstand, nstand), bool), -1)
    for p in range(2):
        B = (g[:, p, :, None] * np.conj(g[:, p, None, :]) * M).astype(np.complex64)
        B = np.where(low[None], B, 0)
        V[:, :, p, :, p] = B + np.conj(B.transpose(0, 2, 1)) + np.einsum('cs,st->cst', (np.abs(g[:, p]) ** 2 * M[:, 0, 0, None].real).astype(np.float32),
                                                                         np.eye(nstand, dtype=np.float32))
    return V


def noisy(rng, V, level):
    """V plus `level` times Hermitian noise of uneven rows (tests/image_ref.py hermitian_uneven), Hermitian bit for bit."""
    nfine, nstand = V.shape[:2]
    return (V + np.float32(level) * hermitian_uneven(rng, nfine, nstand, 0.5, 5.0)).astype(np.complex64)


def model(freq, tau, flux):
    return model_visibilities(freq, tau, flux)
