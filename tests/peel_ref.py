"""The contract of xengPeel* (include/xeng.h, "Direction-dependent gains and peeling") restated in numpy by the contract's own route
(one pass over V per sweep for all directions, then the directions in ascending order, each against the new gains of those before it
and the old gains of those behind it): float64 by default, complex64 with a dtype argument (the gap between the two on a test's own
inputs is a fifth of that test's bar); the subtraction; a textbook dense form of one sweep to compare with; the error measures;
generators of cases on tests/gaincal_ref.py's arrays and skies and tests/image_ref.py's noise."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks.calibration import direction_model_visibilities, model_flux
from caltech_bifrost_dsp_amd.blocks.imaging import steering_delays
from tests.gaincal_ref import FINE_BW, gain_error, read_block, sky, steering
from tests.image_ref import hermitian_uneven, random_array


def _real(dtype):
    return np.float32 if np.dtype(dtype) == np.complex64 else np.float64


def sweep(X, a, F, w, g, dtype=np.complex128):
    """One sweep of the contract on one (channel, pol): X [nstand][nstand] as read_block gives it, a [ndir][nstand] (0 at the stands
    of weight 0), F [ndir], w [nstand], g [ndir][nstand] the gains at the start; returns g' [ndir][nstand], every step in `dtype`."""
    real = _real(dtype)
    live = w != 0
    u = (g * a).astype(dtype)
    Y = ((w * u) @ X.T).astype(dtype)                                        # Y[d][s] = sum_{t != s} X[s][t] w_t u_dt
    ut = u.copy()
    new = np.zeros_like(u)
    for d in range(len(F)):
        if not F[d] > 0:
            continue
        ud = u[d]
        G = (w * np.conj(ut)) @ ud                                           # G[e] = sum_t w_t conj(u~_et) u_dt
        q = w * (ud.real ** 2 + ud.imag ** 2)
        P = q.sum(dtype=real)
        N = Y[d].copy()
        for e in range(len(F)):
            if e != d:
                N -= F[e] * ut[e] * (G[e] - w * np.conj(ut[e]) * ud)
        den = F[d] * (P - q)
        assert N.dtype == dtype and den.dtype == real
        ok = live & (den > 0)
        new[d] = np.where(ok, np.conj(a[d]) * N / np.where(ok, den, 1), 0)
        ut[d] = new[d] * a[d]
    return new.astype(dtype)


def solve(V, freq, tau, flux, w, refant, niter, tol, dtype=np.complex128, start=None, trace=None):
    """(gains [nfine][2][ndir][nstand] after the phase reference, stats f64 [nfine][2][4] = {sweeps, last delta (-1: none), stands
    solved, converged}, keep): the contract, every step in `dtype`'s precision.  `start` is the `keep` of an earlier call
    (unreferenced gains [nfine][2][ndir][nstand], converged and finite [nfine][2]): the warm start.  A list `trace` receives
    (c, p, sweep, delta) of every delta formed."""
    dtype = np.dtype(dtype)
    real = _real(dtype)
    nfine, nstand = V.shape[:2]
    ndir = np.shape(tau)[0]
    Fall = model_flux(flux, nfine, ndir).astype(real)
    w = np.asarray(w).astype(real)
    live = w != 0
    a_all = steering(freq, tau, dtype)
    gains = np.zeros((nfine, 2, ndir, nstand), dtype)
    stats = np.zeros((nfine, 2, 4))
    keep_g = np.zeros((nfine, 2, ndir, nstand), dtype) if start is None else np.array(start[0], dtype)
    keep_ok = np.zeros((nfine, 2), bool) if start is None else np.array(start[1], bool)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for c in range(nfine):
            a = np.where(live[None], a_all[c], 0).astype(dtype)
            F = Fall[c]
            on = (F > 0)[:, None] & live[None]                               # the live (direction, stand)
            for p in range(2):
                X = read_block(V, w, c, p).astype(dtype)
                g = np.where(on, keep_g[c, p] if start is not None and keep_ok[c, p] else 1, 0).astype(dtype)
                it, conv, delta = 0, False, -1.0
                while it < niter and not conv:
                    new = sweep(X, a, F, w, g, dtype)
                    it += 1
                    if it % 2 == 0:
                        delta = float(np.sqrt((np.abs(new - g)[on] ** 2).sum(dtype=real) / (np.abs(new)[on] ** 2).sum(dtype=real)))
                        if trace is not None:
                            trace.append((c, p, it, delta))
                        if tol > 0 and delta <= real(tol):
                            conv = True
                        else:
                            new = ((new + g) * real(0.5)).astype(dtype)
                    g = new
                mag = np.abs(g[:, refant])
                ph = np.where(mag > 0, np.conj(g[:, refant]) / np.where(mag > 0, mag, 1), 1).astype(dtype)
                gains[c, p] = g * ph[:, None]
                solved = np.count_nonzero(live & np.all((g != 0) | ~on, axis=0)) if (F > 0).any() else 0
                stats[c, p] = (it, delta, solved, conv)
                if niter > 0:
                    keep_g[c, p], keep_ok[c, p] = g, conv and bool(np.all(np.isfinite(g)))
    return gains, stats, (keep_g, keep_ok)


def subtract(V, freq, tau, flux, gains, dtype=np.complex128):
    """out in V's layout, `dtype`: on the parallel hands V - sum_d (F_d u_ds) conj(u_dt) with u = g a, of the lower triangle; the
    diagonal's real part and +0; the upper triangle the conjugate of the lower; the cross hands the input's (of the lower triangle,
    mirrored).  Only the words i >= j of V are looked at."""
    dtype = np.dtype(dtype)
    real = _real(dtype)
    V = np.asarray(V)
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    F = model_flux(flux, nfine, np.shape(tau)[0]).astype(real)
    u = (np.asarray(gains).astype(dtype) * steering(freq, tau, dtype)[:, None]).astype(dtype)      # [c][p][d][s]
    Y = np.where(np.tril(np.ones((n, n), bool))[None], V.reshape(nfine, n, n), 0).astype(dtype).reshape(nfine, nstand, 2, nstand, 2)
    with np.errstate(invalid='ignore', over='ignore'):
        for p in range(2):
            M = np.einsum('cds,cdt->cst', (F[:, :, None] * u[:, p]).astype(dtype), np.conj(u[:, p]))
            assert M.dtype == dtype
            Y[:, :, p, :, p] -= M
    Y = Y.reshape(nfine, n, n)
    out = np.where(np.tril(np.ones((n, n), bool), -1)[None], Y, np.conj(Y.transpose(0, 2, 1)))      # (a select: the sign of a zero is turned too)
    out[:, np.arange(n), np.arange(n)] = np.einsum('cii->ci', Y).real
    return out.reshape(nfine, nstand, 2, nstand, 2)


def peel(V, freq, tau, flux, w, refant, niter, tol, dtype=np.complex128, start=None):
    """(out, gains, stats, keep) of one Run"""
    gains, stats, keep = solve(V, freq, tau, flux, w, refant, niter, tol, dtype, start)
    return subtract(V, freq, tau, flux, gains, dtype), gains, stats, keep


def textbook_sweep(V, c, p, freq, tau, flux, w, g):
    """One sweep in float64 the dense way: per direction d the residual R_d = V - sum_{e != d} F_e u~_e u~_e^H is formed as a matrix
    and one StEFCal step against F_d a_d a_d^H is done on it: g'_ds = sum_{t != s} w_t R_d[s][t] g_dt M[t][s] / sum_{t != s} w_t |g_dt
    M[t][s]|^2.  g [ndir][nstand] -> g' [ndir][nstand]."""
    w = np.asarray(w, np.float64)
    live = w != 0
    ndir, nstand = np.shape(tau)
    F = model_flux(flux, V.shape[0], ndir)[c]
    a = np.where(live[None], steering(freq, tau)[c], 0)
    X = read_block(V, w, c, p).astype(np.complex128)
    off = ~np.eye(nstand, dtype=bool)
    cur = np.array(g, np.complex128)
    new = np.zeros_like(cur)
    for d in range(ndir):
        if not F[d] > 0:
            continue
        R = X.copy()
        for e in range(ndir):
            if e != d:
                ue = cur[e] * a[e]
                R -= F[e] * np.outer(ue, np.conj(ue))
        R = np.where(off, R, 0)
        M = F[d] * np.outer(a[d], np.conj(a[d]))                             # M[t][s]
        Z = (w * g[d])[:, None] * M                                          # Z[t][s] = w_t g_dt M[t][s]
        N = np.einsum('st,ts->s', R, Z)
        D = np.einsum('t,ts->s', w * np.abs(g[d]) ** 2, np.abs(M) ** 2 * off)
        new[d] = np.where(live & (D > 0), N / np.where(D > 0, D, 1), 0)
        cur[d] = new[d]
    return new


def dir_gain_error(got, ref):
    """max_s |g - g_ref| / rms_s |g_ref| per (channel, pol, direction): f64 [nfine][2][ndir]; 0 where the reference is all zeros and
    so is the difference"""
    ref = np.asarray(ref, np.complex128)
    d = np.abs(np.asarray(got, np.complex128) - ref).max(axis=-1)
    rms = np.sqrt((np.abs(ref) ** 2).mean(axis=-1))
    return np.where(rms > 0, d / np.where(rms > 0, rms, 1), np.where(d > 0, np.inf, 0.0))


def out_error(got, ref, V):
    """max |out - out_ref| / rms |V| per (channel, pol) over the pp block: f64 [nfine][2] (the rms over V's finite words)"""
    err = np.zeros((V.shape[0], 2))
    for p in range(2):
        A = np.asarray(V[:, :, p, :, p], np.complex128)
        fin = np.isfinite(A)
        rms = np.sqrt((np.abs(np.where(fin, A, 0)) ** 2).sum(axis=(1, 2)) / fin.sum(axis=(1, 2)))
        d = np.abs(np.asarray(got[:, :, p, :, p], np.complex128) - np.asarray(ref[:, :, p, :, p], np.complex128))
        err[:, p] = np.where(np.isfinite(d), d, 0).max(axis=(1, 2)) / rms if np.isfinite(d).any() else np.inf
        err[:, p] = np.where(np.isfinite(d).all(axis=(1, 2)), err[:, p], np.inf)
    return err


def float_gap(V, freq, tau, flux, w, refant, niter, tol=0.0, ref=None):
    """(gain gap, output gap): the worst dir_gain_error and out_error of the complex64 evaluation against the float64 one, each a
    fifth of its float bar."""
    ref = peel(V, freq, tau, flux, w, refant, niter, tol) if ref is None else ref
    got = peel(V, freq, tau, flux, w, refant, niter, tol, np.complex64)
    return float(dir_gain_error(got[1], ref[1]).max()), float(out_error(got[0], ref[0], V).max())


def pack(Mpp, rng=None, noise=0.0):
    """Visibilities complex64 [nfine][nstand][2][nstand][2] with the parallel hands Mpp [nfine][2][nstand][nstand] (rounded once, the
    lower triangle mirrored, so Hermitian bit for bit, the diagonal real) plus `noise` times Hermitian noise of uneven rows
    (tests/image_ref.py hermitian_uneven), cross hands included."""
    nfine, _, nstand, _ = Mpp.shape
    V = np.zeros((nfine, nstand, 2, nstand, 2), np.complex64)
    low = np.tril(np.ones((nstand, nstand), bool), -1)
    for p in range(2):
        B = np.where(low[None], Mpp[:, p].astype(np.complex64), 0)
        V[:, :, p, :, p] = B + np.conj(B.transpose(0, 2, 1)) + np.einsum('cs,st->cst', np.einsum('css->cs', Mpp[:, p]).real.astype(np.float32),
                                                                         np.eye(nstand, dtype=np.float32))
    if noise:
        V = (V + np.float32(noise) * hermitian_uneven(rng, nfine, nstand, 0.5, 5.0)).astype(np.complex64)
    # the upper triangle as the correlator writes it: the lower one's words with the sign of the imaginary part turned, zeros included
    n = 2 * nstand
    A = V.reshape(nfine, n, n)
    A = np.where(np.tril(np.ones((n, n), bool), -1)[None], A, np.conj(A.transpose(0, 2, 1)))
    A[:, np.arange(n), np.arange(n)] = np.einsum('cii->ci', V.reshape(nfine, n, n)).real
    return np.ascontiguousarray(A.astype(np.complex64)).reshape(nfine, nstand, 2, nstand, 2)


def case(nstand, ndir, nfine, noise=0.0, seed=None, flagged=(3,), nback=6, f0=50e6, extent=1200.0):
    """(tau [ndir][nstand], freq [nfine], flux f32 [nfine][ndir], w f32 [nstand], g complex128 [nfine][2][ndir][nstand], V): data as
    they are behind UpchanCalApply.  An array of `extent` metres; `ndir` bright sources of fluxes 100 falling to 10 with gains of
    amplitude 1 +- 0.2 and a phase of sigma 0.5 rad per direction and stand; `nback` background sources of flux 0.3 to 3 with unit
    gains that the model does not know; weights between 0.5 and 2, 0 at the `flagged` stands; `noise` times Hermitian noise."""
    rng = np.random.default_rng(300 + nstand + 7 * ndir if seed is None else seed)
    pos = random_array(rng, nstand, extent, 5.0)
    tau = steering_delays(pos, sky(rng, ndir))
    freq = f0 + FINE_BW * np.arange(nfine)
    flux = (np.geomspace(100.0, 10.0, ndir) if ndir > 1 else np.array([100.0]))[None] * rng.uniform(0.9, 1.1, (nfine, ndir))
    flux = flux.astype(np.float32)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[list(flagged)] = 0
    g = rng.uniform(0.8, 1.2, (nfine, 2, ndir, nstand)) * np.exp(1j * rng.normal(0.0, 0.5, (nfine, 2, ndir, nstand)))
    M = direction_model_visibilities(freq, tau, flux, g)
    if nback:
        btau = steering_delays(pos, sky(rng, nback))
        M = M + direction_model_visibilities(freq, btau, rng.uniform(0.3, 3.0, nback), np.ones((nfine, nback, nstand)))[:, None]
    return tau, freq, flux, w, g, pack(M, rng, noise)


def hermitian_nan(V, stand):
    """V with NaN and Inf all over the rows and columns of `stand`, the cross hands included, still Hermitian bit for bit: the lower
    triangle's words are set, the upper triangle's are their conjugates, the diagonal's imaginary words stay +0."""
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    A = V.reshape(nfine, n, n).copy()
    hit = np.zeros(n, bool)
    hit[2 * stand:2 * stand + 2] = True
    low = np.tril(np.ones((n, n), bool), -1)
    A[:, low & hit[:, None]] = np.complex64(complex(np.nan, np.inf))
    A[:, low & hit[None, :]] = np.complex64(complex(-np.inf, np.nan))
    L = np.where(low[None], A, 0)
    D = np.einsum('cii->ci', A).real.copy()
    D[:, hit] = np.nan
    up = np.conj(L.transpose(0, 2, 1))
    A = np.where(low[None], A, up)
    A[:, np.arange(n), np.arange(n)] = D
    return np.ascontiguousarray(A.astype(np.complex64)).reshape(V.shape)
