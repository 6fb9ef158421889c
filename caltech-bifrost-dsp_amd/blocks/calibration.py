"""Host side of UpchanGainCal: the dense sky model, and what a caller does with a gain solution, all float64.

The solver (xengGaincal*, include/xeng.h) fits, per fine channel and polarisation, V[s][t] = g_s conj(g_t) M[s][t] with the
point-source model M[s][t] = sum_k F_k a_ks conj(a_kt), a_ks = exp(-2 pi i f tau_s(k)) -- tau from imaging.steering_delays of the
sources' directions, the convention under which a unit source images to 1 with UpchanImage.  Gains are complex [nfine][2][nstand];
a gain of 0 marks a stand without a solution (flagged, or cut off from every other stand)."""
import numpy as np


def model_visibilities(freq, tau, flux):
    """The model M complex128 [nfine][nstand][nstand] of freq [nfine] Hz, tau [nsrc][nstand] seconds (steering_delays of the
    sources) and flux [nsrc] or [nfine][nsrc] >= 0.  Dense: nstand^2 words per channel (the solver never forms it)."""
    freq = np.asarray(freq, np.float64).reshape(-1)
    tau = np.asarray(tau, np.float64)
    if tau.ndim != 2 or not tau.size or not freq.size:
        raise ValueError("model_visibilities: freq [nfine] and tau [nsrc][nstand], got %r and %r" % (freq.shape, tau.shape))
    F = model_flux(flux, len(freq), tau.shape[0])
    turns = freq[:, None, None] * tau[None]
    a = np.exp(-2j * np.pi * (turns - np.rint(turns)))                      # [nfine][nsrc][nstand]
    return np.einsum('ck,cks,ckt->cst', F, a, np.conj(a))


def model_flux(flux, nfine, nsrc):
    """flux [nsrc] or [nfine][nsrc], finite and >= 0, as float64 [nfine][nsrc]; else ValueError."""
    try:
        F = np.asarray(flux, np.float64)
    except (TypeError, ValueError):
        F = np.zeros(0)
    if F.shape == (nsrc,):
        F = np.broadcast_to(F, (nfine, nsrc))
    if F.shape != (nfine, nsrc) or not np.all(np.isfinite(F)) or F.min() < 0:
        raise ValueError("model_flux: the fluxes must be [%d] or [%d][%d] finite numbers >= 0" % (nsrc, nfine, nsrc))
    return np.ascontiguousarray(F)


MAX_NSRC, MAX_NSTAND = 32, 512          # include/xeng.h XENG_GAINCAL_MAX_* and XENG_CALAPPLY_MAX_*


def checked_flux(who, flux, nsrc, nfine=None, quiet=False):
    """The fluxes of a block's `nsrc` > 0 sources, float64 [nsrc] or [nfine][nsrc], finite and >= 0 (`nfine`: of the sequence being
    read, None before the first); else ValueError, or None if `quiet`."""
    try:
        F = np.asarray(flux, np.float64)
        ok = nsrc > 0 and F.ndim in (1, 2) and F.shape[-1] == nsrc and F.size > 0 and bool(np.all(np.isfinite(F))) and bool(F.min() >= 0)
        if ok and F.ndim == 2 and nfine is not None:
            ok = F.shape[0] == nfine
    except (TypeError, ValueError):
        F, ok = None, False
    if ok:
        return F
    if quiet:
        return None
    raise ValueError("%s: the fluxes must be [%d] or [nfine][%d] finite numbers >= 0" % (who, nsrc, nsrc))


def _gains(g, V=None):
    g = np.asarray(g, np.complex128)
    if g.ndim != 3 or g.shape[1] != 2 or (V is not None and (V.ndim != 5 or V.shape != (g.shape[0], g.shape[2], 2, g.shape[2], 2))):
        raise ValueError("gains [nfine][2][nstand]%s, got %r%s" % ("" if V is None else " and visibilities [nfine][nstand][2][nstand][2]", g.shape,
                                                                  "" if V is None else " and %r" % (V.shape,)))
    return g


def inverse_gains(g):
    """1 / g per input, complex128 [nfine][2 nstand] with input 2 s + p, and 0 where g = 0: the factor a caller folds into the
    weights of Beamform or UpchanBeamform (w'[c][b][i] = w[c][b][i] * inverse_gains(g)[c][i]) so that the beams are formed from
    calibrated voltages and an unsolved stand drops out."""
    g = _gains(g)
    ok = g != 0
    inv = np.where(ok, 1.0 / np.where(ok, g, 1.0), 0.0)
    return np.ascontiguousarray(inv.transpose(0, 2, 1).reshape(g.shape[0], -1))


def apply_gains(V, g):
    """The calibrated visibilities V[c][s p][t q] / (g_ps conj(g_qt)), complex128 in V's layout [nfine][nstand][2][nstand][2]; the
    rows and columns of a stand whose gain is 0 are zeros, whatever they held."""
    V = np.asarray(V)
    g = _gains(g, V)
    inv = inverse_gains(g).reshape(g.shape[0], g.shape[2], 2)               # [c][s][p]
    keep = inv != 0
    both = keep[:, :, :, None, None] & keep[:, None, None, :, :]
    return np.where(both, np.where(both, V, 0) * inv[:, :, :, None, None] * np.conj(inv)[:, None, None, :, :], 0)


def reference_phase(g, refant):
    """g * conj(g_ref) / |g_ref| per (channel, pol): the reference stand's gain becomes real and positive.  Left as it is where
    g_ref = 0."""
    g = _gains(g)
    if isinstance(refant, bool) or int(refant) != refant or not 0 <= refant < g.shape[2]:
        raise ValueError("reference_phase: stand %r of %d" % (refant, g.shape[2]))
    ref = g[:, :, int(refant)]
    mag = np.abs(ref)
    ph = np.where(mag > 0, np.conj(ref) / np.where(mag > 0, mag, 1.0), 1.0)
    return g * ph[:, :, None]


MAX_NDIR = 8                            # include/xeng.h XENG_PEEL_MAX_NDIR


def direction_model_visibilities(freq, tau, flux, g):
    """The sky of UpchanPeel's model with a gain set per direction: sum_d F_d (g_d o a_d)(g_d o a_d)^H, complex128, of freq [nfine]
    Hz, tau [ndir][nstand] seconds, flux [ndir] or [nfine][ndir] >= 0 and gains g [nfine][ndir][nstand] (the result is
    [nfine][nstand][nstand]) or [nfine][2][ndir][nstand] (one per polarisation: [nfine][2][nstand][nstand]).  Dense, as
    model_visibilities is, which it equals at g = 1."""
    freq = np.asarray(freq, np.float64).reshape(-1)
    tau = np.asarray(tau, np.float64)
    g = np.asarray(g, np.complex128)
    if tau.ndim != 2 or not tau.size or not freq.size:
        raise ValueError("direction_model_visibilities: freq [nfine] and tau [ndir][nstand], got %r and %r" % (freq.shape, tau.shape))
    if g.ndim not in (3, 4) or g.shape[0] != len(freq) or g.shape[-2:] != tau.shape or (g.ndim == 4 and g.shape[1] != 2):
        raise ValueError("direction_model_visibilities: gains [nfine][ndir][nstand] or [nfine][2][ndir][nstand], got %r" % (g.shape,))
    F = model_flux(flux, len(freq), tau.shape[0])
    turns = freq[:, None, None] * tau[None]
    a = np.exp(-2j * np.pi * (turns - np.rint(turns)))                      # [nfine][ndir][nstand]
    if g.ndim == 3:
        u = g * a
        return np.einsum('cd,cds,cdt->cst', F, u, np.conj(u))
    u = g * a[:, None]
    return np.einsum('cd,cpds,cpdt->cpst', F, u, np.conj(u))
