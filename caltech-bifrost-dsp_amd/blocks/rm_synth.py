"""Host side of the Faraday rotation-measure synthesis (BeamRmSynth, xengRmsynth*): everything the library does not know -- the
wavelengths, the depth grid, the rotation table -- and what a caller does with a spectrum, in float64.

The linear polarisation P = Q + iU of a source behind a Faraday screen of rotation measure RM turns by 2 RM lambda^2 across the
band.  RM synthesis (Brentjens & de Bruyn 2005) sums P over the channels with the turn of a trial depth phi taken out,
  F(phi) = sum_g w_g P_g exp(-2i phi (lambda_g^2 - lambda_0^2)) ,
and |F|^2 peaks at phi = RM.  lambda_0^2 is the weighted mean of lambda^2: it takes the steepest phase gradient out of F(phi).
The library forms F per phase bin from a table T[g][k] = w_g (cos theta, sin theta), theta = 2 phi_k (lambda_g^2 - lambda_0^2), sums
|F|^2 over the on-pulse bins, and picks the peak (include/xeng.h, "Faraday rotation-measure synthesis of folded profiles")."""
import numpy as np

C_M_S = 299792458.0
RM_RECORD = np.dtype([('k', '<i4'), ('peak', '<f4'), ('n_on', '<i4'), ('n_off', '<i4')])
FEEDS = {'linear': 0, 'circular': 1}
MAX_NPHI = 4096


def rm_lambda2(freqs_hz):
    """lambda^2 in m^2 at the given frequencies in Hz."""
    f = np.asarray(freqs_hz, np.float64)
    if f.size == 0 or not np.all(np.isfinite(f)) or f.min() <= 0:
        raise ValueError("rm_lambda2: the frequencies must be finite and positive")
    return (C_M_S / f) ** 2


def rm_plan(freqs_hz, chan_bw_hz, phi_max, oversample=4):
    """The depth grid for channels of width chan_bw_hz centred at freqs_hz: dict(fwhm, dphi, nphi, phis, phi_max_chan, max_scale,
    span): fwhm = 3.8 / span of the RMSF, span the extent of the band in lambda^2 (edge to edge); dphi = fwhm / oversample; the grid
    phis = dphi (k - nphi div 2), nphi odd, reaches phi_max; phi_max_chan = sqrt(3) / (the widest channel in lambda^2), the largest
    |phi| a channel's own width lets through at half sensitivity; max_scale = pi / min lambda^2, the largest Faraday-thick scale."""
    f = np.asarray(freqs_hz, np.float64).reshape(-1)
    if not np.isfinite(chan_bw_hz) or chan_bw_hz <= 0 or f.min() - chan_bw_hz / 2 <= 0:
        raise ValueError("rm_plan: the channel width must be positive and every channel above 0 Hz")
    if not np.isfinite(phi_max) or phi_max <= 0 or not oversample >= 1:
        raise ValueError("rm_plan: phi_max must be positive and oversample at least 1")
    lo, hi = rm_lambda2(f + chan_bw_hz / 2), rm_lambda2(f - chan_bw_hz / 2)
    span = float(hi.max() - lo.min())
    fwhm = 3.8 / span
    dphi = fwhm / oversample
    half = int(np.ceil(phi_max / dphi))
    nphi = 2 * half + 1
    if nphi > MAX_NPHI:
        raise ValueError("rm_plan: %d depths of %g rad/m^2 to reach %g; the library takes %d" % (nphi, dphi, phi_max, MAX_NPHI))
    return dict(fwhm=fwhm, dphi=dphi, nphi=nphi, phis=dphi * (np.arange(nphi) - half), phi_max_chan=float(np.sqrt(3.0) / (hi - lo).max()),
                max_scale=float(np.pi / lo.min()), span=span)


def _weights(weights, n):
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if w.size != n or not np.all(np.isfinite(w)):
        raise ValueError("the weights must be %d finite numbers" % n)
    return w


def rm_table(freqs_hz, phis, weights=None):
    """(T float32 [nchg][nphi][2], w float32 [nchg], use uint8 [nchg], lambda0_sq): T[g][k] = w_g (cos theta, sin theta) with
    theta = 2 phi_k (lambda_g^2 - lambda_0^2), lambda_0^2 the mean of lambda^2 under |w|; evaluated in float64 and each word rounded
    once to float32 (chirp_table's rule).  A channel of weight 0 has use = 0."""
    lam2 = rm_lambda2(freqs_hz).reshape(-1)
    phis = np.asarray(phis, np.float64).reshape(-1)
    if phis.size == 0 or phis.size > MAX_NPHI or not np.all(np.isfinite(phis)):
        raise ValueError("rm_table: 1 to %d finite depths" % MAX_NPHI)
    w = _weights(weights, lam2.size)
    use = (w != 0).astype(np.uint8)
    if not use.any():
        raise ValueError("rm_table: every channel has weight 0")
    lambda0_sq = float(np.sum(np.abs(w) * lam2) / np.sum(np.abs(w)))
    theta = 2.0 * phis[None, :] * (lam2[:, None] - lambda0_sq)
    T = np.stack([w[:, None] * np.cos(theta), w[:, None] * np.sin(theta)], axis=-1)
    return np.ascontiguousarray(T, np.float32), w.astype(np.float32), use, lambda0_sq


def rmsf(freqs_hz, phis, weights=None):
    """The rotation-measure spread function R(phi) = sum_g w_g exp(-2i phi (lambda_g^2 - lambda_0^2)) / sum_g w_g, complex128
    [nphi]: 1 at phi = 0."""
    lam2 = rm_lambda2(freqs_hz).reshape(-1)
    w = _weights(weights, lam2.size)
    lambda0_sq = np.sum(np.abs(w) * lam2) / np.sum(np.abs(w))
    phis = np.asarray(phis, np.float64).reshape(-1)
    return (w[None, :] * np.exp(-2j * phis[:, None] * (lam2[None, :] - lambda0_sq))).sum(1) / w.sum()


def rm_refine(spec, phis, k=None):
    """(phi, peak) of the parabola through the spectrum's three words around k (the arg-max if None); at an edge, or where the
    three words do not bend down, the grid's own (phis[k], spec[k])."""
    spec, phis = np.asarray(spec, np.float64), np.asarray(phis, np.float64)
    k = int(np.nanargmax(spec)) if k is None else int(k)
    if k <= 0 or k >= spec.size - 1:
        return float(phis[k]), float(spec[k])
    a, b, c = spec[k - 1], spec[k], spec[k + 1]
    bend = a - 2 * b + c
    if not np.isfinite(bend) or not bend < 0:
        return float(phis[k]), float(b)
    d = 0.5 * (a - c) / bend
    return float(phis[k] + d * (phis[k + 1] - phis[k - 1]) / 2), float(b - 0.25 * (a - c) * d)


def rm_significance(spec):
    """(snr, median, mad): the peak above the spectrum's median in units of 1.4826 MAD over depth (inf over a flat spectrum)."""
    s = np.asarray(spec, np.float64)
    med = float(np.median(s))
    mad = float(np.median(np.abs(s - med)))
    top = float(s.max()) - med
    return (top / (1.4826 * mad) if mad > 0 else (np.inf if top > 0 else 0.0)), med, mad


def rm_error(fwhm, snr):
    """The 1-sigma error of a depth read off a peak of signal-to-noise snr in |F|: fwhm / (2 snr)."""
    return float(fwhm) / (2.0 * float(snr)) if snr > 0 else np.inf


def pol_profile(prof):
    """dict(I, Q, U, V, L, PA, frac_L, frac_V) of a profile [4][nbin] = I, Q, U, V: L = |Q + iU|, PA = atan2(U, Q) / 2 in radians,
    the fractions NaN where I is not positive.  (L is not de-biased.)"""
    I, Q, U, V = (np.asarray(prof[s], np.float64) for s in range(4))
    L = np.hypot(Q, U)
    with np.errstate(divide='ignore', invalid='ignore'):
        fl, fv = np.where(I > 0, L / I, np.nan), np.where(I > 0, V / I, np.nan)
    return dict(I=I, Q=Q, U=U, V=V, L=L, PA=0.5 * np.arctan2(U, Q), frac_L=fl, frac_V=fv)


def rm_offsets(npair, nphi, nbin):
    """(byte offset of spec, of the profile, bytes of the span) behind the npair records of 16 bytes."""
    a = 16 * npair
    b = a + 4 * npair * nphi
    return a, b, b + 16 * npair * nbin


def as_rmsynth(span, npair, nphi, nbin):
    """(records [npair] RM_RECORD, spec f32 [npair][nphi], profile f32 [npair][4][nbin]): views of one output span."""
    a, b, n = rm_offsets(npair, nphi, nbin)
    span = np.ascontiguousarray(span).reshape(-1).view(np.uint8)
    if span.size != n:
        raise ValueError("as_rmsynth: %d bytes, %d expected" % (span.size, n))
    return span[:a].view(RM_RECORD), span[a:b].view(np.float32).reshape(npair, nphi), span[b:].view(np.float32).reshape(npair, 4, nbin)


def rm_reference(X, T, w=None, use=None, off=None, on=None, active=None, feeds=0):
    """The float64 statement of the contract: X [npair][4][nchg][nbin], T [nchg][nphi][2].  dict(k [npair], peak, spec
    [npair][nphi], prof [npair][4][nbin], F complex [npair][nbin][nphi], scale [npair][nbin][nphi] = sum_g (|y_q| + |y_u|)(|Tc| +
    |Ts|), the scale of a rounding-error bound, nused).  No order of summation is stated: that is the library's."""
    X, T = np.asarray(X, np.float64), np.asarray(T, np.float64)
    npair, _, nchg, nbin = X.shape
    nphi = T.shape[1]
    w = np.ones(nchg) if w is None else np.asarray(w, np.float64)
    use = np.ones(nchg, bool) if use is None else np.asarray(use) != 0
    off = np.ones((npair, nbin), bool) if off is None else np.asarray(off) != 0
    on = np.ones((npair, nbin), bool) if on is None else np.asarray(on) != 0
    active = np.ones(npair, bool) if active is None else np.asarray(active) != 0
    out = dict(k=np.full(npair, -1), peak=np.zeros(npair), spec=np.zeros((npair, nphi)), prof=np.zeros((npair, 4, nbin)),
               F=np.zeros((npair, nbin, nphi), np.complex128), scale=np.zeros((npair, nbin, nphi)), nused=int(use.sum()))
    Tc, Ts = T[use, :, 0], T[use, :, 1]
    for p in range(npair):
        if not active[p]:
            continue
        x0, x1, x2, x3 = (X[p, s][use] for s in range(4))
        i, q, u, v = (x0 + x1, 2 * x2, 2 * x3, x0 - x1) if feeds else (x0 + x1, x0 - x1, 2 * x2, 2 * x3)
        y = [s - (s[:, off[p]].mean(1, keepdims=True) if off[p].any() else 0.0) for s in (i, q, u, v)]
        F = (y[1] + 1j * y[2]).T @ (Tc - 1j * Ts)                   # [nbin][nphi]
        out['F'][p] = F
        out['scale'][p] = (np.abs(y[1]) + np.abs(y[2])).T @ (np.abs(Tc) + np.abs(Ts))
        out['spec'][p] = (np.abs(F[on[p]]) ** 2).sum(0)
        out['prof'][p, 0], out['prof'][p, 3] = w[use] @ y[0], w[use] @ y[3]
        if on[p].any() and not np.all(np.isnan(out['spec'][p])):
            k = int(np.nanargmax(out['spec'][p]))
            out['k'][p], out['peak'][p] = k, out['spec'][p, k]
            out['prof'][p, 1], out['prof'][p, 2] = F[:, k].real, F[:, k].imag
    return out
