"""Host side of the template-matched arrival phases (BeamToa, xengToa*): everything the library does not know -- the sub-bands, the
sine and cosine tables, the templates' harmonics -- and what a caller does with its output in float64: the sub-lag refinement
(Taylor's FFTFIT), the DM fit over the sub-bands and the conversion of a phase to a time.

A folded profile p that is a template s delayed by tau turns, p(b) = a + b_amp s(b - tau nbin) + noise, has the harmonics
P_k = b_amp S_k exp(-2 pi i k tau) (k >= 1; P_k = sum_b p_b exp(-2 pi i k b / nbin)).  The library forms P_k for k = 1 .. nharm, the
cross-spectrum C_k = P_k conj(S_k) and its transform onto a grid of lags, ccf[l] = sum_k Re(C_k exp(+2 pi i k l / nlag)), which
peaks at l / nlag = tau, and picks the peak (include/xeng.h, "Template-matched arrival phases of folded profiles").  toa_refine
finds tau between the grid's lags.

References: J. H. Taylor 1992, Phil. Trans. R. Soc. A 341, 117 (appendix A: FFTFIT)."""
from fractions import Fraction

import numpy as np

from .dedisp import KDM

TOA_RECORD = np.dtype([('l', '<i4'), ('peak', '<f4'), ('base', '<f4'), ('var', '<f4')])
MAX_NBIN = 16384
MAX_NHARM = 4096
MAX_NLAG = 65536
MAX_NSUB = 256
MAX_TABLE_BYTES = 1 << 30
REFINE_ITERATIONS = 64


def _count(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def toa_offsets(npair, nsub, nbin, nharm, nlag):
    """(byte offset of P, of PH, of ccf, bytes of the span) behind the npair (nsub + 1) records of 16 bytes."""
    nrow = npair * (nsub + 1)
    a = 16 * nrow
    b = a + 4 * nrow * nbin
    c = b + 8 * nrow * nharm
    return a, b, c, c + 4 * nrow * nlag


def as_toa(span, npair, nsub, nbin, nharm, nlag):
    """(records [npair][nsub+1] TOA_RECORD, P f32 [npair][nsub+1][nbin], PH f32 [npair][nsub+1][nharm][2], ccf f32
    [npair][nsub+1][nlag]): views of one output span.  Row nsub is the whole band."""
    a, b, c, n = toa_offsets(npair, nsub, nbin, nharm, nlag)
    span = np.ascontiguousarray(span).reshape(-1).view(np.uint8)
    if span.size != n:
        raise ValueError("as_toa: %d bytes, %d expected" % (span.size, n))
    return (span[:a].view(TOA_RECORD).reshape(npair, nsub + 1), span[a:b].view(np.float32).reshape(npair, nsub + 1, nbin),
            span[b:c].view(np.float32).reshape(npair, nsub + 1, nharm, 2), span[c:].view(np.float32).reshape(npair, nsub + 1, nlag))


def toa_subbands(nchg, nsub):
    """int32 [nsub + 1]: the edges of nsub contiguous sub-bands of near-equal size over nchg groups, edges[r] = (r nchg) div nsub."""
    if not _count(nchg) or not _count(nsub) or not 1 <= nsub <= min(nchg, MAX_NSUB):
        raise ValueError("toa_subbands: %r sub-bands of %r groups (1 to min(nchg, %d))" % (nsub, nchg, MAX_NSUB))
    return np.array([(r * int(nchg)) // int(nsub) for r in range(nsub + 1)], np.int32)


def _cos_msin(m, n):
    """(cos, -sin)(2 pi m / n) for integers 0 <= m < n in float64, exact at the multiples of a quarter turn: the argument is reduced
    to a quarter turn in integers first."""
    m4 = 4 * np.asarray(m, np.int64)
    q, r = m4 // n, m4 % n
    a = (np.pi / 2) * (r.astype(np.float64) / n)
    c0, s0 = np.cos(a), np.sin(a)
    c = np.choose(q, [c0, -s0, -c0, s0])
    s = np.choose(q, [s0, c0, -s0, -c0])
    return c + 0.0, 0.0 - s             # (no -0 in the table)


def toa_tables(nbin, nharm, nlag):
    """(D float32 [nbin][nharm][2], L float32 [nharm][nlag][2]): D[b][k-1] = (cos, -sin)(2 pi k b / nbin), L[k-1][l] = (cos, -sin)
    (2 pi k l / nlag), k = 1 .. nharm.  The argument is reduced as the integer k b mod nbin (k l mod nlag) before the float64 sine
    and cosine, and each word is rounded once to float32."""
    if not all(_count(v) for v in (nbin, nharm, nlag)) or not 1 <= nbin <= MAX_NBIN or not 1 <= nharm <= min(MAX_NHARM, (nbin - 1) // 2) or \
            not 1 <= nlag <= MAX_NLAG:
        raise ValueError("toa_tables: nbin=%r (1 to %d), nharm=%r (1 to min(%d, (nbin - 1) / 2)), nlag=%r (1 to %d)"
                         % (nbin, MAX_NBIN, nharm, MAX_NHARM, nlag, MAX_NLAG))
    if max(nbin * nharm, nharm * nlag) * 8 > MAX_TABLE_BYTES:
        raise ValueError("toa_tables: a table above 1 GiB")
    k = np.arange(1, nharm + 1, dtype=np.int64)
    D = np.stack(_cos_msin((np.arange(nbin, dtype=np.int64)[:, None] * k[None, :]) % nbin, nbin), axis=-1)
    L = np.stack(_cos_msin((k[:, None] * np.arange(nlag, dtype=np.int64)[None, :]) % nlag, nlag), axis=-1)
    return np.ascontiguousarray(D, np.float32), np.ascontiguousarray(L, np.float32)


def toa_template(profiles, nharm, nsub=1):
    """S float32 [npair][nsub + 1][nharm][2] = (Re, Im) of S_k = sum_b s_b exp(-2 pi i k b / nbin), k = 1 .. nharm, in float64 and
    rounded once.  profiles is [npair][nbin] (one template per pair, used for each of its nsub sub-bands) or [npair][nsub][nbin]
    (one per sub-band); the band row, nsub, is the sum of the sub-bands' rows, as the band profile is the sum of the sub-bands'.
    Phase 0 of a template is the centre of its bin 0.  Refused: a template that is not finite or has no power in the harmonics
    1 .. nharm."""
    s = np.asarray(profiles, np.float64)
    if s.ndim == 2:
        if not _count(nsub) or not 1 <= nsub <= MAX_NSUB:
            raise ValueError("toa_template: nsub %r outside 1..%d" % (nsub, MAX_NSUB))
        s = np.repeat(s[:, None, :], nsub, axis=1)
    if s.ndim != 3 or 0 in s.shape:
        raise ValueError("toa_template: profiles of shape %r, [npair][nbin] or [npair][nsub][nbin] expected" % (s.shape,))
    nbin = s.shape[2]
    if not _count(nharm) or not 1 <= nharm <= min(MAX_NHARM, (nbin - 1) // 2):
        raise ValueError("toa_template: nharm %r outside 1..min(%d, (nbin - 1) / 2) at %d bins" % (nharm, MAX_NHARM, nbin))
    if not np.all(np.isfinite(s)):
        raise ValueError("toa_template: a template is not finite")
    k = np.arange(1, nharm + 1, dtype=np.int64)
    c, ms = _cos_msin((np.arange(nbin, dtype=np.int64)[:, None] * k[None, :]) % nbin, nbin)
    S = np.stack([s @ c, s @ ms], axis=-1)                          # [npair][nsub][nharm][2]
    S = np.concatenate([S, S.sum(1, keepdims=True)], axis=1)
    power = (S ** 2).sum((2, 3))
    floor = (1e-12 * np.abs(np.concatenate([s, s.sum(1, keepdims=True)], axis=1)).sum(2)) ** 2       # (the rounding of the sums above)
    if not np.all(power > floor):
        p, r = np.argwhere(~(power > floor))[0]
        raise ValueError("toa_template: the template of pair %d, row %d has no power in the harmonics 1..%d" % (p, r, nharm))
    return np.ascontiguousarray(S, np.float32)


def toa_refine(PH, S, l, nlag, var, n):
    """FFTFIT (Taylor 1992, appendix A) of one row in float64: PH, S [nharm][2] the profile's and the template's harmonics, l the
    lag the library picked on its grid of nlag, var the profile's off-pulse variance per bin and n its bins.  With
    C_k = P_k conj(S_k), the root of
        g(tau) = sum_k k |P_k| |S_k| sin(arg P_k - arg S_k + 2 pi k tau)                       (Taylor's A7)
    is bracketed by (l - 1) / nlag and (l + 1) / nlag and found by bisection, REFINE_ITERATIONS steps at the most.  Returns
    dict(tau, b, tau_err, b_err, chi2, snr, bracketed):
      tau      in turns, the profile's delay behind the template (not wrapped: within a lag of l / nlag);
      b        = sum_k |P_k||S_k| cos(.) / sum_k |S_k|^2, the amplitude                       (A9);
      tau_err  = sqrt(sigma^2 / (2 b sum_k k^2 |P_k||S_k| cos(.))) / (2 pi) turns            (A10);
      b_err    = sqrt(sigma^2 / (2 sum_k |S_k|^2))                                           (A11);
      chi2     = sum_k |P_k - b S_k exp(-2 pi i k tau)|^2 / sigma^2 per degree of freedom, 2 nharm - 2 of them (A6 at the minimum;
                 NaN at nharm = 1);
      snr      = b / b_err;
    with sigma^2 = n var / 2 the noise variance of one real or imaginary part of a harmonic.  bracketed is False where g has no
    sign change in the bracket: tau is then l / nlag itself.  None where l < 0 or a word is not finite."""
    PH, S = np.asarray(PH, np.float64), np.asarray(S, np.float64)
    if l is None or l < 0 or not (np.all(np.isfinite(PH)) and np.all(np.isfinite(S))):
        return None
    nharm = PH.shape[0]
    k = np.arange(1, nharm + 1, dtype=np.float64)
    P, T = PH[:, 0] + 1j * PH[:, 1], S[:, 0] + 1j * S[:, 1]
    C = P * np.conj(T)

    def g(tau):
        return float(np.sum(k * (C * np.exp(2j * np.pi * k * tau)).imag))

    lo, hi = (l - 1.0) / nlag, (l + 1.0) / nlag
    glo, ghi = g(lo), g(hi)
    bracketed = glo < 0 < ghi or glo > 0 > ghi
    tau = float(l) / nlag
    if glo == 0:
        tau, bracketed = lo, True
    elif ghi == 0:
        tau, bracketed = hi, True
    elif bracketed:
        for _ in range(REFINE_ITERATIONS):
            mid = 0.5 * (lo + hi)
            gm = g(mid)
            if gm == 0 or mid == lo or mid == hi:
                lo = hi = mid
                break
            if (gm < 0) == (glo < 0):
                lo, glo = mid, gm
            else:
                hi = mid
        tau = 0.5 * (lo + hi)
    rot = C * np.exp(2j * np.pi * k * tau)
    ss = float(np.sum(np.abs(T) ** 2))
    b = float(np.sum(rot.real)) / ss
    sigma2 = 0.5 * float(n) * float(var)
    curv = b * float(np.sum(k * k * rot.real))
    with np.errstate(divide='ignore', invalid='ignore'):
        tau_err = float(np.sqrt(sigma2 / (2.0 * curv)) / (2 * np.pi)) if curv > 0 else float('inf')
        b_err = float(np.sqrt(sigma2 / (2.0 * ss)))
        res = float(np.sum(np.abs(P - b * T * np.exp(-2j * np.pi * k * tau)) ** 2))
        chi2 = res / sigma2 / (2 * nharm - 2) if nharm > 1 and sigma2 > 0 else float('nan')
        snr = b / b_err if b_err > 0 else (float('inf') if b > 0 else 0.0)
    return dict(tau=tau, b=b, tau_err=tau_err, b_err=b_err, chi2=chi2, snr=snr, bracketed=bool(bracketed))


def toa_dm_fit(tau, sigma, freqs, f_spin, tau_band=None):
    """Weighted least squares of tau_r = tau_inf + KDM ddm f_spin f_r**-2 over the sub-bands (f_r in Hz here, MHz in the formula;
    KDM of blocks/dedisp.py; f_spin in Hz), tau and sigma in turns.  Every tau_r is first moved by whole turns to the turn nearest
    tau_band (the band row's offset; the offset of the sub-band with the smallest sigma if None).  A sub-band is usable if its tau
    and sigma are finite and sigma > 0.  Returns dict(dm, dm_err, tau_inf, tau_inf_err, chi2, nused, tau): dm = ddm in pc cm^-3,
    the errors propagated from sigma, chi2 the weighted sum of squared residuals (nused - 2 degrees of freedom), tau the unwrapped
    offsets.  With fewer than two usable sub-bands (or all at one frequency) dm, dm_err, tau_inf, tau_inf_err and chi2 are None."""
    tau = np.array([np.nan if v is None else v for v in tau], np.float64)
    sigma = np.array([np.nan if v is None else v for v in sigma], np.float64)
    f = np.asarray(freqs, np.float64) * 1e-6
    if not (tau.shape == sigma.shape == f.shape and tau.ndim == 1) or not (np.all(np.isfinite(f)) and np.all(f > 0)) or not f_spin > 0:
        raise ValueError("toa_dm_fit: one finite positive frequency per sub-band and a positive spin frequency are needed")
    ok = np.isfinite(tau) & np.isfinite(sigma) & (sigma > 0)
    out = dict(dm=None, dm_err=None, tau_inf=None, tau_inf_err=None, chi2=None, nused=int(ok.sum()), tau=tau)
    if not ok.any():
        return out
    ref = float(tau_band) if tau_band is not None and np.isfinite(tau_band) else float(tau[ok][np.argmin(sigma[ok])])
    tau = np.where(ok, tau - np.round(tau - ref), np.nan)
    out['tau'] = tau
    x = KDM * float(f_spin) * f[ok] ** -2
    if ok.sum() < 2 or np.ptp(x) == 0:
        return out
    wt = sigma[ok] ** -2
    x0 = np.sum(wt * x) / np.sum(wt)                                # (centred: the two parameters decouple)
    sxx = np.sum(wt * (x - x0) ** 2)
    dm = np.sum(wt * (x - x0) * tau[ok]) / sxx
    mean = np.sum(wt * tau[ok]) / np.sum(wt)
    tau_inf = mean - dm * x0
    res = tau[ok] - (tau_inf + dm * x)
    out.update(dm=float(dm), dm_err=float(np.sqrt(1.0 / sxx)), tau_inf=float(tau_inf), tau_inf_err=float(np.sqrt(1.0 / np.sum(wt) + x0 * x0 / sxx)),
               chi2=float(np.sum(wt * res * res)))
    return out


def toa_epoch(header, pair, tau):
    """The arrival time, on the sequence's sample clock in seconds as an exact Fraction, of the pulse nearest the sub-integration's
    midpoint, for a profile that lags its template by tau turns.

    Convention.  BeamFold puts a window whose midpoint has the model phase phi(t) = f0 (t - pepoch) + f1 (t - pepoch)^2 / 2 into
    bin floor(frac(phi) nbin), so the centre of bin b is the phase (b + 1/2) / nbin; phase 0 of a template is the centre of its
    bin 0 (toa_template).  The template's phase 0 therefore arrives when frac(phi(t)) = tau + 1 / (2 nbin).  The time refers to the
    frequency BeamFold aligns its channels to -- the centre of the highest fine channel -- at the DM of the header's pulsar list; it
    is topocentric, as f0, f1 and pepoch are.  The midpoint is t_mid = subint_start nchan / bw_hz + subint_nwindow tsamp / 2 (the
    header's subint_start is in samples of nchan / bw_hz seconds).  The result is the solution of phi(t) = N + tau + 1 / (2 nbin)
    with N the integer that brings t nearest t_mid: exact where f1 = 0, else after four Newton steps in rational arithmetic from
    t_mid (an error below 1e-30 s for any pulsar)."""
    e = header['pulsars'][pair]
    if e is None:
        raise ValueError("toa_epoch: pair %d has no pulsar" % pair)
    f0, f1, pepoch = Fraction(e['f0']), Fraction(e.get('f1', 0.0)), Fraction(e.get('pepoch', 0.0))
    per = Fraction(header['nchan']) / Fraction(header['bw_hz'])
    t_mid = Fraction(header['subint_start']) * per + Fraction(header['subint_nwindow']) * Fraction(header['tsamp']) / 2
    target = Fraction(float(tau)) + Fraction(1, 2 * int(header['nbin']))

    def phi(t):
        return f0 * (t - pepoch) + f1 * (t - pepoch) ** 2 / 2

    want = round(phi(t_mid) - target) + target                      # N + the target's fraction
    if f1 == 0:
        return pepoch + want / f0
    t = t_mid
    for _ in range(4):
        t = t - (phi(t) - want) / (f0 + f1 * (t - pepoch))
        t = Fraction(t).limit_denominator(1 << 200)
    return t


def subband_frequencies(freqs_hz, edges, weights=None):
    """float64 [nsub]: the frequency in Hz whose dispersion delay is the mean delay of sub-band r's used groups, (mean of f**-2 under
    |w|)**-1/2; NaN for a sub-band without a used group."""
    f = np.asarray(freqs_hz, np.float64).reshape(-1)
    w = np.ones(f.size) if weights is None else np.abs(np.asarray(weights, np.float64).reshape(-1))
    out = np.full(len(edges) - 1, np.nan)
    for r in range(len(edges) - 1):
        a, b = int(edges[r]), int(edges[r + 1])
        if w[a:b].sum() > 0:
            out[r] = (np.sum(w[a:b] * f[a:b] ** -2) / w[a:b].sum()) ** -0.5
    return out


def toa_reference(X, edges, w, D, L, S, off=None, active=None):
    """The float64 statement of the contract: X [npair][nprod][nchg][nbin], D [nbin][nharm][2], L [nharm][nlag][2], S
    [npair][nsub+1][nharm][2].  dict(P [npair][nsub+1][nbin], base, var [npair][nsub+1], PH [npair][nsub+1][nharm][2], ccf
    [npair][nsub+1][nlag], l [npair][nsub+1], and the scales of a rounding-error bound: A [npair][nsub+1][nbin] = sum_g |w_g||x| + its
    off-pulse mean, ph_scale [npair][nsub+1][nharm][2] = sum_b A_b |D|, ccf_scale [npair][nsub+1][nlag]).  No order of summation is
    stated: that is the library's."""
    X, D, L, S = (np.asarray(a, np.float64) for a in (X, D, L, S))
    npair, nprod, nchg, nbin = X.shape
    nsub, nharm, nlag = len(edges) - 1, D.shape[1], L.shape[1]
    w = np.ones(nchg) if w is None else np.asarray(w, np.float64)
    off = np.ones((npair, nbin), bool) if off is None else np.asarray(off) != 0
    active = np.ones(npair, bool) if active is None else np.asarray(active) != 0
    sh = (npair, nsub + 1)
    out = dict(P=np.zeros(sh + (nbin,)), base=np.zeros(sh), var=np.zeros(sh), PH=np.zeros(sh + (nharm, 2)), ccf=np.zeros(sh + (nlag,)),
               l=np.full(sh, -1), A=np.zeros(sh + (nbin,)), ph_scale=np.zeros(sh + (nharm, 2)), ccf_scale=np.zeros(sh + (nlag,)))
    for p in range(npair):
        if not active[p]:
            continue
        x = X[p, 0] + X[p, 1] if nprod == 4 else X[p, 0]
        ax = np.abs(X[p, 0]) + np.abs(X[p, 1]) if nprod == 4 else np.abs(X[p, 0])
        for r in range(nsub):
            g = np.arange(edges[r], edges[r + 1])
            g = g[w[g] != 0]
            out['P'][p, r] = w[g] @ x[g]
            out['A'][p, r] = np.abs(w[g]) @ ax[g]
        out['P'][p, nsub], out['A'][p, nsub] = out['P'][p, :nsub].sum(0), out['A'][p, :nsub].sum(0)
        n_off = int(off[p].sum())
        if n_off:
            out['base'][p] = out['P'][p][:, off[p]].mean(1)
            out['A'][p] += out['A'][p][:, off[p]].mean(1, keepdims=True)
        d = out['P'][p] - out['base'][p][:, None]
        if n_off:
            out['var'][p] = (d[:, off[p]] ** 2).mean(1)
        PH = np.einsum('rb,bkc->rkc', d, D)
        E = np.einsum('rb,bkc->rkc', out['A'][p], np.abs(D))
        out['PH'][p], out['ph_scale'][p] = PH, E
        sr, si = S[p, :, :, 0], S[p, :, :, 1]
        cr, ci = PH[..., 0] * sr + PH[..., 1] * si, PH[..., 1] * sr - PH[..., 0] * si
        out['ccf'][p] = cr @ L[:, :, 0] + ci @ L[:, :, 1]
        out['ccf_scale'][p] = (E[..., 0] * np.abs(sr) + E[..., 1] * np.abs(si)) @ np.abs(L[:, :, 0]) + \
            (E[..., 1] * np.abs(sr) + E[..., 0] * np.abs(si)) @ np.abs(L[:, :, 1])
        for r in range(nsub + 1):
            c = out['ccf'][p, r]
            used = np.count_nonzero(w[edges[r]:edges[r + 1]]) if r < nsub else np.count_nonzero(w[edges[0]:edges[nsub]])
            if used and not np.all(np.isnan(c)):
                out['l'][p, r] = int(np.nanargmax(c))
    return out
