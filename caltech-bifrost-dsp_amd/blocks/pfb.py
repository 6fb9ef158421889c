"""The polyphase filter bank front end of UpchanBeamform and UpchanCorr (include/xeng.h xengUpchanSetPfb): its default
coefficients and the checks both blocks make on `pfb_ntap` / `pfb_coeffs`."""
import numpy as np

MAX_TAPS = 8        # include/xeng.h: 1 <= ntap <= 8


def pfb_coeffs(ntap, nupchan):
    """The default P-tap, N-channel prototype filter, float32 [P*N]: h[m] = sinc((m + 0.5 - P*N/2) / N) * hamming(P*N)[m],
    scaled so that sum(h) = N (a tone at a fine channel's centre keeps the plain FFT's amplitude at any P).  Symmetric."""
    m = np.arange(ntap * nupchan, dtype=np.float64)
    h = np.sinc((m + 0.5 - ntap * nupchan / 2.0) / nupchan) * np.hamming(ntap * nupchan)
    return (h * (nupchan / h.sum())).astype(np.float32)


def pfb_config(who, ntap, coeffs, nupchan, ntime_gulp):
    """(ntap, float32 coefficients or None) after the blocks' argument checks (ValueError "<who>: ..."): None means the plain
    FFT (ntap 1 without coefficients: no PFB call is made), otherwise the default coefficients when none are given."""
    if isinstance(ntap, bool) or not isinstance(ntap, (int, np.integer)) or not 1 <= ntap <= MAX_TAPS:
        raise ValueError("%s: pfb_ntap %r not an integer in 1..%d" % (who, ntap, MAX_TAPS))
    ntap = int(ntap)
    if (ntap - 1) * nupchan > ntime_gulp:
        raise ValueError("%s: gulps of %d samples are shorter than the PFB history of %d x %d" % (who, ntime_gulp, ntap - 1, nupchan))
    if coeffs is None:
        return ntap, (pfb_coeffs(ntap, nupchan) if ntap > 1 else None)
    h = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1)
    if h.size != ntap * nupchan:
        raise ValueError("%s: %d PFB coefficients given, pfb_ntap x nupchan = %d needed" % (who, h.size, ntap * nupchan))
    if not np.isfinite(h).all():
        raise ValueError("%s: PFB coefficients are not all finite" % who)
    return ntap, h
