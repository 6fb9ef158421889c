"""Host helpers of BeamDetrend (xengDetrend*, include/xeng.h "Baseline removal of the dedispersed beams"): the block length for a
timescale, the spans the block drops at the start of a sequence, the scale as the library takes it, and a float64 statement of what
the library computes, for users and for tests."""
import math

import numpy as np

MAD_TO_SIGMA = 1.4826           # sigma of a normal distribution over its median absolute deviation
NBLK_MIN, NBLK_MAX = 4, 8192


def detrend_k_mad():
    """k_mad for xengDetrendInitialize: the output is in units of 1.4826 MAD, sigma for normal noise."""
    return float(np.float32(MAD_TO_SIGMA))


def detrend_plan(tsamp, timescale_s, nwin):
    """nblk, the block length in windows: the even number nearest timescale_s / tsamp (tsamp the duration of a window in seconds)
    within 4..8192 whose latency 3 nblk / 2 is a whole number of spans of nwin windows and which is at least nwin; ties go to the
    smaller.  The baseline follows variations slower than about two blocks.  ValueError if there is none."""
    if isinstance(nwin, bool) or not isinstance(nwin, int) or nwin < 1:
        raise ValueError("detrend_plan: nwin %r is not a positive integer" % (nwin,))
    for name, v in (('tsamp', tsamp), ('timescale_s', timescale_s)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
            raise ValueError("detrend_plan: %s %r is not a finite positive number" % (name, v))
    want = timescale_s / tsamp
    ok = [n for n in range(NBLK_MIN, NBLK_MAX + 1, 2) if (3 * n // 2) % nwin == 0 and n >= nwin]
    if not ok:
        raise ValueError("detrend_plan: no even nblk in %d..%d has 3 nblk / 2 a multiple of nwin = %d" % (NBLK_MIN, NBLK_MAX, nwin))
    return min(ok, key=lambda n: (abs(n - want), n))


def detrend_startup(dedisp_latency, nblk, nwin):
    """Input spans at the head of a sequence whose detrended windows BeamDetrend does not commit: the dedisperser's first
    S = dedisp_latency windows are partial sums, so every window before W = ceil(S / nblk) nblk + nblk / 2 lies against a knot that
    saw some; the count is ceil(W / nwin)."""
    for name, v in (('dedisp_latency', dedisp_latency), ('nblk', nblk), ('nwin', nwin)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError("detrend_startup: %s %r is not a non-negative integer" % (name, v))
    if nblk < NBLK_MIN or nblk % 2 or nwin < 1:
        raise ValueError("detrend_startup: nblk %r, nwin %r" % (nblk, nwin))
    W = -(-dedisp_latency // nblk) * nblk + nblk // 2
    return -(-W // nwin)


def detrend_reference(z, nblk, normalise=True, k_mad=MAD_TO_SIGMA):
    """What BeamDetrend computes, in float64: z [nwindows][...] -> (y the same shape, M, A [nblocks][...], valid bool
    [nblocks][...]).  y[m] is the detrended window m itself (no latency); windows whose second knot is not complete within z, the
    last nblk / 2 to 3 nblk / 2, read 0, as do windows without a valid knot and results that are not finite."""
    z = np.asarray(z, np.float64)
    shape = z.shape[1:]
    z = z.reshape(z.shape[0], -1)
    nwindows = z.shape[0]
    if nblk % 2 or not NBLK_MIN <= nblk <= NBLK_MAX:
        raise ValueError("detrend_reference: nblk %r is not even and in 4..8192" % (nblk,))
    nb, h = nwindows // nblk, nblk // 2
    blk = z[:nb * nblk].reshape(nb, nblk, -1)
    finite = np.isfinite(blk).all(axis=1)
    with np.errstate(all='ignore'):
        safe = np.where(finite[:, None], blk, 0.0)
        M = np.where(finite, np.median(safe, axis=1), 0.0)
        A = np.where(finite, np.median(np.abs(safe - M[:, None]), axis=1), 0.0)
        valid = finite.copy()
        G = np.zeros_like(M)
        if normalise:
            s = k_mad * A
            valid &= (s > 0) & np.isfinite(s)
            G = np.where(valid, 1.0 / np.where(valid, s, 1.0), 0.0)
        y = np.zeros_like(z)
        for m in range(nwindows):
            k = -1 if m < h else (m - h) // nblk
            t = m - (k * nblk + h)
            a, b = max(k, 0), k + 1
            if b >= nb:
                break
            va, vb = valid[a], valid[b]
            u = (2 * t + 1) / (2.0 * nblk)
            Ma, Mb = np.where(va, M[a], M[b]), np.where(vb, M[b], M[a])
            v = z[m] - (Ma + u * (Mb - Ma))
            if normalise:
                Ga, Gb = np.where(va, G[a], G[b]), np.where(vb, G[b], G[a])
                v = v * (Ga + u * (Gb - Ga))
            y[m] = np.where((va | vb) & np.isfinite(v), v, 0.0)
    return y.reshape((nwindows,) + shape), M.reshape((nb,) + shape), A.reshape((nb,) + shape), valid.reshape((nb,) + shape)
