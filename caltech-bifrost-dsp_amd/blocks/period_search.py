"""Host side of the periodicity search: the record plane xengPeriodRun writes when a stack completes, the false-alarm probability
of a harmonic sum and the thresholding and grouping of a plane over DM.

A plane is [npair][ndm][nlevel] records of two 32-bit words {f32 H, i32 k} (include/xeng.h, "FFT periodicity search of the
dedispersed beams"): per series and harmonic level l (h = 2^l harmonics) the largest harmonic sum of the whitened, stacked power
spectrum and the bin k of its TOP harmonic; k = -1 where nothing qualified.  Under noise a whitened power is exponential with mean
1, so a sum of h harmonics over nstack stacked spectra is Gamma(a = h * nstack, 1) and its survival function has the closed form
Q(a, H) = exp(-H) * sum_{i < a} H^i / i! for the integer a (period_pfa, in log space, no scipy).  A periodic source that is
bright at one DM trial is above the threshold at its neighbours too, so period_candidates reports, per pair and level, the
records whose k agree within one bin as one candidate.  Pure numpy.  Not built: sifting of harmonically related candidates (the
same source is reported once per level that clears the threshold, and at k, 2k ... within a level's search range), and any
grouping across pairs or across stacks."""
import math
import statistics

import numpy as np

RECORD = np.dtype([('H', '<f4'), ('k', '<i4')])


def as_records(plane, npair=None, ndm=None, nlevel=None):
    """A plane as a RECORD array [npair][ndm][nlevel]: from a RECORD array, or from raw bytes / 32-bit words (then with npair, ndm
    and nlevel, or with a shape [npair][ndm][nlevel][2 words])."""
    a = np.asarray(plane)
    if a.dtype != RECORD:
        if npair is None:
            if a.ndim != 4 or a.shape[3] * a.dtype.itemsize != RECORD.itemsize:
                raise ValueError("period_search: a raw plane needs a shape [npair][ndm][nlevel][8 bytes], or npair, ndm and nlevel")
            npair, ndm, nlevel = a.shape[:3]
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size != npair * ndm * nlevel * RECORD.itemsize:
            raise ValueError("period_search: %d bytes are not %d x %d x %d records" % (a.size, npair, ndm, nlevel))
        a = a.view(RECORD).reshape(npair, ndm, nlevel)
    if a.ndim != 3:
        raise ValueError("period_search: a plane is [npair][ndm][nlevel] records, not %r" % (a.shape,))
    return a


def period_pfa(H, h, nstack):
    """The natural log of the probability that one bin's sum of h harmonics over nstack stacked, whitened spectra reaches H under
    noise: ln Q(a, H), a = h * nstack, Q(a, H) = exp(-H) * sum_{i < a} H^i / i!.  H: a number or an array (H <= 0 gives ln 1 = 0);
    evaluated in log space, so that it neither overflows at large a nor underflows at large H."""
    a = int(h) * int(nstack)
    if a < 1:
        raise ValueError("period_search: h * nstack = %d" % a)
    Hs = np.asarray(H, np.float64)
    x = np.maximum(Hs, 0.0)
    i = np.arange(a, dtype=np.float64)
    lfact = np.concatenate(([0.0], np.cumsum(np.log(np.arange(1, a, dtype=np.float64)))))      # ln i!
    with np.errstate(divide='ignore', invalid='ignore'):
        t = i * np.log(x)[..., None] - lfact                    # ln (H^i / i!); H = 0: -inf for i >= 1
        t = np.where(i == 0, 0.0, t)                            # (0 * ln 0)
    m = t.max(axis=-1)
    out = -x + m + np.log(np.exp(t - m[..., None]).sum(axis=-1))
    out = np.minimum(out, 0.0)
    return out if out.ndim else float(out)


def _sigma(log10_p):
    """The Gaussian-equivalent significance of a one-sided probability 10^log10_p (clamped at 1e-300, about 37 sigma)."""
    p = 10.0 ** max(log10_p, -300.0)
    return 0.0 if p >= 0.5 else -statistics.NormalDist().inv_cdf(p)


def period_candidates(plane, threshold, dms, nt, nstack, tsamp, ntrials=None):
    """plane: one record plane (as_records takes it); dms: the ndm trial DMs; nt, nstack, tsamp: the segment length in windows,
    the segments per stack and the window length in seconds.  A record's score is -log10 of its false-alarm probability
    min(1, ntrials * Q): ntrials is the number of bins one series was searched in (default: nlevel * nt / 2, an upper bound).
    Per pair and level, the records with score >= threshold are grouped: the best (among equals the lowest trial) takes with it
    every other whose k lies within one bin of its own, then the best of the rest, and so on.  One candidate per group:
      dict(pair, idm, dm, ntrial, h, k, freq, period, H, log10_pfa, sigma)
    k is the bin of the top harmonic, freq = k / (h * nt * tsamp) the fundamental in Hz, period = 1 / freq, log10_pfa the
    corrected probability and sigma its Gaussian equivalent, ntrial the size of the group.  In order of pair, level, trial."""
    rec = as_records(plane)
    npair, ndm, nlevel = rec.shape
    dms = np.asarray(dms, np.float64).reshape(-1)
    if dms.size != ndm:
        raise ValueError("period_search: %d DMs for a plane of %d trials" % (dms.size, ndm))
    if ntrials is None:
        ntrials = nlevel * (nt // 2)
    ln_nt = math.log(max(float(ntrials), 1.0))
    out = []
    for lv in range(nlevel):
        h = 1 << lv
        ok = rec['k'][:, :, lv] >= 0
        lp = np.minimum((period_pfa(np.where(ok, rec['H'][:, :, lv], 0.0), h, nstack) + ln_nt) / math.log(10.0), 0.0)
        score = np.where(ok, -lp, -np.inf)
        for p in range(npair):
            left = [int(d) for d in np.flatnonzero(score[p] >= float(threshold))]
            left.sort(key=lambda d: (-score[p, d], d))
            while left:
                d = left[0]
                k = int(rec['k'][p, d, lv])
                group = [e for e in left if abs(int(rec['k'][p, e, lv]) - k) <= 1]
                left = [e for e in left if e not in group]
                freq = k / (h * nt * float(tsamp))
                out.append(dict(pair=p, idm=d, dm=float(dms[d]), ntrial=len(group), h=h, k=k, freq=freq, period=1.0 / freq,
                                H=float(rec['H'][p, d, lv]), log10_pfa=float(lp[p, d]), sigma=_sigma(float(lp[p, d]))))
    out.sort(key=lambda c: (c['pair'], c['h'], c['idm']))
    return out
