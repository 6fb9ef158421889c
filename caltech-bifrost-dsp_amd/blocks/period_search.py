"""Host side of the periodicity search: the record plane xengPeriodRun writes when a stack completes, the false-alarm probability
of a harmonic sum and the thresholding and grouping of a plane over DM.

A plane is [npair][ndm][nlevel] records of two 32-bit words {f32 H, i32 k} (include/xeng.h, "FFT periodicity search of the
dedispersed beams"): per series and harmonic level l (h = 2^l harmonics) the largest harmonic sum of the whitened, stacked power
spectrum and the bin k of its TOP harmonic; k = -1 where nothing qualified.  Under noise a whitened power is exponential with mean
1, so a sum of h harmonics over nstack stacked spectra is Gamma(a = h * nstack, 1) and its survival function has the closed form
Q(a, H) = exp(-H) * sum_{i < a} H^i / i! for the integer a (period_pfa, in log space, no scipy).  A periodic source that is
bright at one DM trial is above the threshold at its neighbours too, so period_candidates reports, per pair and level, the
records whose k agree within one bin as one candidate.  Pure numpy.  period_candidates does not sift harmonically related candidates (the
same source is reported once per level that clears the threshold, and at k, 2k ... within a level's search range); the long-segment
search does: its planes carry one record per BAND of fundamental frequency as well ([npair][ndm][nlevel][nband], xengPlong*,
"FFT periodicity search with long segments"), period_bands makes the edges, period_candidates_long thresholds and groups such a
plane and period_sift merges the candidates of one pair whose fundamentals are in a small rational ratio.  Not built: any grouping
across pairs or across stacks."""
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


def period_bands(nt, nband, kmin, kmax=None):
    """The nband + 1 edges of nband log-spaced bands of fundamental frequency from bin kmin to bin kmax (default nt/2): strictly
    ascending integers, the first kmin and the last kmax, as xengPlongInitialize takes them.  Where the logarithmic spacing is
    closer than one bin the edges step by one bin instead."""
    nt, nband, kmin = int(nt), int(nband), int(kmin)
    kmax = nt // 2 if kmax is None else int(kmax)
    if not 1 <= nband <= 32:
        raise ValueError("period_bands: %d bands, not 1 to 32" % nband)
    if not 1 <= kmin < nt // 32:
        raise ValueError("period_bands: kmin %d not in 1 .. nt/32 - 1" % kmin)
    if not kmin + nband <= kmax <= nt // 2:
        raise ValueError("period_bands: kmax %d leaves no room for %d bands between %d and nt/2 = %d" % (kmax, nband, kmin, nt // 2))
    edges = [kmin]
    for i in range(1, nband + 1):
        e = int(round(kmin * (kmax / kmin) ** (i / nband)))
        edges.append(min(max(e, edges[-1] + 1), kmax - (nband - i)))
    return edges


def as_records_long(plane, npair=None, ndm=None, nlevel=None, nband=None):
    """A plane of the long-segment search as a RECORD array [npair][ndm][nlevel][nband]: from a RECORD array, or from raw bytes /
    32-bit words with the four sizes."""
    a = np.asarray(plane)
    if a.dtype != RECORD:
        if None in (npair, ndm, nlevel, nband):
            raise ValueError("period_search: a raw plane needs npair, ndm, nlevel and nband")
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size != npair * ndm * nlevel * nband * RECORD.itemsize:
            raise ValueError("period_search: %d bytes are not %d x %d x %d x %d records" % (a.size, npair, ndm, nlevel, nband))
        a = a.view(RECORD).reshape(npair, ndm, nlevel, nband)
    if a.ndim != 4:
        raise ValueError("period_search: a banded plane is [npair][ndm][nlevel][nband] records, not %r" % (a.shape,))
    return a


def band_bins(kedge, level, nt):
    """The number of top-harmonic bins of every band at level `level`: h*kedge[b] <= k < min(h*kedge[b+1], nt/2)."""
    h, n = 1 << level, nt // 2
    return [max(0, min(h * int(kedge[b + 1]), n) - h * int(kedge[b])) for b in range(len(kedge) - 1)]


def period_candidates_long(plane, threshold, dms, nt, nstack, tsamp, kedge, ntrials=None):
    """period_candidates for a banded plane [npair][ndm][nlevel][nband] (as_records_long takes it) with the edges kedge it was made
    with.  A record's score is -log10 of min(1, ntrials * Q), Q from period_pfa; ntrials is the number of bins one series was
    searched in (default: the bins of every band at every level, counted exactly).  Per pair and level, the records of all
    trials and bands with score >= threshold are grouped as period_candidates groups them: the best (among equals the lowest
    trial, then the lowest band) takes with it every other whose k lies within one bin of its own -- a source at a band's edge
    is in both bands at neighbouring trials -- then the best of the rest, and so on.  One candidate per group:
      dict(pair, idm, dm, ntrial, h, band, k, freq, period, H, log10_pfa, sigma)
    freq = k / (h * nt * tsamp) is the fundamental in Hz.  In order of pair, level, trial, band."""
    rec = as_records_long(plane)
    npair, ndm, nlevel, nband = rec.shape
    if len(kedge) != nband + 1:
        raise ValueError("period_search: %d edges for a plane of %d bands" % (len(kedge), nband))
    dms = np.asarray(dms, np.float64).reshape(-1)
    if dms.size != ndm:
        raise ValueError("period_search: %d DMs for a plane of %d trials" % (dms.size, ndm))
    if ntrials is None:
        ntrials = sum(sum(band_bins(kedge, lv, nt)) for lv in range(nlevel))
    ln_nt = math.log(max(float(ntrials), 1.0))
    out = []
    for lv in range(nlevel):
        h = 1 << lv
        ok = rec['k'][:, :, lv] >= 0
        lp = np.minimum((period_pfa(np.where(ok, rec['H'][:, :, lv], 0.0), h, nstack) + ln_nt) / math.log(10.0), 0.0)
        score = np.where(ok, -lp, -np.inf)
        for p in range(npair):
            left = [(int(d), int(b)) for d, b in np.argwhere(score[p] >= float(threshold))]
            left.sort(key=lambda db: (-score[p][db], db))
            while left:
                d, b = left[0]
                k = int(rec['k'][p, d, lv, b])
                group = [e for e in left if abs(int(rec['k'][p, e[0], lv, e[1]]) - k) <= 1]
                left = [e for e in left if e not in group]
                freq = k / (h * nt * float(tsamp))
                out.append(dict(pair=p, idm=d, dm=float(dms[d]), ntrial=len(group), h=h, band=b, k=k, freq=freq, period=1.0 / freq,
                                H=float(rec['H'][p, d, lv, b]), log10_pfa=float(lp[p, d, b]), sigma=_sigma(float(lp[p, d, b]))))
    out.sort(key=lambda c: (c['pair'], c['h'], c['idm'], c['band']))
    return out


def _ratio(ca, cb, max_ratio, tol_bins):
    """(a, b) with a * f_a = b * f_b, f = k / h the fundamentals in bins, to within tol_bins bins at the top harmonic, or None: k is
    known to a bin, so a * f_a to a / h_a bins and b * f_b to b / h_b, and the two may differ by tol_bins * max(1, a / h_a + b / h_b).
    Among the ratios that fit, the one with the smallest a + b."""
    fa, fb = ca['k'] / ca['h'], cb['k'] / cb['h']
    best = None
    for a in range(1, max_ratio + 1):
        for b in range(1, max_ratio + 1):
            if abs(a * fa - b * fb) <= tol_bins * max(1.0, a / ca['h'] + b / cb['h']) and (best is None or a + b < sum(best)):
                best = (a, b)
    return best


def period_sift(cands, nt, max_ratio=16, tol_bins=1.0):
    """Harmonic sifting of the candidates of period_candidates_long (or period_candidates): within one pair, two candidates are
    merged when their fundamentals are in a ratio a / b with a, b <= max_ratio, to within tol_bins bins at the top harmonic (k is known
    to a bin there: the common harmonic a * f = b * f' may differ by tol_bins * max(1, a / h + b / h')).  The
    candidates of a pair are taken in order of significance (log10_pfa, then the larger H, the smaller h, k, idm and band); the
    most significant one left absorbs every other left that is so related TO IT, then the most significant of the rest, and so
    on.  Each survivor is a copy of its candidate with `harmonics`, the list of the candidates it absorbed in the same order, each
    with `ratio` = (a, b): a times the survivor's fundamental is b times its own.  The output, in order of pair and significance,
    does not depend on the order of the input.  nt: the segment length (k < nt/2 is checked)."""
    def key(c):
        return (c['pair'], c['log10_pfa'], -c['H'], c['h'], c['k'], c['idm'], c.get('band', 0))
    for c in cands:
        if not 0 <= c['k'] < nt // 2:
            raise ValueError("period_sift: bin %d is outside a segment of %d windows" % (c['k'], nt))
    left = sorted(cands, key=key)
    out = []
    while left:
        top, rest = dict(left[0]), []
        top['harmonics'] = []
        for c in left[1:]:
            r = _ratio(top, c, max_ratio, tol_bins) if c['pair'] == top['pair'] else None
            if r is None:
                rest.append(c)
            else:
                top['harmonics'].append(dict(c, ratio=r))
        out.append(top)
        left = rest
    return out
