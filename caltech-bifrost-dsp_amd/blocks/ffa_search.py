"""Host side of the fast-folding search: the record plane xengFfaRun writes when a segment completes, the trial period a record
stands for, a plan of the sizes from a range of periods and a duty cycle, and the thresholding and grouping of a plane.

A plane is [npair][ndm][noct][nwidth] records of four 32-bit words {f32 snr, i32 p, i32 i, i32 j} (include/xeng.h, "Fast-folding
search of the dedispersed beams"): per series, octave o and boxcar width 2^iw the largest matched-filter score over the folds of
the segment, in units of the noise (the sum of w * M samples of unit variance divided by sqrt(w * M)), at base period p samples,
profile i of M = ffa_rows(nt >> o, p) and phase bin j; p = -1 where the (series, octave) had no statistics.  A sample of octave o
is 2^o * nds windows, so the record's period is (p + i / (M - 1)) * 2^o * nds * tsamp seconds (ffa_period).  A source that is
bright at one DM trial is above the threshold at its neighbours, at the neighbouring widths and -- folded at twice the resolution
-- in the next octave too, so ffa_candidates reports, per pair, the records whose periods agree within one period step as one
candidate.  Pure numpy.  Not built: sifting of harmonically related candidates beyond that grouping (a source of period P also
folds up at 2 P, 3 P ... and is then reported there as well), more than one peak per (series, octave, width), and any grouping
across pairs or across segments."""
import math

import numpy as np

RECORD = np.dtype([('snr', '<f4'), ('p', '<i4'), ('i', '<i4'), ('j', '<i4')])


def as_records(plane, npair=None, ndm=None, noct=None, nwidth=None):
    """A plane as a RECORD array [npair][ndm][noct][nwidth]: from a RECORD array, or from raw bytes / 32-bit words (then with
    npair, ndm, noct and nwidth, or with a shape [npair][ndm][noct][nwidth][4 words])."""
    a = np.asarray(plane)
    if a.dtype != RECORD:
        if npair is None:
            if a.ndim != 5 or a.shape[4] * a.dtype.itemsize != RECORD.itemsize:
                raise ValueError("ffa_search: a raw plane needs a shape [npair][ndm][noct][nwidth][16 bytes], or npair, ndm, noct and nwidth")
            npair, ndm, noct, nwidth = a.shape[:4]
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size != npair * ndm * noct * nwidth * RECORD.itemsize:
            raise ValueError("ffa_search: %d bytes are not %d x %d x %d x %d records" % (a.size, npair, ndm, noct, nwidth))
        a = a.view(RECORD).reshape(npair, ndm, noct, nwidth)
    if a.ndim != 4:
        raise ValueError("ffa_search: a plane is [npair][ndm][noct][nwidth] records, not %r" % (a.shape,))
    return a


def ffa_rows(n, p):
    """M: the rows a segment of n samples is folded in at base period p, the largest power of two with M * p <= n (0 if p > n)."""
    n, p = int(n), int(p)
    if p < 1:
        raise ValueError("ffa_search: base period %d" % p)
    if p > n:
        return 0
    M = 1
    while 2 * M * p <= n:
        M *= 2
    return M


def ffa_period(p, i, M, o, nds, tsamp):
    """The period in seconds of profile i of M at base period p in octave o: (p + i / (M - 1)) * 2^o * nds * tsamp."""
    if M < 2 or not 0 <= i < M:
        raise ValueError("ffa_search: profile %d of %d" % (i, M))
    return (p + i / (M - 1.0)) * (1 << o) * nds * float(tsamp)


def ffa_plan(pmin_s, pmax_s, tsamp, duty):
    """The sizes of a search for periods pmin_s .. pmax_s seconds of windows tsamp seconds long and pulses of about `duty` of a
    period: (nds, nt, noct, pmin, pmax, nwidth).  Every octave folds at base periods of pmin .. pmax = 2 pmin - 1 samples, so that a
    sample -- the narrowest boxcar -- is between duty and duty / 2 of a period; pmin = 1 / duty, at least 16.  nds is the
    largest downsampling at which pmin samples are no longer than pmin_s; octave o then covers [pmin, 2 pmin) * 2^o * nds * tsamp,
    and noct octaves reach pmax_s (at most 6, and fewer where the longest segment, 2^14 samples, does not hold two periods of the
    top octave: the range then ends early, see ffa_period).  nt is the longest segment, a power of two.  The widths run up to half
    the shortest period."""
    if not (0 < pmin_s <= pmax_s and tsamp > 0 and 0 < duty <= 0.5):
        raise ValueError("ffa_search: periods %r..%r s, windows of %r s, duty %r" % (pmin_s, pmax_s, tsamp, duty))
    pmin = max(16, int(round(1.0 / duty)))
    pmax = 2 * pmin - 1
    if 2 * pmax > 1 << 14:
        raise ValueError("ffa_search: a duty cycle of %r needs %d samples a period, more than a segment of 2^14 holds twice" % (duty, pmin))
    nds = int(math.floor(pmin_s / (pmin * tsamp) * (1 + 1e-12)))
    if nds < 1:
        raise ValueError("ffa_search: %d samples in a period of %r s are shorter than a window of %r s" % (pmin, pmin_s, tsamp))
    noct = max(1, int(math.ceil(math.log2(pmax_s / (pmin * nds * tsamp)) - 1e-12)))
    nt = 1 << 14
    while noct > 1 and (noct > 6 or 2 * pmax > nt >> (noct - 1)):
        noct -= 1
    nwidth = 1
    while nwidth < 8 and (1 << nwidth) <= pmin // 2:
        nwidth += 1
    return nds, nt, noct, pmin, pmax, nwidth


def ffa_candidates(plane, threshold, dms, nt, nds, tsamp):
    """plane: one record plane (as_records takes it); dms: the ndm trial DMs; nt, nds, tsamp: the segment length in samples, the
    windows per sample and the window length in seconds.  Records with p >= 0 and snr >= threshold (in sigma) qualify.  Per pair
    they are grouped over DM trials, octaves and widths: the best (among equals the lowest trial, octave, width) takes with it
    every other whose period lies within one period step -- the larger of the two records' spacings between neighbouring
    profiles, 2^o * nds * tsamp / (M - 1) -- of its own, then the best of the rest, and so on.  One candidate per group:
      dict(pair, idm, dm, octave, iw, width, p, i, j, M, period, snr, ntrial)
    width = 2^iw samples of the octave, period in seconds, ntrial the size of the group.  In order of pair, then period."""
    rec = as_records(plane)
    npair, ndm, noct, nwidth = rec.shape
    dms = np.asarray(dms, np.float64).reshape(-1)
    if dms.size != ndm:
        raise ValueError("ffa_search: %d DMs for a plane of %d trials" % (dms.size, ndm))
    out = []
    for pr in range(npair):
        with np.errstate(invalid='ignore'):
            hit = np.argwhere((rec['p'][pr] >= 0) & (rec['snr'][pr] >= float(threshold)))
        left = []
        for d, o, iw in hit:
            r = rec[pr, d, o, iw]
            M = ffa_rows(nt >> o, r['p'])
            if M < 2:
                raise ValueError("ffa_search: a base period of %d samples does not fit twice into octave %d of %d samples" % (r['p'], o, nt >> o))
            step = (1 << int(o)) * nds * float(tsamp) / (M - 1.0)
            left.append((-float(r['snr']), int(d), int(o), int(iw), ffa_period(int(r['p']), int(r['i']), M, int(o), nds, tsamp), step, M))
        left.sort()
        while left:
            s, d, o, iw, P, step, M = left[0]
            group = [e for e in left if abs(e[4] - P) <= max(step, e[5]) * (1 + 1e-9)]
            left = [e for e in left if e not in group]
            r = rec[pr, d, o, iw]
            out.append(dict(pair=pr, idm=d, dm=float(dms[d]), octave=o, iw=iw, width=1 << iw, p=int(r['p']), i=int(r['i']), j=int(r['j']), M=M,
                            period=P, snr=-s, ntrial=len(group)))
    out.sort(key=lambda c: (c['pair'], c['period']))
    return out
