"""Host side of the candidate folder (xengCandfold*, include/xeng.h "Folding of search candidates"): the records, the trial table of
period / period-derivative offsets, the integer shift rule as numpy states it, the oscillators of a list of search candidates, and
what a record says about a candidate's frequency and its derivative.

A completed segment gives ncand_max records of 16 bytes {f32 S, f32 S0, i16 it, i16 iw, i16 j, i16 pad} (CANDFOLD_RECORD) and then
f32 [ncand_max][nbin] best profiles.  S is the largest score over the trials it, boxcar widths 2^iw and phase bins j; S0 what the
unrefined fold (the first trial with d1 = d2 = 0) found; it = iw = j = -1 where nothing qualified.

A trial (d1, d2), in sixteenths of a bin, shifts sub-integration s of nsub by r(s) = d1 * tau + d2 * (2 tau)^2 sixteenths, rounded
half up to whole bins, tau = (s + 1/2) / nsub - 1/2 the sub-integration's centre in units of the segment, from its middle:
d1 is the drift across the whole segment, d2 the bow at either end.  candfold_refined derives what that means for the spin
frequency.  Pure numpy.  Not built: DM refinement (it needs the channelised data, which BeamFold has), interpolated (sub-bin)
shifts, a chi^2 statistic, plots or archive output, and a second derivative (jerk)."""
import math
from fractions import Fraction

import numpy as np

from .accel_search import C_LIGHT
from .fold import fold_phase

CANDFOLD_RECORD = np.dtype([('S', '<f4'), ('S0', '<f4'), ('it', '<i2'), ('iw', '<i2'), ('j', '<i2'), ('pad', '<i2')])
MAX_TRIALS = 4096
MAX_OFFSET = 1 << 20


def as_records_candfold(span, ncand_max, nbin):
    """(records CANDFOLD_RECORD [ncand_max], best profiles float32 [ncand_max][nbin]) from the bytes (or 32-bit words) of one output
    span of xengCandfoldRun."""
    a = np.ascontiguousarray(span).reshape(-1).view(np.uint8)
    nrec = ncand_max * CANDFOLD_RECORD.itemsize
    if a.size != nrec + ncand_max * nbin * 4:
        raise ValueError("cand_fold: %d bytes are not %d records and %d profiles of %d bins" % (a.size, ncand_max, ncand_max, nbin))
    return a[:nrec].view(CANDFOLD_RECORD), a[nrec:].view(np.float32).reshape(ncand_max, nbin)


def candfold_trials(ndrift, ncurve, step=16):
    """(d1, d2), int32 each: the (2 ndrift + 1) x (2 ncurve + 1) grid d1 = i * step, d2 = j * step (sixteenths of a bin; step = 16 is
    one bin of drift over the segment, one bin of bow at its ends), ordered centre first: (0, 0), then by |i| + |j|, then by |j|,
    |i|, and the positive before the negative, i before j.  The library takes the first of equal scores, so ties prefer the
    unrefined fold and then the smaller correction."""
    ndrift, ncurve, step = int(ndrift), int(ncurve), int(step)
    if ndrift < 0 or ncurve < 0 or step < 1:
        raise ValueError("candfold_trials: ndrift=%r ncurve=%r step=%r" % (ndrift, ncurve, step))
    if (2 * ndrift + 1) * (2 * ncurve + 1) > MAX_TRIALS or max(ndrift, ncurve) * step > MAX_OFFSET:
        raise ValueError("candfold_trials: %d x %d trials of step %d: more than %d, or beyond 2^20" % (2 * ndrift + 1, 2 * ncurve + 1, step, MAX_TRIALS))
    grid = [(i, j) for i in range(-ndrift, ndrift + 1) for j in range(-ncurve, ncurve + 1)]
    grid.sort(key=lambda ij: (abs(ij[0]) + abs(ij[1]), abs(ij[1]), abs(ij[0]), ij[0] < 0, ij[1] < 0))
    g = np.array(grid, np.int64).reshape(-1, 2) * step
    return g[:, 0].astype(np.int32), g[:, 1].astype(np.int32)


def candfold_shifts(d1, d2, nsub, nbin=None):
    """int64 [ntrial][nsub]: r_t(s) = floor((2 N + D) / (2 D)) with u = 2 s + 1 - nsub, N = d1[t] * u * nsub + 2 * d2[t] * u^2 and
    D = 32 nsub^2, in 64-bit integers with floor division -- the library's rule word for word (|N| < 2^40).  With nbin, reduced
    into 0 .. nbin - 1, which is what the sums over the sub-integrations use."""
    d1, d2 = np.asarray(d1, np.int64).reshape(-1), np.asarray(d2, np.int64).reshape(-1)
    nsub = int(nsub)
    if d1.shape != d2.shape or nsub < 1 or max(np.abs(d1).max(initial=0), np.abs(d2).max(initial=0)) > MAX_OFFSET:
        raise ValueError("candfold_shifts: d1 %r, d2 %r, nsub %r" % (d1.shape, d2.shape, nsub))
    u = 2 * np.arange(nsub, dtype=np.int64) + 1 - nsub
    N = d1[:, None] * u[None, :] * nsub + 2 * d2[:, None] * (u * u)[None, :]
    D = np.int64(32 * nsub * nsub)
    r = (2 * N + D) // (2 * D)
    return r if nbin is None else r % np.int64(nbin)


def candfold_gains(nbin, nwidth):
    """float32 [nwidth]: (float)(1 / sqrt(w (1 - w / nbin))), w = 2^iw, in float64 and rounded once.  A boxcar of w bins less its
    share w / nbin of the whole profile has variance w (1 - w / nbin) times a bin's: the scores of all widths are in units of one
    bin's noise."""
    nbin, nwidth = int(nbin), int(nwidth)
    if nwidth < 1 or 1 << (nwidth - 1) > nbin // 2:
        raise ValueError("candfold_gains: %d widths, not 1 or more with 2^(nwidth-1) <= nbin/2 = %d" % (nwidth, nbin // 2))
    return np.array([1.0 / math.sqrt((1 << iw) * (1.0 - (1 << iw) / nbin)) for iw in range(nwidth)], np.float64).astype(np.float32)


def candfold_oscillators(cands, t0, tsamp, nt):
    """The oscillators of search candidates: dicts of period_candidates[_long], accel_candidates, ffa_candidates or period_sift, each
    with `pair`, `idm` and `freq` (Hz) or `period` (s).  Times are in seconds from the first window of the segment of nt windows
    the candidates were found in; t0 is the time of the window the oscillators start at (m = 0: the window at which
    xengCandfoldSetCandidates takes effect), so t0 >= nt * tsamp folds the segments that follow the search's.

    A candidate without `accel` folds at its frequency with f1 = 0.  An accel_candidates entry was found in the series read
    through n' -> n' + alpha n' (n' - nt) (accel_search.py), where it is periodic at `freq`: its phase at the true window n is, to
    first order in alpha, freq * tsamp * (n - alpha n (n - nt)), so its spin frequency there is freq * (1 - alpha (2 n - nt)).
    At mid-segment, n = nt / 2, that is `freq` itself, and its derivative is -2 alpha freq / tsamp = -accel * freq / c, because
    alpha = accel * tsamp / (2 c).  So pepoch = nt * tsamp / 2, f0 = freq and f1 = -accel * freq / c; a source accelerating away
    (accel > 0) spins down.

    Returns a list of dicts(pair, idm, f0, f1, pepoch, t0, phi0, dphi, ddphi), the last three fold_phase's integers (exact
    rational arithmetic on the floats as given)."""
    t0, tsamp, nt = float(t0), float(tsamp), int(nt)
    if not (tsamp > 0 and nt > 0 and math.isfinite(t0)):
        raise ValueError("candfold_oscillators: t0=%r tsamp=%r nt=%r" % (t0, tsamp, nt))
    pepoch = Fraction(nt) * Fraction(tsamp) / 2
    out = []
    for c in cands:
        if 'pair' not in c or 'idm' not in c or not ('freq' in c or 'period' in c):
            raise ValueError("candfold_oscillators: a candidate needs pair, idm and freq or period: %r" % (sorted(c),))
        f0 = float(c['freq']) if 'freq' in c else 1.0 / float(c['period'])
        if not (math.isfinite(f0) and f0 > 0):
            raise ValueError("candfold_oscillators: frequency %r" % (f0,))
        f1 = -float(c['accel']) * f0 / C_LIGHT if 'accel' in c else 0.0
        phi0, dphi, ddphi = fold_phase(f0, f1, pepoch, t0, tsamp)
        out.append(dict(pair=int(c['pair']), idm=int(c['idm']), f0=f0, f1=f1, pepoch=float(pepoch), t0=t0, phi0=phi0, dphi=dphi, ddphi=ddphi))
    return out


def candfold_refined(cand, record, d1, d2, nbin, nt, tsamp, segment=0):
    """(f0, f1) of a folded candidate at the middle of fold segment `segment` (counted from the one the oscillator started in), from
    its record.  cand: a dict of candfold_oscillators; nt: the windows of a FOLD segment, T = nt * tsamp.

    The refinement adds cube row s at bin b - r(s) into bin b: it lines up a pulse that sits at bin b0 - r(s) in sub-integration s,
    one that arrives earlier and earlier against the fold as r grows.  A source whose phase runs ahead of the fold's by
    dphi(t) = df (t - tm) + df1 (t - tm)^2 / 2 turns (tm the middle of the segment) lands, when its own phase is whole, where
    the fold's phase is -dphi: at bin b0 - nbin * dphi(t).  So r(s) = nbin * dphi(t_s) bins.  The trial's
    r = (d1 tau + d2 (2 tau)^2) / 16 bins with tau = (t - tm) / T gives df = d1 / (16 nbin T) and df1 / 2 = 4 d2 / (16 nbin T^2):
        f0 = f_fold(tm) + d1 / (16 nbin T),    f1 = f1_fold + d2 / (2 nbin T^2).
    A positive d1 is a frequency above the fold's.  One grid step `step` of candfold_trials is step / (16 nbin T) Hz and
    step / (2 nbin T^2) Hz/s.  An empty record (it < 0) returns the fold's own values."""
    T = int(nt) * float(tsamp)
    tm = float(cand['t0']) + (int(segment) + 0.5) * T
    f0 = float(cand['f0']) + float(cand['f1']) * (tm - float(cand['pepoch']))
    f1 = float(cand['f1'])
    it = int(record['it'])
    if it < 0:
        return f0, f1
    return f0 + float(d1[it]) / (16.0 * nbin * T), f1 + float(d2[it]) / (2.0 * nbin * T * T)


def candfold_sigma(cube, hits):
    """float64 [ncand]: a robust per-window sigma of each candidate's series from its folded cube [ncand][nsub][nbin] and hits.  A
    cell that h windows went into holds their sum: its mean less the median of the means, times sqrt(h), scatters by sigma.
    1.4826 times the median of the absolute values (the MAD of a normal distribution); cells without hits and cells that are
    not finite do not count; 0 where nothing counts.  A pulse fills few cells and leaves the median alone."""
    cube, hits = np.asarray(cube, np.float64), np.asarray(hits, np.float64)
    if cube.shape != hits.shape or cube.ndim != 3:
        raise ValueError("candfold_sigma: cube %r, hits %r" % (cube.shape, hits.shape))
    out = np.zeros(cube.shape[0])
    for c in range(cube.shape[0]):
        ok = (hits[c] > 0) & np.isfinite(cube[c])
        if ok.any():
            mean = cube[c][ok] / hits[c][ok]
            out[c] = 1.4826 * np.median(np.abs((mean - np.median(mean)) * np.sqrt(hits[c][ok])))
    return out


def candfold_candidates(records, profiles, oscs, sigma, d1, d2, nbin, nt, tsamp, threshold, segment=0):
    """The folded candidates above a threshold.  A profile bin is the mean of about nt / nbin windows, so its noise is
    sigma / sqrt(nt / nbin), and candfold_gains puts every width's score into units of it: snr = S * sqrt(nt / nbin) / sigma.
    Per candidate c < len(oscs) with it >= 0, sigma[c] > 0 and snr >= threshold:
      dict(cand, pair, idm, snr, snr0, it, iw, width, j, d1, d2, f0, f1, period, profile)
    snr0 the same of S0, f0 / f1 from candfold_refined at the middle of fold segment `segment`, profile the best profile."""
    rec = np.asarray(records)
    if rec.dtype != CANDFOLD_RECORD or rec.ndim != 1 or len(oscs) > rec.size:
        raise ValueError("candfold_candidates: %r records for %d candidates" % (rec.shape, len(oscs)))
    prof = np.asarray(profiles, np.float32).reshape(rec.size, nbin)
    sigma = np.asarray(sigma, np.float64).reshape(-1)
    out = []
    for c, o in enumerate(oscs):
        r = rec[c]
        if r['it'] < 0 or not sigma[c] > 0:
            continue
        k = math.sqrt(nt / float(nbin)) / sigma[c]
        snr = float(r['S']) * k
        if not snr >= float(threshold):
            continue
        f0, f1 = candfold_refined(o, r, d1, d2, nbin, nt, tsamp, segment)
        out.append(dict(cand=c, pair=o['pair'], idm=o['idm'], snr=snr, snr0=float(r['S0']) * k, it=int(r['it']), iw=int(r['iw']), width=1 << int(r['iw']),
                        j=int(r['j']), d1=int(d1[r['it']]), d2=int(d2[r['it']]), f0=f0, f1=f1, period=1.0 / f0, profile=prof[c].copy()))
    return out
