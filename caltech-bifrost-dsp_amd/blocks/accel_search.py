"""Host side of the acceleration search (xengAccel*, include/xeng.h "Acceleration search of the long-segment spectra"): the record
plane, the trial table, the index rule as numpy states it, and the thresholding of a plane.

A plane is [npair][ndm][nlevel][nband] records of four 32-bit words {f32 H, i32 k, i32 ia, f32 H0} (ACCEL_RECORD): per series,
harmonic level and band of fundamental frequency the largest harmonic sum over all trial accelerations, the bin k of its top
harmonic, the trial ia it was found in, and H0, what the unaccelerated trial (alpha == 0) found in the same record; k = ia = -1
where nothing qualified.

Trial a reads the segment of nt windows through z_a[n] = z[n + s_a(n)], s_a(n) = rint(alpha[a] * n * (n - nt)) (accel_index).  A
source with a constant acceleration `acc` (m/s^2) along the line of sight arrives late by acc t^2 / 2c, that is by
acc * tsamp / (2c) * n^2 windows at window n; n^2 = n (n - nt) + nt * n, and the part linear in n is a constant Doppler shift, a
slightly different period, which the search finds as it is.  So alpha = acc * tsamp / (2c) (accel_alpha), and the sign
convention is: alpha > 0 (acc > 0) undoes a source accelerating AWAY from the observer, alpha < 0 one accelerating towards it.
Over the segment T = nt * tsamp the uncorrected signal drifts by z = acc T^2 f / c = 2 alpha nt k bins at bin k.

Not built: jerk trials, a Fourier-domain (correlation) search, interpolating resampling (the nearest sample is taken), stacking
of segments.  Pure numpy."""
import math

import numpy as np

from .period_search import RECORD, band_bins, period_candidates_long

ACCEL_RECORD = np.dtype([('H', '<f4'), ('k', '<i4'), ('ia', '<i4'), ('H0', '<f4')])
C_LIGHT = 299792458.0       # m/s
MAX_TRIALS = 256


def as_records_accel(plane, npair=None, ndm=None, nlevel=None, nband=None):
    """A plane as an ACCEL_RECORD array [npair][ndm][nlevel][nband]: from such an array, or from raw bytes / 32-bit words with the
    four sizes."""
    a = np.asarray(plane)
    if a.dtype != ACCEL_RECORD:
        if None in (npair, ndm, nlevel, nband):
            raise ValueError("accel_search: a raw plane needs npair, ndm, nlevel and nband")
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size != npair * ndm * nlevel * nband * ACCEL_RECORD.itemsize:
            raise ValueError("accel_search: %d bytes are not %d x %d x %d x %d records" % (a.size, npair, ndm, nlevel, nband))
        a = a.view(ACCEL_RECORD).reshape(npair, ndm, nlevel, nband)
    if a.ndim != 4:
        raise ValueError("accel_search: a plane is [npair][ndm][nlevel][nband] records, not %r" % (a.shape,))
    return a


def accel_alpha(acc, tsamp):
    """The index-map coefficient of an acceleration acc (m/s^2; a number or an array) at a window length tsamp (s):
    acc * tsamp / (2c).  alpha > 0 undoes a source accelerating away."""
    a = np.asarray(acc, np.float64) * float(tsamp) / (2.0 * C_LIGHT)
    return a if a.ndim else float(a)


def accel_of(alpha, tsamp):
    """The acceleration (m/s^2) a coefficient alpha stands for: the inverse of accel_alpha."""
    a = np.asarray(alpha, np.float64) * (2.0 * C_LIGHT) / float(tsamp)
    return a if a.ndim else float(a)


def accel_index(alpha, nt):
    """int64 [nt]: n + s(n), where trial alpha reads window n.  s(n) = rint(alpha * float64(n * (n - nt))): the product of the
    integers is exact (below 2^40), then one float64 multiply and a rounding to nearest even, each an IEEE operation -- the
    library's rule word for word.  |alpha| * nt > 0.5 would leave the segment: ValueError."""
    alpha, nt = float(alpha), int(nt)
    if not math.isfinite(alpha) or abs(alpha) * nt > 0.5:
        raise ValueError("accel_index: alpha %r is not finite or above 0.5 / nt = %r" % (alpha, 0.5 / nt))
    n = np.arange(nt, dtype=np.int64)
    return n + np.rint(np.float64(alpha) * (n * (n - nt)).astype(np.float64)).astype(np.int64)


def accel_trials(amax, tsamp, nt, fmax, zstep=1.0):
    """The trial table for accelerations up to |amax| (m/s^2): float64 alphas, symmetric about 0 and with 0.0 itself in the middle,
    i * da for i = -n .. n with da = zstep * c / (T^2 * fmax), T = nt * tsamp -- neighbouring trials differ by zstep bins of drift
    at the frequency fmax (Hz) -- and n = ceil(amax / da).  More than 256 trials, or a trial beyond the limit of the index map
    (|alpha| * nt <= 0.5): ValueError."""
    amax, tsamp, nt, fmax, zstep = float(amax), float(tsamp), int(nt), float(fmax), float(zstep)
    if not (math.isfinite(amax) and amax >= 0 and tsamp > 0 and nt > 0 and fmax > 0 and zstep > 0):
        raise ValueError("accel_trials: amax=%r tsamp=%r nt=%r fmax=%r zstep=%r" % (amax, tsamp, nt, fmax, zstep))
    T = nt * tsamp
    da = zstep * C_LIGHT / (T * T * fmax)
    n = int(math.ceil(amax / da - 1e-12))
    if 2 * n + 1 > MAX_TRIALS:
        raise ValueError("accel_trials: %d trials of %.4g m/s^2 up to %.4g m/s^2, more than %d: raise zstep or lower fmax" % (2 * n + 1, da, amax, MAX_TRIALS))
    alphas = accel_alpha(da * np.arange(-n, n + 1, dtype=np.float64), tsamp)
    if np.abs(alphas).max() * nt > 0.5:
        raise ValueError("accel_trials: %.4g m/s^2 is beyond c / T = %.4g m/s^2, the limit of the index map" % (da * n, C_LIGHT / T))
    return alphas


def accel_candidates(plane, threshold, dms, nt, tsamp, kedge, alphas, ntrials=None):
    """period_candidates_long (nstack = 1) for a plane of the acceleration search made with the edges kedge and the trials alphas.
    The number of independent trials of the false-alarm probability is the bins searched (default: counted exactly) times the
    number of acceleration trials.  Every candidate carries, beside period_candidates_long's keys,
      ia, accel (m/s^2, accel_of its trial), H0 (what the unaccelerated trial found in the record) and z (the bins its top
      harmonic would have drifted over the segment, 2 alpha nt k).
    period_sift takes the list unchanged."""
    rec = as_records_accel(plane)
    alphas = np.asarray(alphas, np.float64).reshape(-1)
    if not 1 <= alphas.size <= MAX_TRIALS:
        raise ValueError("accel_search: %d trials, not 1 to %d" % (alphas.size, MAX_TRIALS))
    if (rec['ia'] >= alphas.size).any():
        raise ValueError("accel_search: the plane names trial %d of %d" % (int(rec['ia'].max()), alphas.size))
    nlevel = rec.shape[2]
    if ntrials is None:
        ntrials = sum(sum(band_bins(kedge, lv, nt)) for lv in range(nlevel))
    hk = np.zeros(rec.shape, RECORD)
    hk['H'], hk['k'] = rec['H'], rec['k']
    out = period_candidates_long(hk, threshold, dms, nt, 1, tsamp, kedge, ntrials=float(ntrials) * alphas.size)
    for c in out:
        r = rec[c['pair'], c['idm'], c['h'].bit_length() - 1, c['band']]
        ia = int(r['ia'])
        c.update(ia=ia, accel=float(accel_of(alphas[ia], tsamp)), H0=float(r['H0']), z=float(2.0 * alphas[ia] * nt * c['k']))
    return out
