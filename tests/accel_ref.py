"""Restatement of the acceleration search (xengAccel*), written from the contract in include/xeng.h, "Acceleration search of the
long-segment spectra": the index rule (accel_index), then tests/plong_ref.py's stacks / harmonic_records (nstack = 1) on the series
read through it, then the best-over-trials rule.  In float32 it is an independent evaluation of the same contract (what the
planted-source tests use); the exact tests compare the device with xengPlong* itself."""
import numpy as np

from tests.plong_ref import RECORD, harmonic_records, plane_of, stacks

ACCEL_RECORD = np.dtype([('H', '<f4'), ('k', '<i4'), ('ia', '<i4'), ('H0', '<f4')])


def accel_index(alpha, nt):
    """n + s(n), s(n) = rint(alpha * float64(n * (n - nt))): an exact integer product, one float64 multiply, half to even."""
    n = np.arange(nt, dtype=np.int64)
    q = n * (n - nt)
    assert np.abs(q).max() < 1 << 40
    return n + np.rint(np.float64(alpha) * q.astype(np.float64)).astype(np.int64)


def resample(z, alpha, nt):
    """z [nt][...] read through trial alpha's map: z_a[n] = z[n + s(n)]."""
    idx = accel_index(alpha, nt)
    assert idx.min() >= 0 and idx.max() < nt and (np.diff(idx) >= 0).all()
    return np.asarray(z)[idx]


def trial_records(z, nt, nlevel, nwhite, kedge, alphas, keep=None, dtype=np.float32):
    """z [nt][nser], one segment: the RECORD array [ntrial][nser][nlevel][nband] of the trials, each the banded records of the
    whitened spectrum of the resampled segment."""
    out = []
    for alpha in alphas:
        (A, _), = stacks(resample(z, alpha, nt), nt, 1, nwhite, keep, dtype)
        out.append(plane_of(harmonic_records(A, nlevel, kedge)))
    return np.stack(out)


def best_over_trials(trec, alphas):
    """The plane of the trial records trec [ntrial][...]: per record the trials in ascending order, the larger H wins (so the
    smaller ia among equals), a NaN or an empty record never; {+0, -1, -1, H0} where nothing qualified.  H0 is the H of the first
    trial whose alpha is 0.0, +0 without one or where that trial's record is empty."""
    trec = np.asarray(trec)
    assert trec.dtype == RECORD
    out = np.zeros(trec.shape[1:], ACCEL_RECORD)
    out['k'], out['ia'] = -1, -1
    for a in range(trec.shape[0]):
        ok = (trec[a]['k'] >= 0) & ~np.isnan(trec[a]['H'])
        with np.errstate(invalid='ignore'):
            take = ok & ((out['k'] < 0) | (trec[a]['H'] > out['H']))
        out['H'] = np.where(take, trec[a]['H'], out['H'])
        out['k'] = np.where(take, trec[a]['k'], out['k'])
        out['ia'] = np.where(take, a, out['ia'])
    zero = [a for a, al in enumerate(alphas) if al == 0.0]
    if zero:
        t = trec[zero[0]]
        out['H0'] = np.where((t['k'] >= 0) & ~np.isnan(t['H']), t['H'], np.float32(0.0))
    return out


def planted_case(shift, seed=5, nt=1 << 15):
    """One series of chi^2 noise with mean / sigma = 55 and pulses of about 10 sigma, one window wide, emitted every 37.3 windows
    and received at rint(tau + a0 tau (tau - nt)) with a0 = -4 shift / nt^2: the map of trial a0 reads window n at
    n + a0 n (n - nt), `shift` windows further on at the middle of the segment, and so undoes it.  17 trials with mid-segment
    shifts of -32 .. 32 in steps of 4, the planted one among them.  Returns (z [nt][1] float32, alphas, the planted trial's index)."""
    rng = np.random.default_rng(seed)
    dof = 2 * 55 ** 2
    z = rng.chisquare(dof, nt)
    sigma = np.sqrt(2.0 * dof)
    a0 = -4.0 * shift / float(nt) ** 2
    tau = np.arange(5.0, nt - 1, 37.3)
    at = np.rint(tau + a0 * tau * (tau - nt)).astype(np.int64)
    at = at[(at >= 0) & (at < nt)]
    np.add.at(z, at, 10.0 * sigma)
    shifts = np.arange(-32, 33, 4)
    alphas = -4.0 * shifts / float(nt) ** 2
    return z.astype(np.float32)[:, None], alphas, int(np.flatnonzero(shifts == shift)[0])
