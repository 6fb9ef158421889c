"""Host side of BeamFold: the integer oscillator of a spin model, the rotations of a dispersion measure, and a small profile
statistic.  The library itself (xengFold*, include/xeng.h) takes integers and knows nothing of pulsars, time or the dispersion
constant.

The spin model is phi(t) = f0*(t - pepoch) + f1*(t - pepoch)**2 / 2 turns.  Sampled at t0 + m*tsamp it is a quadratic in m, which
the library's oscillator Phi(m) = phi0 + dphi*m + ddphi*m(m-1)/2 (turns * 2^64, wrapping) reproduces with
    phi0 = frac(phi(t0)),  dphi = f(t0)*tsamp + f1*tsamp**2/2,  ddphi = f1*tsamp**2,    f(t0) = f0 + f1*(t0 - pepoch),
each rounded once to a multiple of 2^-64 turns: after m windows the oscillator is within (1 + m + m(m-1)/2) * 2^-65 turns of the
model (1.4e-10 turns after 10^5 windows)."""
from fractions import Fraction

import numpy as np

from .dedisp import KDM

TWO64 = 1 << 64


def _round(x):
    """The integer nearest to the Fraction x (ties to even: Python's round)."""
    return int(round(x))


def fold_phase(f0, f1, pepoch, t0, tsamp):
    """(phi0, dphi, ddphi) as Python ints, in exact rational arithmetic from the inputs as given (floats stand for their exact
    binary values; ints and Fractions are taken as they are): phi0 and dphi in [0, 2^64), ddphi signed (it must fit an int64)."""
    f0, f1, pepoch, t0, tsamp = (Fraction(v) for v in (f0, f1, pepoch, t0, tsamp))
    if tsamp <= 0:
        raise ValueError("fold_phase: sampling time %r is not positive" % (tsamp,))
    dt = t0 - pepoch
    phi = f0 * dt + f1 * dt * dt / 2
    phi0 = _round((phi - (phi.numerator // phi.denominator)) * TWO64) % TWO64
    dphi = _round(((f0 + f1 * dt) * tsamp + f1 * tsamp * tsamp / 2) * TWO64) % TWO64
    ddphi = _round(f1 * tsamp * tsamp * TWO64)
    if not -(1 << 63) <= ddphi < (1 << 63):
        raise ValueError("fold_phase: f1 * tsamp^2 = %g turns per window^2 does not fit the oscillator" % float(f1 * tsamp * tsamp))
    return phi0, dphi, ddphi


def fold_rotations(freqs_hz, dm, f_spin, nbin, f_ref_hz=None):
    """int32 [nfine]: rint(KDM * dm * (f**-2 - f_ref**-2) * f_spin * nbin) mod nbin in float64, f in MHz -- the bins by which the
    pulse in channel f trails the pulse at f_ref (the highest channel by default, as dm_delays has it), which a dump undoes:
    out[b] takes channel q's bin (b + rot[q]) mod nbin."""
    f = np.asarray(freqs_hz, np.float64).reshape(-1) * 1e-6
    if f.size == 0 or not (np.all(np.isfinite(f)) and np.all(f > 0)):
        raise ValueError("fold_rotations: frequencies must be positive and finite")
    if not (np.isfinite(dm) and np.isfinite(f_spin) and f_spin > 0):
        raise ValueError("fold_rotations: DM %r must be finite and the spin frequency %r positive" % (dm, f_spin))
    if not (isinstance(nbin, (int, np.integer)) and nbin > 0):
        raise ValueError("fold_rotations: nbin %r is not a positive integer" % (nbin,))
    f_ref = f.max() if f_ref_hz is None else float(f_ref_hz) * 1e-6
    if not (np.isfinite(f_ref) and f_ref > 0):
        raise ValueError("fold_rotations: reference frequency %r is not positive" % (f_ref_hz,))
    r = np.rint(KDM * float(dm) * (f ** -2 - f_ref ** -2) * float(f_spin) * int(nbin))
    return np.mod(r, int(nbin)).astype(np.int32)


def fold_rotations_coherent(freqs_hz, coarse_freqs_hz, dm, dm_coh, f_spin, nbin, f_ref_hz=None):
    """fold_rotations behind BeamCoherentDedisperse, which has aligned the fine channels of a coarse channel to its centre at the DM
    dm_coh already: int32 [nfine],
        rint(KDM * (dm * (f_c**-2 - f_ref**-2) + (dm - dm_coh) * (f**-2 - f_c**-2)) * f_spin * nbin) mod nbin
    in float64, f the fine channel (freqs_hz), f_c the centre of its coarse channel (coarse_freqs_hz, one per fine channel), f_ref
    the highest fine channel by default.  dm_coh = dm leaves the delays between the coarse channels only; dm_coh = 0 is
    fold_rotations to within the rounding of one sum."""
    f = np.asarray(freqs_hz, np.float64).reshape(-1) * 1e-6
    fc = np.asarray(coarse_freqs_hz, np.float64).reshape(-1) * 1e-6
    if f.size == 0 or fc.shape != f.shape or not (np.all(np.isfinite(f)) and np.all(f > 0) and np.all(np.isfinite(fc)) and np.all(fc > 0)):
        raise ValueError("fold_rotations_coherent: frequencies must be positive and finite, one coarse centre per fine channel")
    if not (np.isfinite(dm) and np.isfinite(dm_coh) and np.isfinite(f_spin) and f_spin > 0):
        raise ValueError("fold_rotations_coherent: DMs %r, %r must be finite and the spin frequency %r positive" % (dm, dm_coh, f_spin))
    if not (isinstance(nbin, (int, np.integer)) and nbin > 0):
        raise ValueError("fold_rotations_coherent: nbin %r is not a positive integer" % (nbin,))
    f_ref = f.max() if f_ref_hz is None else float(f_ref_hz) * 1e-6
    if not (np.isfinite(f_ref) and f_ref > 0):
        raise ValueError("fold_rotations_coherent: reference frequency %r is not positive" % (f_ref_hz,))
    r = np.rint((KDM * float(dm) * (fc ** -2 - f_ref ** -2) + KDM * (float(dm) - float(dm_coh)) * (f ** -2 - fc ** -2)) * float(f_spin) * int(nbin))
    return np.mod(r, int(nbin)).astype(np.int32)


def profile_snr(profile):
    """Of a profile [nbin]: dict(mean, sigma, peak, bin, snr).  mean and sigma (population) come from the quietest half of the
    bins: the window of nbin // 2 consecutive bins, cyclically, with the smallest sum (the first such window).  peak is the
    largest value, bin its (first) index, snr = (peak - mean) / sigma, inf where sigma is 0 and the peak stands above the mean,
    0 where it does not."""
    x = np.asarray(profile, np.float64).reshape(-1)
    nbin = x.size
    if nbin < 2 or not np.all(np.isfinite(x)):
        raise ValueError("profile_snr: a profile of at least 2 finite bins is needed")
    h = nbin // 2
    c = np.concatenate([[0.0], np.cumsum(np.concatenate([x, x[:h]]))])
    start = int(np.argmin(c[h:h + nbin] - c[:nbin]))
    off = x[(start + np.arange(h)) % nbin]
    mean, sigma = float(off.mean()), float(off.std())
    b = int(np.argmax(x))
    peak = float(x[b])
    if sigma > 0:
        snr = (peak - mean) / sigma
    else:
        snr = float('inf') if peak > mean else 0.0
    return dict(mean=mean, sigma=sigma, peak=peak, bin=b, snr=snr)
