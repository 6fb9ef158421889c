"""The generalised spectral-kurtosis estimator (Nita & Gary 2010, MNRAS 406, L60) on UpchanSpectra's output, and the
incoherent beam.  Host side, numpy, float64; no device work.

UpchanSpectra gives, per input and fine channel, S1 = sum |X|^2 and S2 = sum |X|^4 over a window of M = nframe_sum frames
(f32 [2][nchan][nupchan][ninput], plane 0 = S1, plane 1 = S2).  For raw power samples (no averaging before the sums, d = 1)

    SK = (M + 1) / (M - 1) * (M * S2 / S1^2 - 1),    E[SK] = 1 for Gaussian noise,  Var[SK] = 4 M^2 / ((M - 1)(M + 2)(M + 3))

A steady narrow-band signal (a carrier) pulls SK below 1, an intermittent one (a burst with a duty cycle under one half)
pushes it above 1.
"""
import numpy as np


def spectral_kurtosis(s1, s2, m):
    """SK of every cell, float64 in the shape of s1; cells with s1 == 0 (a dead input, a window of zeros) give NaN."""
    if m < 2:
        raise ValueError("spectral_kurtosis: a window of %r frames has no estimator (M >= 2)" % (m,))
    s1 = np.asarray(s1, np.float64)
    s2 = np.asarray(s2, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        sk = (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0)
    return np.where(s1 == 0, np.nan, sk)


def sk_variance(m):
    """Var[SK] of Gaussian noise over M frames: 4 M^2 / ((M - 1)(M + 2)(M + 3))."""
    m = float(m)
    return 4.0 * m * m / ((m - 1.0) * (m + 2.0) * (m + 3.0))


def sk_limits(m, nsigma=3.0):
    """(lower, upper) = 1 -/+ nsigma * sqrt(Var[SK]): symmetric limits from the estimator's variance.

    The distribution of SK is skewed to the right, so `nsigma` does not carry the Gaussian tail probability: at nsigma = 3
    clean Gaussian noise is flagged at 1.3 % of cells for M = 30 (where the lower limit is negative and never met: all of it
    is the upper tail) and at 0.5 % for M = 750, not at 0.27 % (seeded float64 simulations of 4e5 and 1e5 cells; 4-bit
    quantised data through a 32-point FFT at M = 30: 1.35 %).  The asymmetric limits from a Pearson type IV fit, which the
    literature uses to set a chosen false-alarm rate, are not implemented here."""
    if m < 2:
        raise ValueError("sk_limits: a window of %r frames has no estimator (M >= 2)" % (m,))
    d = float(nsigma) * np.sqrt(sk_variance(m))
    return 1.0 - d, 1.0 + d


def sk_flags(s1, s2, m, nsigma=3.0):
    """True where SK lies outside sk_limits(m, nsigma) or is NaN; bool in the shape of s1."""
    sk = spectral_kurtosis(s1, s2, m)
    lo, hi = sk_limits(m, nsigma)
    with np.errstate(invalid='ignore'):
        return ~((sk >= lo) & (sk <= hi))


def incoherent_beam(s1, npol=2, flags=None):
    """The sum of S1 over stands, per pol and fine channel.  s1 [..., ninput] with input = stand * npol + pol (the sequence
    header's input_to_ant), flags (optional) bool in the shape of s1, True = leave the cell out.  Returns (beam, count), both
    [..., npol]: float64 sums and the number of cells that went into each."""
    s1 = np.asarray(s1, np.float64)
    ninput = s1.shape[-1]
    if npol <= 0 or ninput % npol:
        raise ValueError("incoherent_beam: %d inputs are not whole stands of %r pols" % (ninput, npol))
    keep = np.ones(s1.shape, bool) if flags is None else ~np.asarray(flags, bool)
    if keep.shape != s1.shape:
        raise ValueError("incoherent_beam: flags of shape %r for S1 of shape %r" % (keep.shape, s1.shape))
    shape = s1.shape[:-1] + (ninput // npol, npol)
    beam = np.where(keep, s1, 0.0).reshape(shape).sum(axis=-2)
    return beam, keep.reshape(shape).sum(axis=-2)
