"""Scenes for the tests of xengDetrend* (tests/test_detrend_*.py): dedispersed series [nwindows][npair][ndm][nprod] as
xengDedispRun writes them, and ways to cut a run into calls."""
import numpy as np

F = np.float32
K_MAD = float(F(1.4826))


def float_scene(seed, nwindows, npair, ndm, nprod, nblk, special=True):
    """Chi-squared-like floats per series (a sum of 8 squares) on a slow sinusoid (period 7.3 nblk) and a ramp, each series with an
    amplitude and a level of its own.  With `special` (and series enough): series 1 constant, series 2 of two values with heavy
    ties (one of them -0 and +0 mixed), series 3 with a NaN in block 2, series 4 with a +inf in block 1 and a -inf in block 3,
    series 5 of many equal values around a few outliers."""
    rng = np.random.default_rng(seed)
    nser = npair * ndm
    n = np.arange(nwindows)[:, None]
    level = rng.uniform(50, 500, nser)[None, :]
    z = (rng.standard_normal((nwindows, nser, 8)) ** 2).sum(axis=2) * level / 8
    z += level * (0.5 * np.sin(2 * np.pi * n / (7.3 * nblk) + rng.uniform(0, 6, nser)[None, :]) + 0.1 * n / nblk)
    x = np.zeros((nwindows, nser, nprod), F)
    if nprod == 1:
        x[..., 0] = z
    else:
        x[..., 0] = 0.6 * z
        x[..., 1] = 0.4 * z
        x[..., 2:] = rng.standard_normal((nwindows, nser, 2)) * 10
    if special:
        def put(s, v):
            if s < nser:
                x[:, s, 0] = v
                if nprod == 4:
                    x[:, s, 1] = 0
        put(1, 777.0)
        two = np.where(rng.random(nwindows) < 0.5, 0.0, 3.25).astype(F)
        two[(two == 0) & (rng.random(nwindows) < 0.5)] = -0.0
        put(2, two)
        eq = np.full(nwindows, 12.5, F)
        eq[rng.random(nwindows) < 0.1] = 99.0
        put(5, eq)
        if nser > 3 and nwindows > 2 * nblk + nblk // 3:
            x[2 * nblk + nblk // 3, 3, 0] = np.nan
        if nser > 4 and nwindows > nblk + 1:
            x[nblk + 1, 4, 0] = np.inf
        if nser > 4 and nwindows > 3 * nblk + 2:
            x[3 * nblk + 2, 4, 0] = -np.inf
    return x.reshape(nwindows, npair, ndm, nprod)


def integer_scene(seed, nwindows, npair, ndm, nprod):
    """Small integers with many ties, a step of 16 every 100 windows: with nblk a power of two and no normalisation every median,
    difference and product of the contract is exact in float32, and float64 arithmetic gives the same words."""
    rng = np.random.default_rng(seed)
    nser = npair * ndm
    z = rng.integers(0, 12, (nwindows, nser)) + 16 * (np.arange(nwindows)[:, None] // 100) + rng.integers(0, 40, nser)[None, :]
    x = np.zeros((nwindows, nser, nprod), F)
    if nprod == 1:
        x[..., 0] = z
    else:
        a = rng.integers(0, 5, (nwindows, nser))
        x[..., 0] = z - a
        x[..., 1] = a
        x[..., 2:] = rng.integers(-9, 9, (nwindows, nser, 2))
    return x.reshape(nwindows, npair, ndm, nprod)


def random_sizes(seed, total, most):
    """Calls of 1..most windows that sum to total."""
    rng = np.random.default_rng(seed)
    out = []
    while total:
        out.append(int(min(total, rng.integers(1, most + 1))))
        total -= out[-1]
    return out


def whole(total, nc):
    """Calls of nc windows and a shorter last one."""
    return [nc] * (total // nc) + ([total % nc] if total % nc else [])
