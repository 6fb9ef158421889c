"""Scenes for the tests of xengCutout* (tests/test_cutout_*.py): power beams [nwindows][npair][nfine][4] as xengDedispRun takes them,
delay tables, a planted dispersed pulse, and ways to cut a run into calls."""
import numpy as np

from tests.detrend_cases import random_sizes, whole  # noqa: F401

F = np.float32
K_MAD = float(F(1.4826))


def table(ndmf, nfine, S):
    """i32[ndmf][nfine]: quadratic in the channel as a cold-plasma sweep is, 0 at the top channel and at trial 0, S at (ndmf-1, 0)."""
    d = np.arange(ndmf)[:, None] / float(max(ndmf - 1, 1))
    u = (nfine - 1 - np.arange(nfine))[None, :] / float(max(nfine - 1, 1))
    if nfine == 1:
        u = np.ones((1, 1))
    return np.ascontiguousarray(np.rint(S * d * u * u), np.int32)


def float_scene(seed, nwindows, npair, nfine):
    """Chi-squared-like floats (a sum of 4 squares per hand) with a level per channel spread over a factor of 100, the cross words
    of either sign: no sum of them is exact, and the order of the contract shows in the last bits."""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(0, 2, (1, 1, nfine))
    x = np.zeros((nwindows, npair, nfine, 4), F)
    x[..., 0] = (rng.standard_normal((nwindows, npair, nfine, 4)) ** 2).sum(axis=-1) * level
    x[..., 1] = (rng.standard_normal((nwindows, npair, nfine, 4)) ** 2).sum(axis=-1) * level * 0.7
    x[..., 2:] = rng.standard_normal((nwindows, npair, nfine, 2)) * level[..., None]
    return x


def integer_scene(seed, nwindows, npair, nfine, top=20):
    """Seeded integer noise, uniform in 0..top-1 per hand; the cross words are small integers of either sign."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, top, (nwindows, npair, nfine, 4)).astype(F)
    x[..., 2:] -= top // 2
    return x


def plant(x, pair, delays_row, n_top, amp, width=1):
    """Adds a pulse of `amp` per channel (on XX) and `width` windows that reaches the top of the band at window n_top and channel
    q delays_row[q] windows later."""
    for q, s in enumerate(np.asarray(delays_row)):
        x[n_top + int(s):n_top + int(s) + width, pair, q, 0] += amp
    return x
