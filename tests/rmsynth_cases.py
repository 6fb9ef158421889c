"""Scenes, tables and masks shared by the tests of xengRmsynth* (tests/test_rmsynth_*.py): seeded, small, and the same on the CPU
and on the GPU."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks import rm_lambda2, rm_table

F = np.float32
NCHG = 70
FREQS = np.linspace(60e6, 79.6e6, NCHG)         # 70 groups over 60 to 79.6 MHz
LEFT_OUT = (11, 47)                             # the two groups of weight 0
DPHI = 0.05


def weights(nchg=NCHG):
    w = np.ones(nchg)
    for g in LEFT_OUT:
        if g < nchg:
            w[g] = 0
    return w


def phis(nphi, dphi=DPHI):
    """nphi depths dphi apart, 0 at k = nphi div 2."""
    return dphi * (np.arange(nphi) - nphi // 2)


def table(nchg, nphi):
    """(T, w, use) of rm_table over the first nchg groups with the two groups left out."""
    T, w, use, _ = rm_table(FREQS[:nchg], phis(nphi), weights(nchg))
    return T, w, use


def float_scene(seed, npair, nchg, nbin):
    """chi-squared powers in XX and YY, normal cross words, a different level per channel: f32 [npair][4][nchg][nbin]."""
    rng = np.random.default_rng(seed)
    X = np.empty((npair, 4, nchg, nbin))
    level = 1.0 + rng.random((npair, 1, nchg, 1))
    X[:, :2] = rng.chisquare(4, (npair, 2, nchg, nbin)) * level
    X[:, 2:] = rng.standard_normal((npair, 2, nchg, nbin)) * level
    return X.astype(F)


def integer_scene(seed, npair, nchg, nbin, top=4):
    """integers 0..top-1 in XX and YY, -(top/2)..top/2 in the cross words."""
    rng = np.random.default_rng(seed)
    X = np.empty((npair, 4, nchg, nbin))
    X[:, :2] = rng.integers(0, top, (npair, 2, nchg, nbin))
    X[:, 2:] = rng.integers(-(top // 2), top // 2 + 1, (npair, 2, nchg, nbin))
    return X.astype(F)


def poison_left_out(X, use):
    """NaN and Inf in the channels that are left out: nothing of them may arrive."""
    idle = np.flatnonzero(np.asarray(use) == 0)
    for n, g in enumerate(idle):
        X[:, :, g, :] = np.nan if n % 2 == 0 else np.inf
    return X


def masks(kind, npair, nbin):
    """(off, on) uint8 [npair][nbin].  full: every bin in both; partial: on = the middle third (shifted by a bin per pair), off =
    the rest; empty_off / empty_on: pair 0 has no off-pulse / no on-pulse bin, the others are partial."""
    off, on = np.ones((npair, nbin), np.uint8), np.ones((npair, nbin), np.uint8)
    if kind == 'full':
        return off, on
    for p in range(npair):
        a, b = nbin // 3 + p, max(nbin // 3 + p + 1, 2 * nbin // 3 + p)
        on[p] = 0
        on[p, a:b] = 1
        off[p] = 1 - on[p]
    if kind == 'empty_off':
        off[0] = 0
    elif kind == 'empty_on':
        on[0] = 0
    else:
        assert kind == 'partial'
    return off, on


def planted(seed=5, nbin=40, rm=1.37, amp=10.0, noise=0.3):
    """The planted scene: a Gaussian pulse of sigma 2 bins at bin 20, 60 % linear with PA 0.3 + 0.05 (b - 20) rad, Faraday-rotated by
    `rm` rad/m^2 over the 70 groups, Q and U offsets of +0.8 and -0.2, normal noise of `noise` per Stokes word.  Linear feeds:
    f64 [1][4][nchg][nbin], the off-pulse mask (bins outside 12..28) and the on-pulse mask."""
    rng = np.random.default_rng(seed)
    b = np.arange(nbin)
    lam2 = rm_lambda2(FREQS)[:, None]
    I = amp * np.exp(-0.5 * ((b - 20) / 2.0) ** 2)[None, :] * np.ones((NCHG, 1))
    chi = 0.3 + 0.05 * (b - 20)[None, :] + rm * lam2
    Q, U, V = 0.6 * I * np.cos(2 * chi) + 0.8, 0.6 * I * np.sin(2 * chi) - 0.2, 0.1 * I
    I, Q, U, V = (s + noise * rng.standard_normal(s.shape) for s in (I + 1.0, Q, U, V))
    X = np.stack([(I + Q) / 2, (I - Q) / 2, U / 2, V / 2])[None]
    on = ((b >= 12) & (b <= 28)).astype(np.uint8)[None]
    return X, 1 - on, on
