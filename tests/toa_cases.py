"""Scenes, tables, templates and masks shared by the tests of xengToa* (tests/test_toa_*.py): seeded, small, and the same on the CPU
and on the GPU."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks import toa_subbands, toa_tables, toa_template

F = np.float32
LEFT_OUT = (11, 47)                             # the two groups of weight 0
EDGES = (0, 9, 40, 70)                          # the first case's uneven sub-bands over 70 groups


def weights(nchg, left_out=LEFT_OUT):
    """0.5 .. 1.5 per group, 0 in the groups left out."""
    w = 0.5 + ((np.arange(nchg) * 7) % 11) / 10.0
    for g in left_out:
        if g < nchg:
            w[g] = 0
    return w.astype(F)


def pulse(nbin, centre, width):
    """A wrapped Gaussian of sigma `width` bins at bin `centre` (fractional), peak 1."""
    d = (np.arange(nbin) - centre + nbin / 2.0) % nbin - nbin / 2.0
    return np.exp(-0.5 * (d / width) ** 2)


def float_scene(seed, npair, nprod, nchg, nbin, amp=3.0):
    """chi-squared powers in XX and YY (normal cross words at nprod = 4), a different level per group, and a pulse of `amp` per
    plane at bin 0.37 nbin + 2 p: f32 [npair][nprod][nchg][nbin]."""
    rng = np.random.default_rng(seed)
    X = np.empty((npair, nprod, nchg, nbin))
    level = 1.0 + rng.random((npair, 1, nchg, 1))
    n = min(nprod, 2)
    X[:, :n] = rng.chisquare(4, (npair, n, nchg, nbin)) * level
    for p in range(npair):
        X[p, :n] += amp * pulse(nbin, 0.37 * nbin + 2 * p, max(1.0, nbin / 25.0))
    if nprod == 4:
        X[:, 2:] = rng.standard_normal((npair, 2, nchg, nbin)) * level
    return X.astype(F)


def integer_scene(seed, npair, nprod, nchg, nbin, top=4):
    """integers 0..top-1 in every word."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, top, (npair, nprod, nchg, nbin)).astype(F)


def poison_unused(X, edges, w):
    """NaN and Inf in the groups that are not used (weight 0, or outside the sub-bands): nothing of them may arrive."""
    idle = [g for g in range(X.shape[2]) if w[g] == 0 or not edges[0] <= g < edges[-1]]
    for n, g in enumerate(idle):
        X[:, :, g, :] = np.nan if n % 2 == 0 else np.inf
    return X


def masks(kind, npair, nbin):
    """off uint8 [npair][nbin].  full: every bin; partial: the bins outside the middle third (shifted by a bin per pair); empty:
    pair 0 has no off-pulse bin, the others are partial."""
    off = np.ones((npair, nbin), np.uint8)
    if kind == 'full':
        return off
    for p in range(npair):
        a, b = nbin // 3 + p, max(nbin // 3 + p + 1, 2 * nbin // 3 + p)
        off[p, a:b] = 0
    if kind == 'empty':
        off[0] = 0
    else:
        assert kind == 'partial'
    return off


def templates(npair, nsub, nbin, nharm, per_subband=False):
    """S of toa_template: Gaussian templates at bin 0.25 nbin (+ r bins in sub-band r with per_subband), one width per pair."""
    if per_subband:
        prof = np.array([[pulse(nbin, 0.25 * nbin + r, max(1.0, nbin / 25.0) * (1 + 0.2 * p)) for r in range(nsub)] for p in range(npair)])
    else:
        prof = np.array([pulse(nbin, 0.25 * nbin, max(1.0, nbin / 25.0) * (1 + 0.2 * p)) for p in range(npair)])
    return toa_template(prof, nharm, nsub)


def case(seed, npair, nprod, nchg, nbin, edges, nharm, nlag, kind='partial', left_out=LEFT_OUT, per_subband=False, scene=float_scene):
    """dict(X, edges, w, D, L, S, off) of one call; edges an int (near-equal sub-bands) or the list itself."""
    edges = toa_subbands(nchg, edges) if isinstance(edges, int) else np.array(edges, np.int32)
    w = weights(nchg, left_out)
    D, L = toa_tables(nbin, nharm, nlag)
    X = poison_unused(scene(seed, npair, nprod, nchg, nbin), edges, w)
    return dict(X=X, edges=edges, w=w, D=D, L=L, S=templates(npair, len(edges) - 1, nbin, nharm, per_subband), off=masks(kind, npair, nbin))


# ---------------------------------------------------------------- the planted pulsar (tests of the block)
def wrapped_gaussian(x, sigma):
    """A Gaussian of sigma turns at phase 0, wrapped onto the turn; x in turns."""
    x = np.asarray(x, np.float64)
    return sum(np.exp(-0.5 * ((x - np.round(x) + m) / sigma) ** 2) for m in (-2, -1, 0, 1, 2))


def planted_template(nbin, width_bins=1.5):
    """The template's bins: phase 0 is the centre of bin 0."""
    return wrapped_gaussian(np.arange(nbin) / nbin, width_bins / nbin)


def planted_windows(seed, nwindow, npair, freqs_hz, nbin, f0, taus, ddm, amp=1.0, noise=0.3, width_bins=1.5):
    """f32 [nwindow][npair][nfine][4] = [XX, YY, Re, Im] of a pulsar whose period is nbin windows (window n has the phase
    (n + 1/2) / nbin): I = XX + YY = 1 + amp s(phase - 1/(2 nbin) - taus[p] - delta_q) with s the template, delayed by taus[p] turns
    and dispersed by the DM error ddm against the highest channel, delta_q = KDM ddm f0 (f_q^-2 - f_ref^-2) turns (f in MHz); normal
    noise of `noise` in every word."""
    from caltech_bifrost_dsp_amd.blocks.dedisp import KDM
    rng = np.random.default_rng(seed)
    f = np.asarray(freqs_hz, np.float64) * 1e-6
    delta = KDM * ddm * f0 * (f ** -2 - f.max() ** -2)
    phase = (np.arange(nwindow) + 0.5) / nbin
    x = noise * rng.standard_normal((nwindow, npair, f.size, 4))
    for p in range(npair):
        I = 1.0 + amp * wrapped_gaussian(phase[:, None] - 0.5 / nbin - taus[p] - delta[None, :], width_bins / nbin)
        x[:, p, :, 0] += I / 2
        x[:, p, :, 1] += I / 2
    return np.ascontiguousarray(x, F)


def fold_cube(x, nbin, nprod):
    """What BeamFold(nfscr=1, normalise=True) makes of windows [nwindow][npair][nfine][4] whose window n falls in bin n mod nbin, to
    float64 accuracy: f32 [npair][nprod][nfine][nbin], the mean per bin (nprod = 1: of XX + YY)."""
    nwindow, npair, nfine, _ = x.shape
    assert nwindow % nbin == 0
    m = x.astype(np.float64).reshape(nwindow // nbin, nbin, npair, nfine, 4).mean(0)         # [nbin][npair][nfine][4]
    m = m.transpose(1, 3, 2, 0)
    return np.ascontiguousarray(m[:, :1] + m[:, 1:2] if nprod == 1 else m, F)


def cramer_rao(S, amp, sigma_bin, nbin):
    """The Cramer-Rao error in turns of the delay of a profile amp s + noise of sigma_bin per bin against the template whose
    harmonics are S [nharm][2]: sigma_F / (amp sqrt(2 sum k^2 |S_k|^2)) / (2 pi), sigma_F^2 = nbin sigma_bin^2 / 2."""
    S = np.asarray(S, np.float64)
    k = np.arange(1, S.shape[0] + 1)
    return float(np.sqrt(nbin * sigma_bin ** 2 / 2) / (amp * np.sqrt(2 * np.sum(k * k * (S ** 2).sum(1)))) / (2 * np.pi))


def line_errors(sigma, x, x_ref):
    """(error of the slope, error of the line at x_ref) of a weighted straight-line fit through points at x with errors sigma."""
    wt = np.asarray(sigma, np.float64) ** -2
    x = np.asarray(x, np.float64)
    x0 = np.sum(wt * x) / wt.sum()
    sxx = np.sum(wt * (x - x0) ** 2)
    return float(np.sqrt(1 / sxx)), float(np.sqrt(1 / wt.sum() + (x_ref - x0) ** 2 / sxx))
