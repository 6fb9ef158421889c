"""Host helpers of BeamRfiClean (xengRfi*, include/xeng.h "Cleaning of the fine-channel power beams"): the thresholds as the library
takes them, what the stats and flags say, and the numpy statements of the library's median and summation rules."""
import math

import numpy as np

MAD_TO_SIGMA = 1.4826           # sigma of a normal distribution over its median absolute deviation
FLAG_MASK, FLAG_DEAD, FLAG_OUTLIER = 1, 2, 4
CODE_OK, CODE_FEW, CODE_BROAD, CODE_BEFORE = 0, 1, 2, 4
RFI_CHAINS = 256


def rfi_controls(nsig_chan=5.0, nsig_clip=6.0, nsig_broad=5.0, min_fraction=0.5, nfine=None):
    """(k_chan, t_clip, t_broad, min_count) for xengRfiSetControl from thresholds in sigma: a channel is an outlier beyond nsig_chan
    sigma of R's scatter over the band (the MAD times 1.4826), a sample is clipped beyond nsig_clip sigma of z = y_0 + y_1 (two
    unit-variance words: sqrt 2), a window is dropped when its sum over count channels is beyond nsig_broad sigma (sqrt(2 count)),
    or when fewer than min_fraction of the nfine channels are left."""
    if nfine is None or int(nfine) != nfine or nfine < 1:
        raise ValueError("rfi_controls: nfine %r is not a positive integer" % (nfine,))
    for name, v in (('nsig_chan', nsig_chan), ('nsig_clip', nsig_clip), ('nsig_broad', nsig_broad)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
            raise ValueError("rfi_controls: %s %r is not a finite positive number" % (name, v))
    if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float)) or not 0 <= min_fraction <= 1:
        raise ValueError("rfi_controls: min_fraction %r is not in 0..1" % (min_fraction,))
    s2 = math.sqrt(2.0)
    return (float(np.float32(MAD_TO_SIGMA * nsig_chan)), float(np.float32(s2 * nsig_clip)), float(np.float32(s2 * nsig_broad)),
            int(math.ceil(min_fraction * nfine)))


def rfi_occupancy(stats):
    """The fraction of samples excised per pair, float64 [npair], from stats i32 [...][npair][4] = {count, clipped, code, not
    kept}: a window with a code loses every channel, another one all but `count`; windows from before the first block (code 4) do
    not count.  NaN for a pair without a counted window."""
    st = np.asarray(stats).reshape(-1, np.shape(stats)[-2], 4).astype(np.int64)
    nfine = st[..., 0] + st[..., 1] + st[..., 3]
    counted = st[..., 2] != CODE_BEFORE
    lost = np.where(st[..., 2] == CODE_OK, nfine - st[..., 0], nfine)
    total = (nfine * counted).sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return (lost * counted).sum(axis=0) / total.astype(np.float64)


def rfi_weights(flags):
    """A BeamDedisperse weight list, float32 [nfine], from a block's flags u8 [npair][nfine] (or [nfine]): 1 where every pair keeps
    the channel, 0 elsewhere -- for users who want to mask but not clean."""
    f = np.asarray(flags)
    if f.ndim == 1:
        f = f[None]
    if f.ndim != 2:
        raise ValueError("rfi_weights: flags of shape %r are not [npair][nfine]" % (f.shape,))
    return (f == 0).all(axis=0).astype(np.float32)


def rfi_sort_key(v):
    """The library's sortable key of float32 values: monotonic over the finite floats, -0 taken as +0."""
    u = (np.asarray(v, np.float32) + np.float32(0)).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(1 << 31))


def rfi_median(v, live=None):
    """The library's median of the float32 values v where `live`: ranked by key, ties by index; the middle value of an odd count,
    0.5f (lo + hi) of the two middle ones of an even count (one float32 addition, one exact halving), +0 of none."""
    v = np.asarray(v, np.float32).reshape(-1)
    idx = np.arange(v.size) if live is None else np.flatnonzero(np.asarray(live).reshape(-1))
    if idx.size == 0:
        return np.float32(0)
    order = idx[np.argsort(rfi_sort_key(v[idx]), kind='stable')]
    lo, hi = v[order[(idx.size - 1) // 2]], v[order[idx.size // 2]]
    with np.errstate(over='ignore', invalid='ignore'):
        return hi if idx.size & 1 else np.float32(np.float32(0.5) * np.float32(lo + hi))


def rfi_mad(v, live=None):
    """(median, median of |v - median|) by rfi_median's rule."""
    v = np.asarray(v, np.float32).reshape(-1)
    med = rfi_median(v, live)
    with np.errstate(over='ignore', invalid='ignore'):
        return med, rfi_median(np.abs(v - med), live)


def rfi_tree_sum(y):
    """The library's sum over channels of y [nfine][...], float32: 256 chains, chain t over the channels t, t + 256, ... in ascending
    order from +0, then P_t = P_t + P_{t + h} for t < h, h = 128, 64, .. 1."""
    y = np.asarray(y, np.float32)
    P = np.zeros((RFI_CHAINS,) + y.shape[1:], np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for q in range(y.shape[0]):
            P[q % RFI_CHAINS] = P[q % RFI_CHAINS] + y[q]
        h = RFI_CHAINS // 2
        while h:
            P[:h] = P[:h] + P[h:2 * h]
            h //= 2
    return P[0]
