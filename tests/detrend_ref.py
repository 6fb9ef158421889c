"""The contract of xengDetrend* (include/xeng.h, "Baseline removal of the dedispersed beams") restated in numpy float32, operation by
operation: every `+`, `-`, `*` and `/` below is one float32 operation on float32 operands (numpy rounds each once), the medians
come from a sort of fl(v + 0), and the knots of a window from the header's index rule.  Written from the header, not from the
kernels."""
import numpy as np

F = np.float32


def median_even(v):
    """v [..., n], n even, no NaN: fl(0.5f fl(lo + hi)) of the values fl(v + 0) of ranks n/2 - 1 and n/2 along the last axis.  (A
    sort of floats without NaN and without -0 is the order of the header's key.)"""
    s = np.sort(np.asarray(v, F) + F(0), axis=-1)
    n = s.shape[-1]
    assert n % 2 == 0
    with np.errstate(all='ignore'):
        return (F(0.5) * (s[..., n // 2 - 1] + s[..., n // 2])).astype(F)


def series(x, nprod):
    """z [nc][nser] of x [nc][..][nprod]: the first word at nprod 1, fl(XX + YY) at nprod 4."""
    x = np.asarray(x, F)
    x = x.reshape(x.shape[0], -1, nprod)
    with np.errstate(all='ignore'):
        return x[..., 0].copy() if nprod == 1 else (x[..., 0] + x[..., 1]).astype(F)


def knot(blk, normalise, k_mad):
    """blk [nser][nblk] -> (M, A, G float32, valid bool), each [nser]."""
    blk = np.asarray(blk, F)
    finite = np.isfinite(blk).all(axis=-1)
    safe = np.where(finite[:, None], blk, F(0)).astype(F)
    with np.errstate(all='ignore'):
        M = median_even(safe)
        A = median_even(np.abs(safe - M[:, None]))
        M = np.where(finite, M, F(0)).astype(F)
        A = np.where(finite, A, F(0)).astype(F)
        valid = finite.copy()
        G = np.zeros_like(M)
        if normalise:
            s = (F(k_mad) * A).astype(F)
            valid &= (s > 0) & np.isfinite(s)
            G = np.where(valid, F(1.0) / np.where(valid, s, F(1)), F(0)).astype(F)
    return M, A, G, valid


class DetrendRef(object):
    def __init__(self, nser, nblk, normalise, k_mad, nprod=1):
        assert nblk % 2 == 0 and 4 <= nblk <= 8192
        self.nser, self.nblk, self.normalise, self.k_mad, self.nprod = nser, nblk, bool(normalise), F(k_mad), nprod
        self.h = nblk // 2
        self.D = 3 * self.h
        self.r = F(1.0) / F(2 * nblk)
        self.reset()

    def reset(self):
        self.n = 0
        self.nblocks = 0
        self.z = {}                     # window -> z [nser]
        self.knots = {}                 # block -> (M, A, G, valid)
        self.newest = None              # (M, A, valid u8) of the newest decided block, as xengDetrendGetKnots gives them

    def _take(self, z):
        self.z[self.n] = z
        self.z.pop(self.n - self.D - self.nblk - 1, None)
        self.n += 1
        if self.n % self.nblk == 0:
            k = self.n // self.nblk - 1
            blk = np.stack([self.z[w] for w in range(k * self.nblk, (k + 1) * self.nblk)], axis=-1)
            M, A, G, valid = knot(blk, self.normalise, self.k_mad)
            self.knots[k] = (M, A, G, valid)
            self.knots.pop(k - 4, None)
            self.nblocks += 1
            self.newest = (M, A, valid.astype(np.uint8))

    def window(self, m):
        """The detrended window m [nser]."""
        out = np.zeros(self.nser, F)
        if m < 0:
            return out
        if m < self.h:
            k, t = -1, m + self.h
        else:
            k = (m - self.h) // self.nblk
            t = m - (k * self.nblk + self.h)
        Ma_, _, Ga_, va = self.knots[max(k, 0)]
        Mb_, _, Gb_, vb = self.knots[k + 1]
        with np.errstate(all='ignore'):
            u = F(F(2 * t + 1) * self.r)
            Ma, Mb = np.where(va, Ma_, Mb_), np.where(vb, Mb_, Ma_)
            base = Ma + u * (Mb - Ma)
            y = self.z[m] - base
            if self.normalise:
                Ga, Gb = np.where(va, Ga_, Gb_), np.where(vb, Gb_, Ga_)
                g = Ga + u * (Gb - Ga)
                y = y * g
            assert y.dtype == F
            out = np.where((va | vb) & np.isfinite(y), y, F(0)).astype(F)
        return out

    def run(self, x):
        """x [nc][nser or npair, ndm][nprod] -> out [nc][nser]"""
        z = series(x, self.nprod)
        n0 = self.n
        for i in range(z.shape[0]):
            self._take(z[i])
        return np.stack([self.window(n0 + i - self.D) for i in range(z.shape[0])])


def detrend(x, sizes, nblk, normalise, k_mad, nprod=1):
    """The outputs of a run of calls of `sizes` windows from a reset, [sum sizes][nser], and the knots per decided block."""
    x = np.asarray(x, F)
    assert x.ndim >= 3 and x.shape[-1] == nprod
    ref = DetrendRef(int(np.prod(x.shape[1:-1])), nblk, normalise, k_mad, nprod)
    outs, knots, a = [], [], 0
    for nc in sizes:
        before = ref.nblocks
        outs.append(ref.run(x[a:a + nc]))
        a += nc
        if ref.nblocks > before:
            knots.append(ref.newest)
    return np.concatenate(outs), knots
