"""The contract of xengRfi* (include/xeng.h, "Cleaning of the fine-channel power beams") restated in numpy float32, operation by
operation: every `+`, `-`, `*`, `/` and sqrt below is one float32 operation on float32 operands (numpy rounds each once), the chains
run in window order, the tree is as written, and the medians come from a stable sort of the sortable keys (ties by index).  Written
from the header, not from the kernels."""
import numpy as np

F = np.float32
CHAINS = 256


def sort_key(v):
    """The sortable key of fl(v + 0): monotonic over the finite floats, -0 as +0."""
    u = (np.asarray(v, F) + F(0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def median_ties_by_index(v, live):
    """The median of v over the entries where live: rank by key, ties by index; the value of rank n/2 for odd n, 0.5 (lo + hi) of
    ranks (n-1)/2 and n/2 for even n, +0 for n = 0."""
    idx = np.flatnonzero(live)
    n = idx.size
    if n == 0:
        return F(0)
    order = idx[np.argsort(sort_key(v[idx]), kind='stable')]
    lo, hi = F(v[order[(n - 1) // 2]]), F(v[order[n // 2]])
    with np.errstate(all='ignore'):
        return hi if n & 1 else F(F(0.5) * F(lo + hi))


def tree_sum(y):
    """y [nfine][nw]: chain t takes the rows q = t (mod 256) ascending from +0, then P_t = P_t + P_{t+h}, h = 128 .. 1."""
    y = np.asarray(y, F)
    P = np.zeros((CHAINS,) + y.shape[1:], F)
    with np.errstate(all='ignore'):
        for q0 in range(0, y.shape[0], CHAINS):
            seg = y[q0:q0 + CHAINS]
            P[:seg.shape[0]] = P[:seg.shape[0]] + seg
        h = CHAINS // 2
        while h >= 1:
            P[:h] = P[:h] + P[h:2 * h]
            h //= 2
    return P[0]


def decide(c, m, v, mask, k_chan):
    """One pair's block: c, m [nfine][4], v [nfine][2], mask u8 [nfine] -> dict(flags, mu, var, r, gains, med, mad)."""
    k_chan = F(k_chan)
    with np.errstate(all='ignore'):
        mu = (c[:, 0] + m[:, 0]) + (c[:, 1] + m[:, 1])
        V = v[:, 0] + v[:, 1]
        R = V / (mu * mu)
        ok = np.isfinite(m).all(axis=1) & (v[:, 0] > 0) & np.isfinite(v[:, 0]) & (v[:, 1] > 0) & np.isfinite(v[:, 1]) & (mu > 0) & np.isfinite(R)
        flags = ((mask != 0).astype(np.uint8) | np.where(ok, 0, 2).astype(np.uint8)).astype(np.uint8)
        live = flags == 0
        med = median_ties_by_index(R, live)
        dev = np.abs(R - med)
        mad = median_ties_by_index(dev, live)
        out = live & (dev > F(k_chan * mad))
        flags[out] |= 4
        kept = flags == 0
        g = np.zeros((c.shape[0], 4), F)
        g0 = F(1) / np.sqrt(v[kept, 0])
        g1 = F(1) / np.sqrt(v[kept, 1])
        gx = np.sqrt(g0 * g1)
        g[kept] = np.stack([g0, g1, gx, gx], axis=1)
    return dict(flags=flags, mu=mu.astype(F), var=V.astype(F), r=R.astype(F), gains=g, med=med, mad=mad)


def apply_window(x, c, m, tab, t_clip, t_broad, min_count, zerodm):
    """One pair's window x [nfine][4] under a block's tables -> (out [nfine][4], stats i32 [4])."""
    flags, g = tab['flags'], tab['gains']
    kept = flags == 0
    nfine = x.shape[0]
    with np.errstate(all='ignore'):
        y = ((x - c) - m) * g
        z = y[:, 0] + y[:, 1]
        good = np.isfinite(y).all(axis=1) & (np.abs(z) <= F(t_clip))
        K = kept & good
        count = int(K.sum())
        clipped = int((kept & ~good).sum())
        yK = np.where(K[:, None], y, F(0)).astype(F)
        Z = tree_sum(yK)
        zm = Z / F(count) if count else np.zeros(4, F)
        code = 0
        if count < min_count:
            code = 1
        elif np.abs(F(Z[0] + Z[1])) > F(F(t_broad) * np.sqrt(F(count))):
            code = 2
        out = np.zeros((nfine, 4), F)
        if code == 0:
            out[K] = (y[K] - zm) if zerodm else y[K]
    return out, np.array([count, clipped, code, int((~kept).sum())], np.int32)


class RfiRef(object):
    def __init__(self, npair, nfine, nstat):
        self.npair, self.nfine, self.nstat = npair, nfine, nstat
        self.mask = np.zeros(nfine, np.uint8)
        self.ctl = None
        self.r = F(1.0) / F(nstat)
        self.reset()

    def set_control(self, k_chan, t_clip, t_broad, min_count, zerodm):
        self.ctl = (F(k_chan), F(t_clip), F(t_broad), int(min_count), int(bool(zerodm)))

    def set_mask(self, mask):
        self.mask = np.zeros(self.nfine, np.uint8) if mask is None else np.array(mask, np.uint8).reshape(self.nfine)

    def reset(self):
        self.n = 0
        self.nblocks = 0
        self.hist = {}                  # window index -> [npair][nfine][4]
        self.blocks = {}                # block index -> (c, m, per-pair tables, controls)
        self.c = self.a = self.s = None
        self.block = None               # the newest decided block's tables, as xengRfiGetBlock gives them

    def _ingest(self, x):
        pos = self.n % self.nstat
        with np.errstate(all='ignore'):
            if pos == 0:
                self.c = x.copy()
                self.a = np.zeros_like(x)
                self.s = np.zeros(x.shape[:2] + (2,), F)
            d = x - self.c
            self.a = self.a + d
            self.s = self.s + d[..., :2] * d[..., :2]
            if pos == self.nstat - 1:
                m = self.a * self.r
                v = self.s * self.r - m[..., :2] * m[..., :2]
                k = self.n // self.nstat
                tabs = [decide(self.c[p], m[p], v[p], self.mask, self.ctl[0]) for p in range(self.npair)]
                self.blocks[k] = (self.c, m, tabs, self.ctl[1:])
                self.blocks.pop(k - 2, None)
                self.nblocks += 1
                self.block = tuple(np.stack([t[key] for t in tabs]) for key in ('flags', 'mu', 'var', 'r', 'gains'))
                self.block_cmv = (self.c, m, v)
        self.hist[self.n] = x
        self.hist.pop(self.n - 2 * self.nstat - 1, None)
        self.n += 1

    def run(self, x):
        """x [nc][npair][nfine][4] -> (out the same shape, stats i32 [nc][npair][4])"""
        x = np.ascontiguousarray(x, F)
        nc = x.shape[0]
        out = np.zeros_like(x)
        stats = np.zeros((nc, self.npair, 4), np.int32)
        n0 = self.n
        for i in range(nc):
            self._ingest(x[i])
        for i in range(nc):
            ns = n0 + i - self.nstat
            if ns < 0:
                stats[i, :, 2] = 4
                continue
            c, m, tabs, ctl = self.blocks[ns // self.nstat]
            for p in range(self.npair):
                out[i, p], stats[i, p] = apply_window(self.hist[ns][p], c[p], m[p], tabs[p], *ctl)
        return out, stats
