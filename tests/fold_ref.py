"""Restatement of the phase folder, written from the contract in include/xeng.h ("Phase-folded profiles of the fine-channel
power beams"), not from the kernels:

  * the oscillator in Python ints mod 2^64:  Phi(m) = phi0 + dphi*m + ddphi*(m(m-1)/2),  bin = ((Phi >> 32) * nbin) >> 32;
  * the accumulation as float32 adds in window order:  prof[p][bin][q][k] = fl(prof[p][bin][q][k] + x[n][p][q][k]);
  * the dump as one chain per output of explicit float32 steps:  sum = fmaf(w[q], x, sum) from +0 over the group's channels in
    ascending q, x = prof[p][(b + rot[p][q]) mod nbin][q][k] (divided by (float)hits in fp32 when normalising, +0 at 0 hits), a
    channel of weight 0 left out, an inactive pair's plane +0.

fmaf32 below is a correctly rounded fp32 fused multiply-add: the product of two fp32 is exact in fp64, the fp64 sum is rounded to
odd (with the error term of a two-sum), and rounding that to fp32 is then the single rounding of the exact result."""
import numpy as np

MASK = (1 << 64) - 1


def osc_phase(phi0, dphi, ddphi, m):
    """Phi(m) in [0, 2^64): Python ints, wrapping."""
    return (int(phi0) + int(dphi) * m + int(ddphi) * (m * (m - 1) // 2)) & MASK


def osc_bin(phi0, dphi, ddphi, m, nbin):
    return ((osc_phase(phi0, dphi, ddphi, m) >> 32) * nbin) >> 32


def fmaf32(a, x, s):
    """fl32(a*x + s) with one rounding, elementwise; a, x, s float32 (arrays or scalars)."""
    a, x, s = (np.asarray(v, np.float32).astype(np.float64) for v in (a, x, s))
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * x                                   # exact: 24 + 24 bits
        t = p + s
        bb = t - p
        err = (p - (t - bb)) + (s - bb)             # two-sum: p + s = t + err exactly
        inexact = np.isfinite(t) & np.isfinite(err) & (err != 0)
        even = (t.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        t = np.where(inexact & even, np.nextafter(t, toward), t)      # round to odd
        return t.astype(np.float32)


def products32(x, nprod):
    """[..., 4] float32 -> [..., nprod] float32: I = fl(XX + YY) or the four words."""
    x = np.asarray(x, np.float32)
    if nprod == 1:
        return (x[..., 0] + x[..., 1])[..., None]
    assert nprod == 4
    return x


class FoldRef:
    """The state of one context and the calls that change it."""

    def __init__(self, npair, nfine, nbin, nprod):
        self.npair, self.nfine, self.nbin, self.nprod = npair, nfine, nbin, nprod
        self.prof = np.zeros((npair, nbin, nfine, nprod), np.float32)
        self.hits = np.zeros((npair, nbin), np.uint32)
        self.n, self.n_ref, self.osc = 0, 0, None
        self.rot, self.w = None, np.ones(nfine, np.float32)

    def set_phase(self, phi0, dphi, ddphi, active, n_ref):
        assert 0 <= n_ref <= self.n
        self.osc = [(int(a), int(b), int(c), bool(d)) for a, b, c, d in zip(phi0, dphi, ddphi, active)]
        assert len(self.osc) == self.npair
        self.n_ref = int(n_ref)

    def set_rotations(self, rot):
        self.rot = np.zeros((self.npair, self.nfine), np.int64) if rot is None else np.asarray(rot, np.int64).reshape(self.npair, self.nfine).copy()
        assert self.rot.min() >= 0 and self.rot.max() < self.nbin

    def set_weights(self, w):
        self.w = np.ones(self.nfine, np.float32) if w is None else np.asarray(w, np.float32).reshape(self.nfine).copy()

    def bins(self, nwin_call):
        """[npair][nwin_call] bins of the next windows (-1 for a pair left out)."""
        out = np.full((self.npair, nwin_call), -1, np.int64)
        for p, (phi0, dphi, ddphi, active) in enumerate(self.osc):
            if active:
                out[p] = [osc_bin(phi0, dphi, ddphi, self.n - self.n_ref + i, self.nbin) for i in range(nwin_call)]
        return out

    def run(self, x):
        """x: [nwin_call][npair][nfine][4]; float32 adds in window order."""
        assert self.osc is not None
        v = products32(x, self.nprod)
        b = self.bins(v.shape[0])
        for i in range(v.shape[0]):
            for p in range(self.npair):
                if b[p, i] >= 0:
                    self.prof[p, b[p, i]] = self.prof[p, b[p, i]] + v[i, p]         # (float32 + float32 -> one rounding)
                    self.hits[p, b[p, i]] += 1
        self.n += v.shape[0]

    def dump(self, nfscr, normalise, clear):
        """(out float32 [npair][nprod][nfine/nfscr][nbin], hits uint32 [npair][nbin])"""
        assert self.rot is not None and self.nfine % nfscr == 0
        ng = self.nfine // nfscr
        out = np.zeros((self.npair, self.nprod, ng, self.nbin), np.float32)
        b = np.arange(self.nbin)
        for p in range(self.npair):
            if self.osc is None or not self.osc[p][3]:
                continue
            for g in range(ng):
                s = np.zeros((self.nprod, self.nbin), np.float32)
                for q in range(g * nfscr, (g + 1) * nfscr):
                    if self.w[q] == 0:
                        continue
                    rows = (b + self.rot[p, q]) % self.nbin
                    x = self.prof[p, rows, q, :].T                          # [nprod][nbin]
                    if normalise:
                        h = self.hits[p, rows]
                        with np.errstate(divide='ignore', invalid='ignore'):
                            x = np.where(h > 0, x / h.astype(np.float32)[None, :], np.float32(0)).astype(np.float32)
                    s = fmaf32(self.w[q], x, s)
                out[p, :, g] = s
        hits = self.hits.copy()
        if clear:
            self.prof[...] = 0
            self.hits[...] = 0
        return out, hits

    def reset(self):
        self.prof[...] = 0
        self.hits[...] = 0
        self.n, self.n_ref = 0, 0


def fold_naive(x, bins, rot, w, nbin, nfscr, nprod, normalise, absolute=False):
    """The same by the definition, one term at a time in float64 (small sizes only): x [nwindows][npair][nfine][4], bins
    [npair][nwindows] (-1: not folded).  absolute: the sum of |w * x| terms instead (the scale of an error bound)."""
    x = np.asarray(x, np.float64)
    nwindows, npair, nfine, _ = x.shape
    prof = np.zeros((npair, nbin, nfine, nprod))
    hits = np.zeros((npair, nbin), np.int64)
    for n in range(nwindows):
        for p in range(npair):
            if bins[p][n] < 0:
                continue
            hits[p, bins[p][n]] += 1
            for q in range(nfine):
                v = [x[n, p, q, 0] + x[n, p, q, 1]] if nprod == 1 else x[n, p, q]
                for k in range(nprod):
                    prof[p, bins[p][n], q, k] += abs(v[k]) if absolute else v[k]
    out = np.zeros((npair, nprod, nfine // nfscr, nbin))
    for p in range(npair):
        for k in range(nprod):
            for q in range(nfine):
                if w[q] == 0:
                    continue
                for b in range(nbin):
                    r = (b + rot[p][q]) % nbin
                    if normalise and hits[p, r] == 0:
                        continue
                    t = prof[p, r, q, k] / (hits[p, r] if normalise else 1)
                    out[p, k, q // nfscr, b] += abs(w[q] * t) if absolute else w[q] * t
    return out, hits
