"""The numpy restatement of xengCandfold* (include/xeng.h "Folding of search candidates"): what the device must equal byte for byte.
The fold is np.add.at on a float32 cube in window order -- unbuffered and sequential, so it is the chain itself; the refinement is
float32 operation by operation (numpy rounds every array operation to float32 and fuses nothing).  CandfoldRef keeps the
context's state and answers like the C entry points, for the tests of call splits, Reset and SetCandidates and for the block's
backend on CPU rings."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks.cand_fold import CANDFOLD_RECORD, candfold_shifts

MASK64 = (1 << 64) - 1
EMPTY = (0.0, 0.0, -1, -1, -1, 0)


def series(x, nprod):
    """z float32 [nwin][nser] of a span [nwin][npair][ndm][nprod]: the word, or fl(XX + YY)."""
    x = np.asarray(x, np.float32).reshape(x.shape[0], -1, nprod)
    return x[..., 0].copy() if nprod == 1 else x[..., 0] + x[..., 1]


def bins(phi0, dphi, ddphi, m, nbin):
    """fold_bin for an array of m (0 <= m < 2^31): Phi = phi0 + dphi m + ddphi m (m - 1) / 2 in wrapping 64-bit arithmetic,
    bin = ((Phi >> 32) * nbin) >> 32."""
    m = np.asarray(m, np.uint64)
    tri = (m * (m - np.minimum(m, np.uint64(1)))) >> np.uint64(1)
    with np.errstate(over='ignore'):
        phi = np.uint64(int(phi0) & MASK64) + np.uint64(int(dphi) & MASK64) * m + np.uint64(int(ddphi) & MASK64) * tri
    return (((phi >> np.uint64(32)) * np.uint64(nbin)) >> np.uint64(32)).astype(np.int64)


def profiles(cube, hits, rot):
    """p_t float32 [ntrial][nbin] of one candidate: cube float32 and hits uint32 [nsub][nbin], rot int [ntrial][nsub] (mod nbin)."""
    ntrial, nsub = rot.shape
    nbin = cube.shape[1]
    j = np.arange(nbin)
    P, H = np.zeros((ntrial, nbin), np.float32), np.zeros((ntrial, nbin), np.uint32)
    for s in range(nsub):
        idx = (j[None, :] - rot[:, s:s + 1]) % nbin
        P = P + cube[s][idx]
        H = H + hits[s][idx]
    with np.errstate(all='ignore'):
        return np.where(H > 0, P / H.astype(np.float32), np.float32(0.0)).astype(np.float32)


def best(C):
    """(value, flat index) of the largest entry of C that is not NaN, the first among equals in C's own order; (None, -1) without one."""
    C = C.reshape(-1)
    ok = ~np.isnan(C)
    if not ok.any():
        return None, -1
    top = C[ok].max()
    k = int(np.flatnonzero(ok & (C == top))[0])
    return C[k], k


def scores(p, total, gains, nwidth):
    """C float32 [ntrial][nwidth][nbin] from the profiles p [ntrial][nbin]."""
    nbin = p.shape[1]
    C = np.empty((p.shape[0], nwidth, nbin), np.float32)
    B = p
    with np.errstate(all='ignore'):
        for iw in range(nwidth):
            w = 1 << iw
            base = np.float32(total) * np.float32(w / nbin)
            C[:, iw, :] = (B - base) * np.float32(gains[iw])
            B = B + np.roll(B, -w, axis=1)
    return C


def refine(cube, hits, rot, gains, nwidth, izero):
    """(record tuple, best profile float32 [nbin]) of one active candidate."""
    nsub, nbin = cube.shape
    pz = profiles(cube, hits, np.zeros((1, nsub), np.int64))[0]
    total = pz[0]
    with np.errstate(all='ignore'):
        for b in range(1, nbin):
            total = np.float32(total + pz[b])
    p = profiles(cube, hits, rot)
    C = scores(p, total, gains, nwidth)
    S, k = best(C)
    S0 = np.float32(0.0)
    if izero >= 0:
        v, _ = best(C[izero])
        if v is not None:
            S0 = v
    if k < 0:
        return (0.0, S0, -1, -1, -1, 0), np.zeros(nbin, np.float32)
    it, rest = divmod(k, nwidth * nbin)
    return (S, S0, it, rest // nbin, rest % nbin, 0), p[it].copy()


class CandfoldRef:
    """The context of xengCandfold* in numpy: set_candidates / run / reset as the C entry points behave, `cube` and `hits` of the
    last completed segment as xengCandfoldGetCube returns them."""

    def __init__(self, npair, ndm, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains):
        self.nser, self.nprod, self.ncand_max, self.nbin, self.nsub, self.nsubwin, self.nwidth = npair * ndm, nprod, ncand_max, nbin, nsub, nsubwin, nwidth
        self.nt = nsub * nsubwin
        self.rot = candfold_shifts(d1, d2, nsub, nbin)
        zero = np.flatnonzero((np.asarray(d1) == 0) & (np.asarray(d2) == 0))
        self.izero = int(zero[0]) if zero.size else -1
        self.gains = np.asarray(gains, np.float32)
        self.cands, self.waiting, self.n_ref = None, None, 0
        self.cube, self.hits = None, None
        self.reset()

    def _clear(self):
        self._cube = np.zeros((self.ncand_max, self.nsub * self.nbin), np.float32)
        self._hits = np.zeros((self.ncand_max, self.nsub * self.nbin), np.uint32)

    def reset(self):
        self._clear()
        self.nwindows, self.nsegs = 0, 0
        if self.waiting is not None:
            self.cands, self.waiting = self.waiting, None
        self.n_ref = 0

    def set_candidates(self, series_, phi0, dphi, ddphi, active):
        cands = [(int(s), int(a), int(b), int(c), bool(on)) for s, a, b, c, on in zip(series_, phi0, dphi, ddphi, active)]
        assert 1 <= len(cands) <= self.ncand_max and all(0 <= c[0] < self.nser for c in cands)
        if self.nwindows % self.nt == 0:
            self.cands, self.waiting, self.n_ref = cands, None, self.nwindows
        else:
            self.waiting = cands

    def _fold(self, z, pos, m0):
        n = np.arange(z.shape[0])
        s = (pos + n) // self.nsubwin
        for c, (ser, phi0, dphi, ddphi, on) in enumerate(self.cands):
            if on:
                np.add.at(self._cube[c], s * self.nbin + bins(phi0, dphi, ddphi, m0 + n, self.nbin), z[:, ser])
                np.add.at(self._hits[c], s * self.nbin + bins(phi0, dphi, ddphi, m0 + n, self.nbin), np.uint32(1))

    def _refine(self):
        rec, prof = np.zeros(self.ncand_max, CANDFOLD_RECORD), np.zeros((self.ncand_max, self.nbin), np.float32)
        rec[:] = EMPTY
        for c, cand in enumerate(self.cands):
            if cand[4]:
                r, prof[c] = refine(self._cube[c].reshape(self.nsub, self.nbin), self._hits[c].reshape(self.nsub, self.nbin), self.rot, self.gains,
                                    self.nwidth, self.izero)
                rec[c] = r
        return rec, prof

    def run(self, x):
        """x [nc][npair][ndm][nprod]; None, or (records, profiles) when the call completes a segment."""
        assert self.cands is not None
        z = series(x, self.nprod)
        nc, pos = z.shape[0], self.nwindows % self.nt
        head = min(nc, self.nt - pos)
        self._fold(z[:head], pos, self.nwindows - self.n_ref)
        out = None
        if pos + head == self.nt:
            out = self._refine()
            self.cube = self._cube.reshape(self.ncand_max, self.nsub, self.nbin)
            self.hits = self._hits.reshape(self.ncand_max, self.nsub, self.nbin)
            self._clear()
            if self.waiting is not None:
                self.cands, self.waiting, self.n_ref = self.waiting, None, self.nwindows + head
            if nc > head:
                self._fold(z[head:], 0, self.nwindows + head - self.n_ref)
            self.nsegs += 1
        self.nwindows += nc
        return out

    @staticmethod
    def span(out):
        """The bytes of an output span: records, then profiles."""
        return out[0].tobytes() + out[1].tobytes()
