"""The contract of xengCutout* (include/xeng.h, "Dedispersed cut-outs and DM refinement of single pulses") restated in numpy float32,
operation by operation: every `+`, `-`, `*` and `/` below is one float32 operation on float32 operands (numpy rounds each once), the
fused multiply-add is the correctly rounded fmaf32 of tests/fold_ref.py (the one tests/dedisp_ref.py uses), the medians come from a
sort of fl(v + 0) (tests/detrend_ref.py median_even: xengDetrend's knot rule), and the serving rule is the header's, from counts
alone.  Written from the header, not from the kernels."""
import numpy as np

from tests.detrend_ref import median_even
from tests.fold_ref import fmaf32

F = np.float32
RECORD = np.dtype([('id', '<i4'), ('status', '<i4'), ('S', '<f4'), ('S0', '<f4'), ('i', '<i2'), ('iw', '<i2'), ('j', '<i2'), ('pad', '<i2'),
                   ('M', '<f4'), ('A', '<f4')])
REQUEST = np.dtype([('id', '<i4'), ('pair', '<i4'), ('n_c', '<i8'), ('ic', '<i4'), ('dstep', '<i4')])
EMPTY = (-1, 0, 0.0, 0.0, -1, -1, -1, 0, 0.0, 0.0)
assert RECORD.itemsize == 32 and REQUEST.itemsize == 24


def requests(rows):
    """[(id, pair, n_c, ic, dstep)] -> a REQUEST array."""
    return np.array([tuple(r) for r in rows], REQUEST).reshape(-1)


def best_of_row(row, nwidth, k_mad):
    """row f32[nt] -> (C, iw, j, M, A) of the row's best score, or None: the row is not valid or has no score that is not NaN."""
    row = np.asarray(row, F)
    nt = row.size
    if not np.isfinite(row).all():
        return None
    with np.errstate(all='ignore'):
        M = median_even(row)
        A = median_even(np.abs((row + F(0)) - M))
        sc = F(k_mad) * A
        if not (sc > 0 and np.isfinite(sc)):
            return None
        G = F(1.0) / sc
        B = (row - M).astype(F)                 # B_1 = y
        best = None
        for iw in range(nwidth):
            w = 1 << iw
            rho = F(2.0 ** (-0.5 * iw))
            C = ((B * G).astype(F) * rho).astype(F)
            cand = np.flatnonzero(~np.isnan(C) & (np.arange(nt) >= w - 1))
            if cand.size:
                j = int(cand[np.argmax(C[cand])])                   # (argmax: the first of equal maxima = the smallest j)
                if best is None or C[j] > best[0]:                  # (strictly greater: among equals the smaller iw stays)
                    best = (C[j], iw, j, M, A)
            if iw + 1 < nwidth:
                nxt = np.full(nt, np.nan, F)                        # (B_2w[j] is defined for j >= 2w - 1 only)
                nxt[2 * w - 1:] = B[2 * w - 1:] + B[w - 1:nt - w]
                B = nxt
    return best


class CutoutRef(object):
    def __init__(self, npair, nfine, nwin, delays, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, k_mad, weights=None):
        self.s = np.asarray(delays, np.int64)
        self.ndmf = self.s.shape[0]
        assert self.s.shape == (self.ndmf, nfine) and self.s.min() >= 0 and nfine % nband == 0 and nt % 2 == 0
        self.npair, self.nfine, self.nwin, self.nhist, self.nband, self.nt, self.tscr = npair, nfine, nwin, nhist, nband, nt, tscr
        self.ndmc, self.nwidth, self.nreq_max, self.k_mad = ndmc, nwidth, nreq_max, F(k_mad)
        self.ntu = nt * tscr
        self.c = ndmc // 2
        assert self.s.max() + self.ntu <= nhist
        self.smax = self.s.max(axis=1)
        self.rec_bytes = 32 * nreq_max
        self.w_bytes = 4 * nband * nt
        self.p_bytes = 4 * ndmc * nt
        self.out_bytes = nreq_max * (32 + self.w_bytes + self.p_bytes)
        self.set_weights(weights)
        self.reset()

    def set_weights(self, weights):
        self.w = np.ones(self.nfine, F) if weights is None else np.asarray(weights, F).copy()
        assert np.isfinite(self.w).all()

    def reset(self):
        self.n = 0
        self.x = {}                     # window -> fl(XX + YY) [npair][nfine]
        self.pending = []               # (id, pair, n_c, ic, dstep, first, last)

    def trials(self, ic, dstep):
        d = ic + (np.arange(self.ndmc) - self.c) * dstep
        return [int(v) if 0 <= v < self.ndmf else None for v in d]

    def request(self, reqs):
        add = []
        for r in requests(reqs) if not isinstance(reqs, np.ndarray) else reqs:
            rid, pair, n_c, ic, dstep = (int(r[k]) for k in ('id', 'pair', 'n_c', 'ic', 'dstep'))
            assert 0 <= pair < self.npair and 0 <= ic < self.ndmf and n_c >= 0 and dstep >= 1
            first = n_c - self.ntu // 2
            last = first + self.ntu - 1 + max(int(self.smax[d]) for d in self.trials(ic, dstep) if d is not None)
            add.append((rid, pair, n_c, ic, dstep, first, last))
        assert len(self.pending) + len(add) <= 1024
        self.pending += add

    def cut(self, pair, n_c, ic, dstep):
        """(W f32[nband][nt], P f32[ndmc][nt]) of one request from the windows held."""
        first = n_c - self.ntu // 2
        Q = self.nfine // self.nband
        W = np.zeros((self.nband, self.nt), F)
        P = np.zeros((self.ndmc, self.nt), F)
        lo = max(first, 0)
        hi = first + self.ntu - 1 + max(int(self.smax[d]) for d in self.trials(ic, dstep) if d is not None)
        X = np.stack([self.x[n][pair] for n in range(lo, hi + 1)])       # (a window that is not held any more is a KeyError)
        with np.errstate(all='ignore'):
            for i, d in enumerate(self.trials(ic, dstep)):
                if d is None:
                    continue
                B = np.zeros(self.ntu, F)
                for g in range(self.nband):
                    D = np.zeros(self.ntu, F)
                    for q in range(g * Q, (g + 1) * Q):
                        v = np.zeros(self.ntu, F)
                        n = first + np.arange(self.ntu) + int(self.s[d, q])
                        if self.w[q] != 0:                          # (what a left-out channel holds is never looked at)
                            v[n >= 0] = X[n[n >= 0] - lo, q]
                        D = fmaf32(self.w[q], v, D)
                    B = B + D
                    if i == self.c:
                        a = np.zeros(self.nt, F)
                        for u in range(self.tscr):
                            a = a + D[u::self.tscr]
                        W[g] = a
                a = np.zeros(self.nt, F)
                for u in range(self.tscr):
                    a = a + B[u::self.tscr]
                P[i] = a
        assert W.dtype == F and P.dtype == F
        return W, P

    def record(self, rid, P, ic, dstep):
        rec = np.array([EMPTY], RECORD)[0]
        rec['id'], rec['status'] = rid, 1
        best = None
        for i, d in enumerate(self.trials(ic, dstep)):
            b = None if d is None else best_of_row(P[i], self.nwidth, self.k_mad)
            if b is None:
                continue
            if i == self.c:
                rec['S0'] = b[0]
            if best is None or b[0] > best[1][0]:                   # (strictly greater: among equals the smaller i stays)
                best = (i, b)
        if best is not None:
            i, (C, iw, j, M, A) = best
            rec['status'], rec['S'], rec['i'], rec['iw'], rec['j'], rec['M'], rec['A'] = 0, C, i, iw, j, M, A
        return rec

    def run(self, x, fill=0xCD):
        """x [nc][npair][nfine][4] -> (served ids, expired ids, out): out is None on a call that serves nothing, else the uint8
        array of a serving call's output over bytes of `fill`: what is not `fill` afterwards is what the call writes."""
        x = np.asarray(x, F)
        assert 1 <= x.shape[0] <= self.nwin and x.shape[1:] == (self.npair, self.nfine, 4)
        with np.errstate(all='ignore'):
            I = (x[..., 0] + x[..., 1]).astype(F)
        for k in range(x.shape[0]):
            self.x[self.n] = I[k]
            self.n += 1
        for old in [k for k in self.x if k < self.n - self.nhist]:
            del self.x[old]
        served, expired, keep = [], [], []
        for p in self.pending:
            if p[5] < self.n - self.nhist:
                expired.append(p[0])
            elif p[6] < self.n and len(served) < self.nreq_max:
                served.append(p)
            else:
                keep.append(p)
        self.pending = keep
        if not served:
            return [], expired, None
        out = np.full(self.out_bytes, fill, np.uint8)
        recs = np.array([EMPTY] * self.nreq_max, RECORD)
        self.last = []
        for z, (rid, pair, n_c, ic, dstep, _, _) in enumerate(served):
            W, P = self.cut(pair, n_c, ic, dstep)
            recs[z] = self.record(rid, P, ic, dstep)
            a = self.rec_bytes + z * self.w_bytes
            out[a:a + self.w_bytes] = W.reshape(-1).view(np.uint8)
            a = self.rec_bytes + self.nreq_max * self.w_bytes + z * self.p_bytes
            out[a:a + self.p_bytes] = P.reshape(-1).view(np.uint8)
            self.last.append((recs[z].copy(), W, P))
        out[:self.rec_bytes] = recs.view(np.uint8)
        return [p[0] for p in served], expired, out


def split_out(out, nreq_max, nband, nt, ndmc):
    """A serving call's output bytes -> (RECORD [nreq_max], W f32[nreq_max][nband][nt], P f32[nreq_max][ndmc][nt])."""
    out = np.ascontiguousarray(out).reshape(-1).view(np.uint8)
    a, b = 32 * nreq_max, 32 * nreq_max + 4 * nreq_max * nband * nt
    assert out.size == b + 4 * nreq_max * ndmc * nt
    return out[:a].view(RECORD), out[a:b].view(F).reshape(nreq_max, nband, nt), out[b:].view(F).reshape(nreq_max, ndmc, nt)
