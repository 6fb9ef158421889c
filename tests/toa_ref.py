"""Restatement of the template-matched arrival phases, written from the contract in include/xeng.h ("Template-matched arrival
phases of folded profiles"), not from the kernels, in numpy float32, operation by operation:

  * the intensity: the first plane, or one float32 add of the first two at nprod = 4;
  * a sub-band's profile: a chain of fmaf32 (tests/fold_ref.py: one rounding) from +0 over its used groups (w != 0) in ascending g;
    the band row a chain of adds over the sub-bands in ascending r;
  * base: 64 partial chains over the off-pulse bins b mod 64 = j in ascending b, summed in ascending j, divided by (float)n_off in
    float32 (numpy's division is correctly rounded), +0 at n_off = 0; var the same over fl(d d), d = fl(P - base);
  * the harmonics: two chains of fmaf32 over all bins in ascending b;
  * the cross-spectrum: cr = fmaf(re, sr, fl(im si)), ci = fmaf(im, sr, -fl(re si));
  * the correlation: a chain over the harmonics in ascending k, two fmaf32 each;
  * the record: the largest word, the smallest l among equals, a NaN never; -1 with nothing comparable or no used group.

Arrays are vectorised over what the contract leaves independent (pairs' rows, bins, harmonics, lags); every chain runs in the order
stated."""
import numpy as np

from tests.fold_ref import fmaf32

F = np.float32
RECORD = np.dtype([('l', '<i4'), ('peak', '<f4'), ('base', '<f4'), ('var', '<f4')])
RUN = 64


def mean32(s, off):
    """s [..][nbin] float32, off [nbin]: the contract's mean over the off-pulse bins."""
    part = np.zeros(s.shape[:-1] + (RUN,), F)
    t = np.zeros(s.shape[:-1], F)
    n = int(np.count_nonzero(off))
    if n == 0:
        return t
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(s.shape[-1]):
            if off[b]:
                part[..., b % RUN] = part[..., b % RUN] + s[..., b]
        for j in range(RUN):
            t = t + part[..., j]
        return (t / F(n)).astype(F)


def offsets(npair, nsub, nbin, nharm, nlag):
    """(byte offset of P, of PH, of ccf, bytes of the output)"""
    nrow = npair * (nsub + 1)
    a = 16 * nrow
    b = a + 4 * nrow * nbin
    c = b + 8 * nrow * nharm
    return a, b, c, c + 4 * nrow * nlag


def split_out(out, npair, nsub, nbin, nharm, nlag):
    a, b, c, n = offsets(npair, nsub, nbin, nharm, nlag)
    out = np.ascontiguousarray(out).reshape(-1).view(np.uint8)
    assert out.size == n
    return (out[:a].view(RECORD).reshape(npair, nsub + 1), out[a:b].view(F).reshape(npair, nsub + 1, nbin), out[b:c].view(F).reshape(npair, nsub + 1, nharm, 2),
            out[c:].view(F).reshape(npair, nsub + 1, nlag))


def toa(X, edges, w, D, L, S, off=None, active=None):
    """(records [npair][nsub+1] RECORD, P f32 [npair][nsub+1][nbin], PH f32 [npair][nsub+1][nharm][2], ccf f32 [npair][nsub+1][nlag])"""
    X, D, L, S = np.asarray(X, F), np.asarray(D, F), np.asarray(L, F), np.asarray(S, F)
    npair, nprod, nchg, nbin = X.shape
    nsub, nharm, nlag = len(edges) - 1, D.shape[1], L.shape[1]
    assert nprod in (1, 4) and D.shape == (nbin, nharm, 2) and L.shape == (nharm, nlag, 2) and S.shape == (npair, nsub + 1, nharm, 2)
    w = np.ones(nchg, F) if w is None else np.asarray(w, F)
    off = np.ones((npair, nbin), np.uint8) if off is None else np.asarray(off)
    active = np.ones(npair, np.uint8) if active is None else np.asarray(active)
    rec = np.zeros((npair, nsub + 1), RECORD)
    rec['l'] = -1
    P, PH, ccf = np.zeros((npair, nsub + 1, nbin), F), np.zeros((npair, nsub + 1, nharm, 2), F), np.zeros((npair, nsub + 1, nlag), F)
    used = [[g for g in range(edges[r], edges[r + 1]) if w[g] != 0] for r in range(nsub)]
    for p in range(npair):
        if not active[p]:
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            band = np.zeros(nbin, F)
            for r in range(nsub):
                acc = np.zeros(nbin, F)
                for g in used[r]:                       # (a group that is not used is not read at all)
                    x = X[p, 0, g] + X[p, 1, g] if nprod == 4 else X[p, 0, g]
                    acc = fmaf32(w[g], x, acc)
                P[p, r] = acc
                band = band + acc
            P[p, nsub] = band
            base = mean32(P[p], off[p])
            d = (P[p] - base[:, None]).astype(F)
            var = mean32((d * d).astype(F), off[p])
            re, im = np.zeros((nsub + 1, nharm), F), np.zeros((nsub + 1, nharm), F)
            for b in range(nbin):
                re = fmaf32(d[:, b, None], D[None, b, :, 0], re)
                im = fmaf32(d[:, b, None], D[None, b, :, 1], im)
            PH[p, :, :, 0], PH[p, :, :, 1] = re, im
            sr, si = S[p, :, :, 0], S[p, :, :, 1]
            cr = fmaf32(re, sr, (im * si).astype(F))
            ci = fmaf32(im, sr, -(re * si).astype(F))
            acc = np.zeros((nsub + 1, nlag), F)
            for k in range(nharm):
                acc = fmaf32(cr[:, k, None], L[None, k, :, 0], acc)
                acc = fmaf32(ci[:, k, None], L[None, k, :, 1], acc)
            ccf[p] = acc
        for r in range(nsub + 1):
            nu = len(used[r]) if r < nsub else sum(len(u) for u in used)
            ok = ~np.isnan(acc[r])
            l, peak = -1, F(0)
            if nu > 0 and ok.any():
                l = int(np.flatnonzero(ok & (acc[r] == acc[r][ok].max()))[0])
                peak = acc[r][l]                        # (the word at l itself: +0 and -0 are equal)
            rec[p, r] = (l, peak, base[r], var[r])
    return rec, P, PH, ccf


def out_bytes(rec, P, PH, ccf):
    return np.frombuffer(rec.tobytes() + P.tobytes() + PH.tobytes() + ccf.tobytes(), np.uint8)


def canonical(out, nrow):
    """A copy of an output's bytes with every NaN float word as 0x7FC00000 (the records' peak, base and var too, not their l): the
    contract states which words are NaN, not a NaN's sign and payload."""
    out = np.array(out, np.uint8).reshape(-1)
    words = out.view(np.uint32)
    nan = np.isnan(words.view(F))
    nan[:4 * nrow:4] = False
    words[nan] = 0x7FC00000
    return out
