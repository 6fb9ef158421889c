"""Restatement of the Faraday rotation-measure synthesis, written from the contract in include/xeng.h ("Faraday rotation-measure
synthesis of folded profiles"), not from the kernels, in numpy float32, operation by operation:

  * the Stokes words of the feeds, one float32 add or subtract each;
  * the baseline: 64 partial chains over the off-pulse bins b mod 64 = j in ascending b, summed in ascending j, divided by
    (float)n_off in float32 (numpy's division is correctly rounded), +0 at n_off = 0;
  * the Faraday word: four fmaf32 (tests/fold_ref.py: one rounding) per used channel in ascending g, pw = fmaf(im, im, fl(re re));
  * the spectrum: per run of 64 bins a chain over the on-pulse bins in ascending b, then a chain over the runs;
  * the record: the largest word, the smallest k among equals, a NaN never; -1 at n_on = 0 or with nothing comparable;
  * the profile: chains of fmaf32 over the used channels.

Arrays are vectorised over what the contract leaves independent (depths, bins, words); every chain runs in the order stated."""
import numpy as np

from tests.fold_ref import fmaf32

F = np.float32
RECORD = np.dtype([('k', '<i4'), ('peak', '<f4'), ('n_on', '<i4'), ('n_off', '<i4')])
RUN = 64


def stokes32(Xp, feeds):
    """[4][nchg][nbin] float32 -> i, q, u, v, each one float32 operation."""
    x0, x1, x2, x3 = (np.asarray(Xp[s], F) for s in range(4))
    with np.errstate(invalid='ignore', over='ignore'):
        if feeds:
            return x0 + x1, x2 + x2, x3 + x3, x0 - x1
        return x0 + x1, x0 - x1, x2 + x2, x3 + x3


def baseline32(s, off):
    """s [nchg'][nbin] float32, off [nbin]: the baseline per channel."""
    nbin = s.shape[-1]
    part = np.zeros(s.shape[:-1] + (RUN,), F)
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(nbin):
            if off[b]:
                part[..., b % RUN] = part[..., b % RUN] + s[..., b]
        t = np.zeros(s.shape[:-1], F)
        n = int(np.count_nonzero(off))
        if n == 0:
            return t
        for j in range(RUN):
            t = t + part[..., j]
        return (t / F(n)).astype(F)


def offsets(npair, nphi, nbin):
    """(byte offset of spec, of the profile, bytes of the output)"""
    a = 16 * npair
    b = a + 4 * npair * nphi
    return a, b, b + 16 * npair * nbin


def split_out(out, npair, nphi, nbin):
    a, b, n = offsets(npair, nphi, nbin)
    out = np.ascontiguousarray(out).reshape(-1).view(np.uint8)
    assert out.size == n
    return out[:a].view(RECORD), out[a:b].view(F).reshape(npair, nphi), out[b:].view(F).reshape(npair, 4, nbin)


def rmsynth(X, T, w=None, use=None, off=None, on=None, active=None, feeds=0, cube=False):
    """(records [npair] RECORD, spec f32 [npair][nphi], profile f32 [npair][4][nbin]) and, with cube, the Faraday words
    (re, im) f32 [npair][nbin][nphi]."""
    X = np.asarray(X, F)
    T = np.asarray(T, F)
    npair, _, nchg, nbin = X.shape
    nphi = T.shape[1]
    assert X.shape[1] == 4 and T.shape == (nchg, nphi, 2)
    w = np.ones(nchg, F) if w is None else np.asarray(w, F)
    use = np.ones(nchg, np.uint8) if use is None else np.asarray(use)
    off = np.ones((npair, nbin), np.uint8) if off is None else np.asarray(off)
    on = np.ones((npair, nbin), np.uint8) if on is None else np.asarray(on)
    active = np.ones(npair, np.uint8) if active is None else np.asarray(active)
    used = [g for g in range(nchg) if use[g]]
    rec = np.zeros(npair, RECORD)
    spec = np.zeros((npair, nphi), F)
    prof = np.zeros((npair, 4, nbin), F)
    Fre, Fim = np.zeros((npair, nbin, nphi), F), np.zeros((npair, nbin, nphi), F)
    nrun = -(-nbin // RUN)
    for p in range(npair):
        if not active[p]:
            rec[p] = (-1, 0.0, 0, 0)
            continue
        Xu = X[p][:, used, :]                           # (a channel left out is not read at all)
        y = []
        with np.errstate(invalid='ignore', over='ignore'):
            for s in stokes32(Xu, feeds):
                y.append((s - baseline32(s, off[p])[:, None]).astype(F))
        yi, yq, yu, yv = y
        re, im = np.zeros((nbin, nphi), F), np.zeros((nbin, nphi), F)
        si, sv = np.zeros(nbin, F), np.zeros(nbin, F)
        for i, g in enumerate(used):
            tc, ts = T[g, :, 0][None, :], T[g, :, 1][None, :]
            q, u = yq[i][:, None], yu[i][:, None]
            re = fmaf32(q, tc, re)
            re = fmaf32(u, ts, re)
            im = fmaf32(u, tc, im)
            im = fmaf32(-q, ts, im)
            si = fmaf32(w[g], yi[i], si)
            sv = fmaf32(w[g], yv[i], sv)
        with np.errstate(invalid='ignore', over='ignore'):
            pw = fmaf32(im, im, (re * re).astype(F))
            sp = np.zeros(nphi, F)
            for r in range(nrun):
                a = np.zeros(nphi, F)
                for b in range(r * RUN, min(nbin, (r + 1) * RUN)):
                    if on[p, b]:
                        a = a + pw[b]
                sp = sp + a
        n_on, n_off = int(np.count_nonzero(on[p])), int(np.count_nonzero(off[p]))
        ok = ~np.isnan(sp)
        k, peak = -1, F(0)
        if n_on > 0 and ok.any():
            k = int(np.flatnonzero(ok & (sp == sp[ok].max()))[0])
            peak = sp[k]                                # (the word at k itself: +0 and -0 are equal)
        rec[p] = (k, peak if k >= 0 else 0.0, n_on, n_off)
        spec[p] = sp
        prof[p, 0], prof[p, 3] = si, sv
        if k >= 0:
            prof[p, 1], prof[p, 2] = re[:, k], im[:, k]
        Fre[p], Fim[p] = re, im
    return (rec, spec, prof, Fre, Fim) if cube else (rec, spec, prof)


def out_bytes(rec, spec, prof):
    return np.frombuffer(rec.tobytes() + spec.tobytes() + prof.tobytes(), np.uint8)


def canonical(out, npair):
    """A copy of an output's bytes with every NaN of the float words behind the records as 0x7FC00000: the contract states which
    words are NaN, not a NaN's sign and payload (a negated operand and the order of an fma's operands decide those)."""
    out = np.array(out, np.uint8).reshape(-1)
    words = out[16 * npair:].view(np.uint32)
    words[np.isnan(words.view(F))] = 0x7FC00000
    return out
