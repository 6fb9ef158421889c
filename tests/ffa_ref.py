"""A numpy restatement of the fast-folding search's contract (include/xeng.h, "Fast-folding search of the dedispersed beams"), for the
tests: the series and the downsample chain, the octave pyramid, the statistics in float64 (and in float32, in any order), and
-- given {c, m, g} per (series, octave) -- the folds, the boxcars, the scores and the records in float32, bit for bit what the
library computes, because every word is one correctly rounded add of two fixed words or a product of two."""
import numpy as np

RECORD = np.dtype([('snr', '<f4'), ('p', '<i4'), ('i', '<i4'), ('j', '<i4')])
f32 = np.float32


def ffa_rows(n, p):
    """M: the largest power of two with M * p <= n."""
    M = 1
    while 2 * M * p <= n:
        M *= 2
    return M


def series(x, dtype=np.float32):
    """[nwindows][...][nprod] -> z [nwindows][nser]: the word (nprod = 1) or fl(XX + YY) (nprod = 4)."""
    x = np.asarray(x)
    z = x[..., 0].astype(np.float32) if x.shape[-1] == 1 else (x[..., 0].astype(np.float32) + x[..., 1].astype(np.float32))
    return z.reshape(x.shape[0], -1).astype(dtype)


def downsample(z, nds):
    """z [n * nds][nser] float32 -> u_0 [n][nser]: ((z0 + z1) + z2) + ..., one sequential float32 chain."""
    z = np.asarray(z, np.float32)
    n = z.shape[0] // nds
    g = z[:n * nds].reshape(n, nds, -1)
    u = g[:, 0].copy()
    for k in range(1, nds):
        u = (u + g[:, k]).astype(np.float32)
    return u


def pyramid(u0, noct):
    """u_0 [NT][nser] float32 -> [u_0, u_1 ...], u_o[k] = fl(u_{o-1}[2k] + u_{o-1}[2k+1])."""
    out = [np.asarray(u0, np.float32)]
    for _ in range(1, noct):
        u = out[-1]
        out.append((u[0::2] + u[1::2]).astype(np.float32))
    return out


def stats64(u):
    """The statistics of one octave in float64, the contract's formulas without rounding: u [N][nser] -> c, m, v, g [nser]."""
    u = np.asarray(u, np.float64)
    c = u[0]
    d = u - c
    m = d.mean(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        v = (d * d).mean(axis=0) - m * m
        g = 1.0 / np.sqrt(v)
    return c, m, v, g


def stats32_pairwise(u):
    """The same in float32 with a summation order like the library's: 256 strided partial sums (q by fused multiply-add is not
    restated: the products are rounded), a pairwise tree over them."""
    u = np.asarray(u, np.float32)
    N = u.shape[0]
    c = u[0]
    d = (u - c).astype(np.float32)
    a = np.zeros((256,) + d.shape[1:], np.float32)
    q = np.zeros_like(a)
    for k0 in range(0, N, 256):
        blk = d[k0:k0 + 256]
        a[:blk.shape[0]] += blk
        q[:blk.shape[0]] += blk * blk
    while a.shape[0] > 1:
        a = (a[0::2] + a[1::2]).astype(np.float32)
        q = (q[0::2] + q[1::2]).astype(np.float32)
    r = f32(1.0 / N)
    m = (a[0] * r).astype(np.float32)
    v = ((q[0] * r).astype(np.float64) - m.astype(np.float64) ** 2).astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        g = (f32(1.0) / np.sqrt(v).astype(np.float32)).astype(np.float32)
    return c, m, v, g


def stats32_sequential(u):
    """The plain sequential one-pass chain in float32: the upper end of what an order can cost."""
    u = np.asarray(u, np.float32)
    N = u.shape[0]
    c = u[0]
    a = np.zeros(u.shape[1:], np.float32)
    q = np.zeros(u.shape[1:], np.float32)
    for k in range(N):
        d = (u[k] - c).astype(np.float32)
        a = (a + d).astype(np.float32)
        q = (q + (d * d).astype(np.float32)).astype(np.float32)
    r = f32(1.0 / N)
    m = (a * r).astype(np.float32)
    v = ((q * r).astype(np.float64) - m.astype(np.float64) ** 2).astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        g = (f32(1.0) / np.sqrt(v).astype(np.float32)).astype(np.float32)
    return c, m, v, g


def valid(m, v):
    m, v = np.asarray(m), np.asarray(v)
    with np.errstate(invalid='ignore'):
        return np.isfinite(m) & (v > 0) & (v < np.inf)


def fold(x, p):
    """x [..., N] float32 -> the M profiles [..., M, p] of base period p by the contract's stages."""
    N = x.shape[-1]
    M = ffa_rows(N, p)
    X = np.ascontiguousarray(x[..., :M * p], np.float32).reshape(x.shape[:-1] + (M, p))
    L = 2
    while L <= M:
        B = X.reshape(x.shape[:-1] + (M // L, L, p))
        lo, hi = B[..., :L // 2, :], B[..., L // 2:, :]
        i = np.arange(L)
        h = i >> 1
        jj = (np.arange(p)[None, :] + (((i + 1) >> 1) % p)[:, None]) % p
        out = lo[..., h, :] + hi[..., h[:, None], jj]
        X = out.astype(np.float32).reshape(x.shape[:-1] + (M, p))
        L *= 2
    return X


def rho(iw, M):
    return f32(1.0 / np.sqrt(float((1 << iw) * M)))


def best_of(S):
    """S [..., n] float32 -> (value, flat index) of the largest non-NaN word, among equals the first; index -1 if all are NaN."""
    nan = np.isnan(S)
    T = np.where(nan, -np.inf, S)
    e = T.argmax(axis=-1)
    val = np.take_along_axis(T, e[..., None], axis=-1)[..., 0]
    none = nan.all(axis=-1)
    return np.where(none, f32(0), val).astype(np.float32), np.where(none, -1, e)


def octave_records(x, g, pmin, pmax, nwidth, ok=None):
    """x [nser][N] float32 (x_o), g [nser] float32 -> RECORD [nser][nwidth]: per width the largest score over (p, i, j), among
    equals the smallest p, then i, then j.  ok [nser]: the VALID flags; an invalid series reads {+0, -1, -1, -1}."""
    nser, N = x.shape
    rec = np.zeros((nser, nwidth), RECORD)
    rec['p'] = rec['i'] = rec['j'] = -1
    g = np.asarray(g, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for p in range(pmin, pmax + 1):
            M = ffa_rows(N, p)
            B = fold(x, p)
            for iw in range(nwidth):
                S = ((B * g[:, None, None]).astype(np.float32) * rho(iw, M)).astype(np.float32)
                val, e = best_of(S.reshape(nser, -1))
                better = (e >= 0) & ((rec['p'][:, iw] < 0) | (val > rec['snr'][:, iw]))
                for s in np.flatnonzero(better):
                    rec[s, iw] = (val[s], p, e[s] // p, e[s] % p)
                if iw + 1 < nwidth:
                    B = (B + np.roll(B, -(1 << iw), axis=-1)).astype(np.float32)
    if ok is not None:
        bad = ~np.asarray(ok, bool)
        rec[bad] = (0.0, -1, -1, -1)
    return rec


def records(u0, noct, pmin, pmax, nwidth, stats=None):
    """u0 [NT][nser] float32 -> (RECORD [nser][noct][nwidth], stats [nser][noct][4] = {c, m, v, g}).  stats: the library's own
    (xengFfaGetStats), whose {c, m, g} then replace the restatement's; without them the float32 pairwise ones are used."""
    us = pyramid(u0, noct)
    nser = us[0].shape[1]
    out = np.zeros((nser, noct, nwidth), RECORD)
    st = np.zeros((nser, noct, 4), np.float32)
    for o, u in enumerate(us):
        if stats is None:
            c, m, v, g = stats32_pairwise(u)
        else:
            c, m, v, g = (np.asarray(stats, np.float32).reshape(nser, noct, 4)[:, o, k] for k in range(4))
        st[:, o] = np.stack([c, m, v, g], axis=-1)
        with np.errstate(invalid='ignore', over='ignore'):
            x = ((u - c).astype(np.float32) - m).astype(np.float32).T
        out[:, o] = octave_records(np.ascontiguousarray(x), g, pmin, pmax, nwidth, valid(m, v))
    return out, st
