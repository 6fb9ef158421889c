"""Restatement of the boxcar single-pulse search (xengPulse*), written from the contract in include/xeng.h, "Boxcar single-pulse
search of the dedispersed beams": baseline blocks with a pivot, the normalised series, the pairwise boxcar tree, the score and
the record of a call.

pulse_search(z, nstat, nwidth, dtype, sizes) is vectorised over the series.  dtype = np.float64 is the tolerance reference (every
step in float64, rho and g exact to float64).  dtype = np.float32 follows the contract's roundings one by one: every fl() is a
float32 operation and fmaf(a, b, c) is the correctly rounded fused multiply-add of tests/fold_ref.py (fmaf32: the exact product, the
sum rounded to odd in float64, one rounding to float32), so the float32 mode is the contract's value on any data, float data
included, not only on the integer data of the word-for-word tests; g = float32(1) / sqrt(v) in float32, the library's documented
choice.  pulse_search_naive is the same definition one
term at a time, with a mask for "has a y" where the vectorised version has one too (no NaN sentinel in either)."""
import numpy as np

from tests.fold_ref import fmaf32

NONE = (0.0, -1, -1, 0.0)           # the record of a series with nothing scored in the call


def series(x, dtype=np.float64):
    """z of the contract from the input layout [nwindows][...][nprod]: word 0, or word 0 + word 1 in one rounding."""
    x = np.asarray(x)
    if x.shape[-1] == 1:
        return x[..., 0].astype(dtype)
    return (x[..., 0].astype(dtype) + x[..., 1].astype(dtype)).astype(dtype)


def _fma(a, b, c, dtype):
    if dtype == np.float64:
        return a * b + c
    return fmaf32(a, b, c)


def rho(iw, dtype):
    """2^(-iw/2): rounded to float32 as the host hands it to the kernel, or in float64 -- there as 1 or 2^-0.5 times a power of
    two, so that rho[iw + 2] is exactly half of rho[iw] as it is in float32."""
    r = (1.0, 0.5 ** 0.5)[iw % 2] * 0.5 ** (iw // 2)
    return np.float32(r) if dtype == np.float32 else r


def block_chain(zb, dtype):
    """(c, a, q) of the contract after the first zb.shape[1] windows of a block, zb [nblocks][windows][nser]: the pivot and the
    two running sums (the state of a block that is not complete yet)."""
    with np.errstate(all='ignore'):
        c = zb[:, 0].copy()
        a = np.zeros_like(c)
        q = np.zeros_like(c)
        for i in range(zb.shape[1]):
            d = (zb[:, i] - c).astype(dtype)
            a = (a + d).astype(dtype)
            q = _fma(d, d, q, dtype)
    return c, a, q


def baseline_blocks(z, nstat, dtype):
    """(c, m, v, valid, g) of every complete block, [nblocks][nser] each."""
    nb = z.shape[0] // nstat
    zb = z[:nb * nstat].reshape(nb, nstat, z.shape[1])
    r = dtype(np.float32(1.0) / np.float32(nstat)) if dtype == np.float32 else 1.0 / nstat
    with np.errstate(all='ignore'):
        c, a, q = block_chain(zb, dtype)
        m = (a * r).astype(dtype)
        v = _fma(-m, m, (q * r).astype(dtype), dtype)
        valid = (v > 0) & (v < np.inf)
        g = np.where(valid, dtype(1) / np.sqrt(np.where(valid, v, 1).astype(dtype)), 0).astype(dtype)
    return c, m, v, valid, g


def pulse_search(z, nstat, nwidth, dtype=np.float64, sizes=None):
    """z: [nwindows][...] (the trailing axes are the series).  Returns a dict: 'snr', 'B' [nwindows][nwidth][...] (NaN where
    not scored), 'scored' (bool, same shape), 'c', 'm', 'v', 'valid', 'g' [nblocks][...], and, with `sizes` (the windows of the
    consecutive calls), 'records': per call a dict of 'snr', 'n', 'iw', 'B' [...]."""
    z = np.asarray(z).astype(dtype)
    shape = z.shape[1:]
    z = z.reshape(z.shape[0], -1)
    nwindows, nser = z.shape
    c, m, v, valid, g = baseline_blocks(z, nstat, dtype)
    k = np.arange(nwindows) // nstat
    has = np.zeros((nwindows, nser), bool)
    y = np.zeros((nwindows, nser), dtype)
    gn = np.zeros((nwindows, nser), dtype)
    later = k >= 1
    with np.errstate(all='ignore'):
        if later.any():
            kp = k[later] - 1
            has[later] = valid[kp]
            y[later] = np.where(valid[kp], ((z[later] - c[kp]).astype(dtype) - m[kp]).astype(dtype), 0)
            gn[later] = g[kp]
        snr = np.full((nwindows, nwidth, nser), np.nan, dtype)
        Bs = np.full((nwindows, nwidth, nser), np.nan, dtype)
        scored = np.zeros((nwindows, nwidth, nser), bool)
        B, allhas = y, has
        n = np.arange(nwindows)
        for iw in range(nwidth):
            w = 1 << iw
            if iw:
                h = w // 2
                B2 = np.zeros_like(B)
                B2[h:] = (B[h:] + B[:-h]).astype(dtype)         # newer half first
                a2 = np.zeros_like(allhas)
                a2[h:] = allhas[h:] & allhas[:-h]
                B, allhas = B2, a2
            s = ((B * gn).astype(dtype) * rho(iw, dtype)).astype(dtype)
            ok = allhas & (n - w + 1 >= nstat)[:, None] & ~np.isnan(s)
            scored[:, iw] = ok
            snr[:, iw] = np.where(ok, s, np.nan)
            Bs[:, iw] = np.where(ok, B, np.nan)
    out = dict(snr=snr.reshape((nwindows, nwidth) + shape), B=Bs.reshape((nwindows, nwidth) + shape),
               scored=scored.reshape((nwindows, nwidth) + shape), c=c.reshape((-1,) + shape), m=m.reshape((-1,) + shape),
               v=v.reshape((-1,) + shape), valid=valid.reshape((-1,) + shape), g=g.reshape((-1,) + shape))
    if sizes is not None:
        assert sum(sizes) == nwindows
        recs, a = [], 0
        for nc in sizes:
            recs.append({f: r.reshape(shape) for f, r in call_record(snr[a:a + nc], Bs[a:a + nc], scored[a:a + nc]).items()})
            a += nc
        out['records'] = recs
    return out


def call_record(snr, B, scored):
    """The record of one call from its [nc][nwidth][nser] cubes: the largest scored snr, among equals the smallest n, then the
    smallest iw (the first in (n, iw) order)."""
    nc, nwidth, nser = snr.shape
    key = np.where(scored, snr, -np.inf).reshape(nc * nwidth, nser)
    sc = scored.reshape(nc * nwidth, nser)
    idx = key.argmax(axis=0)                                    # (the first of equal maxima)
    top = key[idx, np.arange(nser)]
    first = sc.argmax(axis=0)
    idx = np.where(np.isneginf(top), first, idx)                # (a scored -inf is a score: the first scored entry holds one then)
    any_ = sc.any(axis=0)
    col = np.arange(nser)
    return dict(snr=np.where(any_, snr.reshape(nc * nwidth, nser)[idx, col], 0).astype(snr.dtype),
                n=np.where(any_, idx // nwidth, -1).astype(np.int32), iw=np.where(any_, idx % nwidth, -1).astype(np.int32),
                B=np.where(any_, B.reshape(nc * nwidth, nser)[idx, col], 0).astype(snr.dtype))


def merge_records(records, sizes):
    """What the host does with the calls' records: strictly greater replaces, in call order; n becomes the window of the run."""
    best, a = None, 0
    for rec, nc in zip(records, sizes):
        rec = {f: np.array(r) for f, r in rec.items()}
        rec['n'] = np.where(rec['n'] >= 0, rec['n'] + a, -1)
        if best is None:
            best = rec
        else:
            with np.errstate(invalid='ignore'):
                take = (rec['n'] >= 0) & ((best['n'] < 0) | (rec['snr'] > best['snr']))
            for f in best:
                best[f] = np.where(take, rec[f], best[f])
        a += nc
    return best


def pulse_search_naive(z, nstat, nwidth, sizes):
    """The definition one term at a time in float64, z [nwindows][nser]: (snr, scored) [nwindows][nwidth][nser] and the list of
    per-call records [(snr, n, iw, B)] per series."""
    z = np.asarray(z, np.float64)
    nwindows, nser = z.shape
    snr = np.full((nwindows, nwidth, nser), np.nan)
    scored = np.zeros((nwindows, nwidth, nser), bool)
    Bc = np.full((nwindows, nwidth, nser), np.nan)
    with np.errstate(all='ignore'):
        for s in range(nser):
            blocks = []
            for k in range(nwindows // nstat):
                c, a, q = z[k * nstat, s], 0.0, 0.0
                for n in range(k * nstat, (k + 1) * nstat):
                    d = z[n, s] - c
                    a += d
                    q += d * d
                mk = a / nstat
                vk = q / nstat - mk * mk
                blocks.append((c, mk, vk, 0 < vk < np.inf))
            y = {}
            for n in range(nstat, nwindows):
                c, mk, vk, ok = blocks[n // nstat - 1]
                if ok:
                    y[n] = (z[n, s] - c) - mk

            def box(n, w):
                if w == 1:
                    return y.get(n)
                new, old = box(n, w // 2), box(n - w // 2, w // 2)
                return None if new is None or old is None else new + old

            for n in range(nwindows):
                for iw in range(nwidth):
                    w = 1 << iw
                    if n - w + 1 < nstat:
                        continue
                    B = box(n, w)
                    if B is None:
                        continue
                    val = B / np.sqrt(blocks[n // nstat - 1][2]) * 2.0 ** (-0.5 * iw)
                    if not np.isnan(val):
                        snr[n, iw, s], scored[n, iw, s], Bc[n, iw, s] = val, True, B
    records, a = [], 0
    for nc in sizes:
        per = []
        for s in range(nser):
            best = NONE
            for n in range(a, a + nc):
                for iw in range(nwidth):
                    if scored[n, iw, s] and (best[1] < 0 or snr[n, iw, s] > best[0]):
                        best = (snr[n, iw, s], n - a, iw, Bc[n, iw, s])
            per.append(best)
        records.append(per)
        a += nc
    return snr, scored, records
