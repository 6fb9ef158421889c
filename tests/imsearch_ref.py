"""Restatement of the dedispersed transient search of the images (xengImsearch*), written from the contract in include/xeng.h,
"Dedispersed transient search of the images": the series I = XX + YY per (group, pixel), xengPulse's baseline blocks
(tests/pulse_ref.py baseline_blocks, the same definition), the normalised series u, the delayed weighted sum z, the pairwise boxcar
tree, the score and the record of every integration.

imsearch(images, delays, weights, nstat, nwidth, dtype) is vectorised over the pixels.  dtype = np.float64 is the tolerance
reference (every step in float64, kappa, rho and g exact to float64).  dtype = np.float32 follows the contract's roundings one by
one: every fl() is one float32 numpy operation, fmaf as in pulse_ref._fma, g = float32(1) / sqrt(v) in float32, kappa rounded once
from float64.  "No u" and "no z" are masks here, not NaN sentinels.  imsearch_naive is the same definition one term at a time in
float64.

`weights` is one float32 [ngroup] vector or a schedule [(n_from, vector), ...] with ascending n_from, the first 0: the weights set
(xengImsearchSetWeights) when n_from integrations had been taken.  No boxcar of integration n reaches before the n_from in force."""
import numpy as np

from tests.pulse_ref import baseline_blocks, call_record, rho

RECORD = np.dtype([('snr', '<f4'), ('idm', '<i2'), ('iw', '<i2')])


def series(images, dtype):
    """I of the contract from [nint][ngroup][4][npix]: word 0 + word 1 in one rounding."""
    x = np.asarray(images)
    with np.errstate(all='ignore'):
        return (x[:, :, 0].astype(dtype) + x[:, :, 1].astype(dtype)).astype(dtype)


def kappa(weights, dtype):
    k = 1.0 / np.sqrt((np.asarray(weights, np.float64) ** 2).sum())
    return np.float32(k) if dtype == np.float32 else k


def _schedule(weights, nint):
    """per integration (n_from, weights in force)"""
    sched = weights if isinstance(weights, list) else [(0, weights)]
    assert sched[0][0] == 0 and all(a[0] < b[0] for a, b in zip(sched, sched[1:]))
    out = []
    for n in range(nint):
        n_from, w = [e for e in sched if e[0] <= n][-1]
        out.append((n_from, np.asarray(w, np.float32)))
    return out


def normalised(I, nstat, dtype):
    """(u, has_u) [nint][ngroup][npix] and the blocks' (c, m, v, valid) [nblocks][ngroup][npix]"""
    nint = I.shape[0]
    shape = I.shape[1:]
    flat = I.reshape(nint, -1)
    c, m, v, valid, g = baseline_blocks(flat, nstat, dtype)
    u = np.zeros_like(flat)
    has = np.zeros(flat.shape, bool)
    with np.errstate(all='ignore'):
        for n in range(nstat, nint):
            k = n // nstat - 1
            has[n] = valid[k]
            u[n] = np.where(valid[k], (((flat[n] - c[k]).astype(dtype) - m[k]).astype(dtype) * g[k]).astype(dtype), 0)
    return (u.reshape((nint,) + shape), has.reshape((nint,) + shape),
            tuple(a.reshape((-1,) + shape) for a in (c, m, v, valid)))


def imsearch(images, delays, weights, nstat, nwidth, dtype=np.float64):
    """images [nint][ngroup][4][npix], delays int [ndm][ngroup].  Returns a dict: 'score' [nint][ndm][nwidth][npix] (NaN where not
    scored), 'scored' (bool, same shape), 'snr', 'idm', 'iw' [nint][npix] (the records), 'c', 'm', 'v', 'valid'
    [nblocks][ngroup][npix]."""
    delays = np.asarray(delays)
    ndm, ngroup = delays.shape
    I = series(images, dtype)
    nint, _, npix = I.shape
    u, has, (c, m, v, valid) = normalised(I, nstat, dtype)
    back = delays.max() - delays
    sched = _schedule(weights, nint)
    z = np.zeros((nint, ndm, npix), dtype)
    zex = np.zeros((nint, ndm, npix), bool)
    with np.errstate(all='ignore'):
        for n in range(nint):
            w = sched[n][1]
            for d in range(ndm):
                acc = np.zeros(npix, dtype)
                ex = np.ones(npix, bool)
                for g in range(ngroup):
                    if w[g] == 0:
                        continue
                    t = n - back[d, g]
                    if t < nstat:
                        ex[:] = False
                        continue
                    ex &= has[t, g]
                    acc = (acc + (dtype(w[g]) * u[t, g]).astype(dtype)).astype(dtype)
                z[n, d], zex[n, d] = acc, ex
        score = np.full((nint, ndm, nwidth, npix), np.nan, dtype)
        scored = np.zeros((nint, ndm, nwidth, npix), bool)
        B = z
        for iw in range(nwidth):
            wd = 1 << iw
            if iw:
                h = wd // 2
                B2 = np.zeros_like(B)
                B2[h:] = (B[h:] + B[:-h]).astype(dtype)            # newer half first
                B = B2
            for n in range(nint):
                n_from, w = sched[n]
                if n - wd + 1 < max(n_from, 0):
                    continue
                s = ((B[n] * kappa(w, dtype)).astype(dtype) * rho(iw, dtype)).astype(dtype)
                ok = zex[n - wd + 1:n + 1].all(axis=0) & ~np.isnan(s)
                scored[n, :, iw] = ok
                score[n, :, iw] = np.where(ok, s, np.nan)
    snr = np.zeros((nint, npix), dtype)
    idm = np.zeros((nint, npix), np.int16)
    iw_ = np.zeros((nint, npix), np.int16)
    for n in range(nint):
        r = call_record(score[n], score[n], scored[n])          # (first axis: trials; the first of equal maxima in (d, iw) order)
        snr[n], idm[n], iw_[n] = r['snr'], r['n'], r['iw']
    return dict(score=score, scored=scored, snr=snr, idm=idm, iw=iw_, c=c, m=m, v=v, valid=valid, z=z, zex=zex)


def records(res, n):
    """The plane of integration n as the library writes it."""
    out = np.zeros(res['snr'].shape[1], RECORD)
    out['snr'], out['idm'], out['iw'] = res['snr'][n].astype(np.float32), res['idm'][n], res['iw'][n]
    return out


def imsearch_naive(images, delays, weights, nstat, nwidth):
    """The definition one term at a time in float64: (score, scored) [nint][ndm][nwidth][npix] and per integration and pixel the
    record (snr, idm, iw)."""
    x = np.asarray(images, np.float64)
    delays = np.asarray(delays)
    ndm, ngroup = delays.shape
    nint, _, _, npix = x.shape
    S = int(delays.max())
    sched = _schedule(weights, nint)
    score = np.full((nint, ndm, nwidth, npix), np.nan)
    scored = np.zeros((nint, ndm, nwidth, npix), bool)
    recs = [[(0.0, -1, -1)] * npix for _ in range(nint)]
    with np.errstate(all='ignore'):
        for p in range(npix):
            u = {}
            for g in range(ngroup):
                I = x[:, g, 0, p] + x[:, g, 1, p]
                blocks = []
                for k in range(nint // nstat):
                    c, a, q = I[k * nstat], 0.0, 0.0
                    for n in range(k * nstat, (k + 1) * nstat):
                        dl = I[n] - c
                        a += dl
                        q += dl * dl
                    mk = a / nstat
                    vk = q / nstat - mk * mk
                    blocks.append((c, mk, vk, 0 < vk < np.inf))
                for n in range(nstat, nint):
                    c, mk, vk, ok = blocks[n // nstat - 1]
                    if ok:
                        u[n, g] = ((I[n] - c) - mk) * (1.0 / np.sqrt(vk))
            z = {}
            for n in range(nint):
                w = sched[n][1]
                for d in range(ndm):
                    acc, ok = 0.0, True
                    for g in range(ngroup):
                        if w[g] == 0:
                            continue
                        t = n - (S - int(delays[d, g]))
                        if t < nstat or (t, g) not in u:
                            ok = False
                            break
                        acc = acc + float(w[g]) * u[t, g]
                    if ok:
                        z[n, d] = acc

            def box(n, d, wd, n_from):
                if wd == 1:
                    return z.get((n, d)) if n >= n_from else None
                new, old = box(n, d, wd // 2, n_from), box(n - wd // 2, d, wd // 2, n_from)
                return None if new is None or old is None else new + old

            for n in range(nint):
                n_from, w = sched[n]
                kap = 1.0 / np.sqrt(sum(float(a) ** 2 for a in w))
                best = (0.0, -1, -1)
                for d in range(ndm):
                    for iw in range(nwidth):
                        B = box(n, d, 1 << iw, n_from)
                        if B is None:
                            continue
                        val = B * kap * 2.0 ** (-0.5 * iw)
                        if np.isnan(val):
                            continue
                        score[n, d, iw, p], scored[n, d, iw, p] = val, True
                        if best[1] < 0 or val > best[0]:
                            best = (val, d, iw)
                recs[n][p] = best
    return score, scored, recs


def integer_case(npix, ngroup, ndm, nint, seed=0, S=12):
    """(images, delays): integer noise 0..49 in words 0 and 1 of every group, NaN in words 2 and 3 (never read), and ramp_delays."""
    rng = np.random.default_rng(seed)
    x = np.full((nint, ngroup, 4, npix), np.nan, np.float32)
    x[:, :, :2] = rng.integers(0, 50, (nint, ngroup, 2, npix)).astype(np.float32)
    return x, ramp_delays(ndm, ngroup, S)


def ramp_delays(ndm, ngroup, S):
    """Delays growing towards group 0 (the bottom of the band) and with the trial, rounded from a ramp whose largest is exactly S;
    with one trial that trial has the ramp."""
    d = np.arange(ndm)[:, None] if ndm > 1 else np.ones((1, 1))
    g = (ngroup - 1 - np.arange(ngroup))[None, :] if ngroup > 1 else np.ones((1, 1))
    t = d * g
    return np.round(t * (S / t.max())).astype(np.int32)


def plant(x, delays_row, t0, width, pixel, amplitude=150):
    """A box of `width` integrations added to word 0 of `pixel`, in every group delayed by the trial's delay behind t0, the
    integration at which it reaches the top of the band."""
    for g, s in enumerate(delays_row):
        x[t0 + int(s):t0 + int(s) + width, g, 0, pixel] += amplitude
    return x


def planted_case():
    """The planted pulse: npix 70, ngroup 5, ndm 4, delays d * [4, 3, 2, 1, 0], weights [1, 1, 0, 2, 1], nwidth 3, nstat 16, 64
    integrations of integer noise 0..49, +150 in word 0 at pixel 33 for 2 integrations along trial 2, the top of the band at
    integration 33: the pulse and its sweep lie in block 2, whose previous block is clean.  Returns (images, delays, weights,
    expected (n, pixel, idm, iw))."""
    npix, ngroup, ndm, nint = 70, 5, 4, 64
    rng = np.random.default_rng(1)
    x = np.full((nint, ngroup, 4, npix), np.nan, np.float32)
    x[:, :, :2] = rng.integers(0, 50, (nint, ngroup, 2, npix)).astype(np.float32)
    delays = (np.arange(ndm)[:, None] * np.array([4, 3, 2, 1, 0])[None, :]).astype(np.int32)
    plant(x, delays[2], 33, 2, 33)
    return x, delays, np.array([1, 1, 0, 2, 1], np.float32), (46, 33, 2, 1)
