"""The contract of xengFlag* (include/xeng.h, "Outlier flags from the fine-channel visibilities") restated in numpy: the statistics
in float64 (and in float32, whose gap to float64 on a test's own inputs is a fifth of that test's bar; and in the kernel's own
summation order, for the emulated kernels), steps 2 and 3 in float32 on a given {R, A} table -- every operation of those steps is
exact or one correctly rounded float32 operation, so the restatement is bit for bit --, the error measure, and a generator of cases
with injections."""
import numpy as np

MAD_SIGMA = 1.4826
BIT_CROSS, BIT_AUTO, BIT_CHAN, BIT_NONFINITE, BIT_WEIGHT = 1, 2, 4, 8, 16
TILE = 32


def thresholds(nsig_cross=6.0, nsig_auto=6.0, nsig_chan=6.0):
    """k = float32(nsig * 1.4826): the product in float64, rounded once"""
    return tuple(np.float32(float(n) * MAD_SIGMA) for n in (nsig_cross, nsig_auto, nsig_chan))


def _pp(V):
    """The parallel hands of the LOWER triangle as [nfine][2][nstand s][nstand t], t <= s; everything else 0 and never looked at"""
    V = np.asarray(V)
    nstand = V.shape[1]
    low = np.tril(np.ones((nstand, nstand), bool))
    return np.stack([np.where(low[None], V[:, :, p, :, p], 0) for p in range(2)], axis=1)


def power(V, w, dtype=np.float64):
    """m [nfine][2][s][t] = |V[c][s p][t p]|^2 for s != t with both weights > 0, read from the lower triangle and mirrored; 0
    elsewhere (a select: what a stand of weight 0 holds is not looked at).  float32: fma(re, re, im * im)."""
    L = _pp(V)
    nstand = L.shape[2]
    on = np.asarray(w) > 0
    keep = on[:, None] & on[None, :] & np.tril(np.ones((nstand, nstand), bool), -1)
    re = np.where(keep, L.real, 0).astype(np.float64)
    im = np.where(keep, L.imag, 0).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        if np.dtype(dtype) == np.float32:
            m = (re * re + (im.astype(np.float32) * im.astype(np.float32)).astype(np.float64)).astype(np.float32)
        else:
            m = re * re + im * im
    return m + m.transpose(0, 1, 3, 2)


def autos(V, w):
    """A [nfine][2][nstand] = Re V[c][s p][s p], +0 where w_s = 0 (exact in any precision)"""
    V = np.asarray(V)
    d = np.stack([np.einsum('css->cs', V[:, :, p, :, p]).real for p in range(2)], axis=1)
    return np.where(np.asarray(w) > 0, d, 0)


def statistics(V, w, dtype=np.float64):
    """(R, A) [nfine][2][nstand] in `dtype`.  float64: numpy's sum.  float32: the contract's sum taken term by term, the stands t in
    ascending order from +0 (a cumulative sum) -- numpy's own float32 sum is pairwise in blocks, more accurate than any evaluation
    that adds the terms one after another, so its gap to float64 would not be that of the formula evaluated in float32."""
    with np.errstate(invalid='ignore', over='ignore'):
        m = power(V, w, dtype)
        R = np.cumsum(m, axis=3, dtype=dtype)[..., -1] if np.dtype(dtype) == np.float32 else m.sum(axis=3)
    return R, autos(V, w).astype(dtype)


def statistics_kernel_order(V, w):
    """(R, A) float32 in the one summation order of include/xeng.h: tiles of 32 stands, a tile's terms from +0 in ascending t, the
    tiles' partials from +0 in ascending K"""
    m = power(V, w, np.float32)
    nstand = m.shape[2]
    R = np.zeros(m.shape[:3], np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for K in range((nstand + TILE - 1) // TILE):
            part = np.zeros(m.shape[:3], np.float32)
            for t in range(K * TILE, min(nstand, (K + 1) * TILE)):
                part = part + m[:, :, :, t]
            R = R + part
    return R, autos(V, w).astype(np.float32)


def stat_error(x, ref, w):
    """max_s |x - ref| / rms_s ref per (c, p), over the stands of weight > 0 whose reference is finite; f64 [nfine][2]"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    live = (np.asarray(w) > 0) & np.isfinite(ref)
    r = np.where(live, ref, 0)
    rms = np.sqrt((r ** 2).sum(axis=2) / np.maximum(live.sum(axis=2), 1))
    return np.abs(np.where(live, x - ref, 0)).max(axis=2) / rms


def float_gap(V, w, ref=None):
    """The float32 evaluation's stat_error against the float64 one, (R's, A's) f64 [nfine][2] each: a fifth of the float bar.  A is
    a copy of an input word, so its gap is 0: the device's A must be exact."""
    ref = statistics(V, w) if ref is None else ref
    lo = statistics(V, w, np.float32)
    return stat_error(lo[0], ref[0], w), stat_error(lo[1], ref[1], w)


def median(v):
    """Of n >= 1 float32 values: v[n / 2] of the ascending order for odd n, 0.5f * (v[(n-1) / 2] + v[n / 2]) for even n"""
    v = np.sort(np.asarray(v, np.float32))
    n = len(v)
    return v[n // 2] if n & 1 else np.float32(0.5) * (v[(n - 1) // 2] + v[n // 2])


def outliers(x, k):
    """(med, mad, d, flags) of the float32 values x: d = |x - med|, flags = d > k * mad with k > 0 (none with k = 0)"""
    x = np.asarray(x, np.float32)
    med = median(x)
    d = np.abs(x - med)
    mad = median(d)
    k = np.float32(k)
    return med, mad, d, (d > k * mad) if k > 0 else np.zeros(len(x), bool)


def flags(stats, w, k_cross, k_auto, k_chan, wchan, detail=None):
    """Steps 2 and 3 on a stats table f32 [nfine][2][nstand][2] = {R, A}: (mask u8 [nfine][2][nstand], chan f32 [nfine][2][4]).
    `detail`, a list, receives (d, threshold) float64 array pairs of every test that was taken."""
    stats = np.asarray(stats, np.float32)
    nfine, _, nstand, _ = stats.shape
    on = np.asarray(w) > 0
    mask = np.zeros((nfine, 2, nstand), np.uint8)
    chan = np.zeros((nfine, 2, 4), np.float32)
    mask[:, :, ~on] |= BIT_WEIGHT
    for c in range(nfine):
        for p in range(2):
            R, A = stats[c, p, :, 0], stats[c, p, :, 1]
            fin = np.isfinite(R) & np.isfinite(A)
            mask[c, p, on & ~fin] |= BIT_NONFINITE
            L = np.flatnonzero(on & fin)
            chan[c, p, 3] = len(L)
            if len(L) < 4:
                continue
            for x, k, bit in ((R, k_cross, BIT_CROSS), (A, k_auto, BIT_AUTO)):
                med, mad, d, out = outliers(x[L], k)
                mask[c, p, L[out]] |= bit
                if bit == BIT_CROSS:
                    chan[c, p, 0], chan[c, p, 1] = med, mad
                if detail is not None and np.float32(k) > 0:
                    detail.append((d.astype(np.float64), np.full(len(d), float(np.float32(k) * mad))))
    k_chan = np.float32(k_chan)
    for p in range(2):
        has = np.flatnonzero(chan[:, p, 3] >= 4)
        mask[chan[:, p, 3] < 4, p, :] |= BIT_CHAN
        if not len(has):
            continue
        y = chan[:, p, 0]
        if wchan == 0:
            b = np.full(len(has), median(y[has]), np.float32)
        else:
            b = np.array([median(y[has[(has >= c - wchan) & (has <= c + wchan)]]) for c in has], np.float32)
        chan[has, p, 2] = b
        ar = np.abs(y[has] - b)
        m = median(ar)
        if k_chan > 0:
            mask[has[ar > k_chan * m], p, :] |= BIT_CHAN
            if detail is not None:
                detail.append((ar.astype(np.float64), np.full(len(ar), float(k_chan * m))))
    return mask, chan


def margin(detail):
    """The least |d - threshold| / threshold over every test taken (inf where the threshold is 0 and d is not)"""
    worst = np.inf
    for d, thr in detail:
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = np.where(thr > 0, np.abs(d - thr) / np.where(thr > 0, thr, 1), np.where(d > 0, np.inf, 0.0))
        worst = min(worst, float(rel.min()))
    return worst


def case(nstand, nfine, seed=None, ntime=1024, spread=0.05, noise=0.1):
    """V complex64 [nfine][nstand][2][nstand][2] = G (sky + noise) G^H as a correlator forms it: ntime samples of x = g o (a s + n)
    per input, one point source of unit flux per polarisation (independent in the two), noise of variance `noise`, gains of
    modulus uniform in 1 +- spread and any phase, V = x x^H / ntime.  The sky dominates the cross-power, so R_s is |g_s|^2 times a
    sum that all stands share nearly: the spread of R and A over the stands is that of |g|^2, bounded by 1 +- 2 spread, and the
    spread of y over the channels is that of the source's sampled flux, about 2 / sqrt(ntime)."""
    rng = np.random.default_rng(300 + nstand if seed is None else seed)
    n = 2 * nstand
    g = (1 + spread * rng.uniform(-1, 1, (nfine, n))) * np.exp(2j * np.pi * rng.uniform(0, 1, (nfine, n)))
    a = np.exp(2j * np.pi * rng.uniform(0, 1, (nfine, nstand)))
    V = np.empty((nfine, n, n), np.complex64)
    for c in range(nfine):
        s = (rng.standard_normal((2, ntime)) + 1j * rng.standard_normal((2, ntime))) / np.sqrt(2)
        x = (a[c][:, None, None] * s[None]).reshape(n, ntime)
        x = x + np.sqrt(noise / 2) * (rng.standard_normal((n, ntime)) + 1j * rng.standard_normal((n, ntime)))
        x = g[c][:, None] * x
        V[c] = (x @ np.conj(x.T) / ntime).astype(np.complex64)
    return V.reshape(nfine, nstand, 2, nstand, 2)


def scale_stand(V, c, s, f):
    """Stand s's voltages times f in channel c: its rows and columns times f, its own 2 x 2 block times f^2 (in place)"""
    with np.errstate(invalid='ignore'):
        V[c, s] *= np.float32(f)
        V[c, :, :, s] *= np.float32(f)


def scale_channel(V, c, f):
    """Every stand's voltages times f in channel c (in place)"""
    with np.errstate(invalid='ignore'):
        V[c] *= np.float32(f * f)


def scale_auto(V, s, f):
    """Stand s's autos (both polarisations, every channel) times f; nothing else (in place)"""
    with np.errstate(invalid='ignore'):
        for p in range(2):
            V[:, s, p, s, p] *= np.float32(f)


def upper_and_cross_nan(V):
    """A copy of V with every word above the diagonal and every cross-hand word NaN: nothing may look at them"""
    V = np.array(V, np.complex64)
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    bad = np.triu(np.ones((n, n), bool), 1).reshape(nstand, 2, nstand, 2)
    bad[:, 0, :, 1] = True
    bad[:, 1, :, 0] = True
    V[:, bad] = np.complex64(complex(np.nan, np.nan))
    return V
