"""float64 / int64 restatement of the incoherent dedisperser, written from the contract in include/xeng.h ("Incoherent
dedispersion of fine-channel power beams"), not from the kernel:

    y[n][p][d] = sum_q w[q] * x[n - b[d][q]][p][q],   b[d][q] = S - s[d][q],  S = max s,

n counting windows since the last reset, terms with a negative time index counting as zero and channels whose weight is exactly
0 left out (whatever they hold).  nprod = 1: x = XX + YY; nprod = 4: the four words, each by itself."""
import numpy as np


def products(x, nprod, dtype=np.float64):
    """[..., 4] -> [..., nprod] in `dtype`."""
    x = np.asarray(x)
    if nprod == 1:
        return (x[..., 0].astype(dtype) + x[..., 1].astype(dtype))[..., None]
    assert nprod == 4
    return x.astype(dtype)


def dedisperse(x, delays, weights=None, nprod=1, dtype=np.float64, absolute=False):
    """x: [nwindows][npair][nfine][4], every window since the reset; delays: int [ndm][nfine]; weights: [nfine] or None.
    Returns y [nwindows][npair][ndm][nprod] in `dtype` (np.int64: integer-valued data and weights, exact).  absolute: the sum
    of |w * x| instead (the scale of the a-priori error bound of an fp32 sum)."""
    x = np.asarray(x)
    s = np.asarray(delays, np.int64)
    nwindows, npair, nfine, _ = x.shape
    ndm = s.shape[0]
    assert s.shape == (ndm, nfine) and s.min() >= 0
    w = np.ones(nfine) if weights is None else np.asarray(weights, np.float64)
    keep = w != 0
    if dtype == np.int64:
        assert np.array_equal(w, np.rint(w))
        xk = x[:, :, keep]
        assert np.array_equal(xk, np.rint(xk))
    v = np.zeros((nwindows, npair, nfine, nprod), dtype)
    v[:, :, keep] = products(x[:, :, keep], nprod, dtype)         # (what a left-out channel holds is never looked at)
    w = w.astype(dtype)
    if absolute:
        v, w = np.abs(v), np.abs(w)
    b = s.max() - s
    y = np.zeros((nwindows, npair, ndm, nprod), dtype)
    for d in range(ndm):
        for back in np.unique(b[d]):
            sel = (b[d] == back) & keep
            if back >= nwindows or not sel.any():
                continue
            # windows n >= back take window n - back of these channels
            y[back:, :, d] += np.einsum('npqk,q->npk', v[:nwindows - back, :, sel], w[sel])
    return y


def dedisperse_naive(x, delays, weights=None, nprod=1):
    """The same by the definition, one term at a time (small sizes only)."""
    x = np.asarray(x, np.float64)
    s = np.asarray(delays)
    nwindows, npair, nfine, _ = x.shape
    ndm = s.shape[0]
    S = int(s.max())
    y = np.zeros((nwindows, npair, ndm, nprod))
    for n in range(nwindows):
        for d in range(ndm):
            for q in range(nfine):
                wq = 1.0 if weights is None else float(weights[q])
                m = n - (S - int(s[d, q]))
                if wq == 0 or m < 0:
                    continue
                for p in range(npair):
                    if nprod == 1:
                        y[n, p, d, 0] += wq * (x[m, p, q, 0] + x[m, p, q, 1])
                    else:
                        y[n, p, d] += wq * x[m, p, q]
    return y
