"""float64 / int64 restatement of the incoherent dedisperser, written from the contract in include/xeng.h ("Incoherent
dedispersion of fine-channel power beams"), not from the kernel:

    y[n][p][d] = sum_q w[q] * x[n - b[d][q]][p][q],   b[d][q] = S - s[d][q],  S = max s,

n counting windows since the last reset, terms with a negative time index counting as zero and channels whose weight is exactly
0 left out (whatever they hold).  nprod = 1: x = XX + YY; nprod = 4: the four words, each by itself.

dedisperse_ordered32 is the same sum in the contract's evaluation order and in explicit float32 steps (the "Numerics" paragraph),
for holding float data bit for bit; its fused multiply-add is the correctly rounded fmaf32 of tests/fold_ref.py."""
import numpy as np

from tests.fold_ref import fmaf32, products32


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


def dedisperse_ordered32(x, delays, weights=None, nprod=1):
    """The contract's evaluation order ("Numerics" in include/xeng.h) in explicit float32 steps, so that float data can be held
    bit for bit: I = fl(XX + YY) in one rounding; the channels cut into 4 segments of Q = ceil(nfine / 4), segment k =
    [k*Q, min((k+1)*Q, nfine)); P_k from +0 over its channels in ascending q, one correctly rounded fmaf(w[q], x, sum) each, a
    term that counts as zero or is left out entering as fmaf(w[q], +0, sum) (what the left-out channel holds is never looked
    at); y = ((P_0 + P_1) + P_2) + P_3.  x: every window since the reset; returns float32 [nwindows][npair][ndm][nprod]."""
    x = np.asarray(x, np.float32)
    s = np.asarray(delays, np.int64)
    nwindows, npair, nfine, _ = x.shape
    ndm = s.shape[0]
    assert s.shape == (ndm, nfine) and s.min() >= 0
    w = np.ones(nfine, np.float32) if weights is None else np.asarray(weights, np.float32)
    keep = w != 0
    v = np.zeros((nwindows, npair, nfine, nprod), np.float32)
    v[:, :, keep] = products32(x[:, :, keep], nprod)
    b = s.max() - s
    Q = -(-nfine // 4)
    y = np.zeros((nwindows, npair, ndm, nprod), np.float32)
    for d in range(ndm):
        P = []
        for k in range(4):
            acc = np.zeros((nwindows, npair, nprod), np.float32)
            for q in range(k * Q, min((k + 1) * Q, nfine)):
                term = np.zeros_like(acc)
                back = int(b[d, q])
                if keep[q] and back < nwindows:
                    term[back:] = v[:nwindows - back, :, q]
                acc = fmaf32(w[q], term, acc)
            P.append(acc)
        y[:, :, d] = ((P[0] + P[1]) + P[2]) + P[3]          # (float32 + float32: one rounding each)
    return y


def dedisperse_one_chain32(x, delays, weights=None, nprod=1):
    """NOT the contract: one ascending chain of fmaf over all channels.  Only there to show that data can tell the orders apart."""
    x = np.asarray(x, np.float32)
    s = np.asarray(delays, np.int64)
    nwindows, npair, nfine, _ = x.shape
    w = np.ones(nfine, np.float32) if weights is None else np.asarray(weights, np.float32)
    v = np.zeros((nwindows, npair, nfine, nprod), np.float32)
    v[:, :, w != 0] = products32(x[:, :, w != 0], nprod)
    b = s.max() - s
    y = np.zeros((nwindows, npair, s.shape[0], nprod), np.float32)
    for d in range(s.shape[0]):
        acc = np.zeros((nwindows, npair, nprod), np.float32)
        for q in range(nfine):
            term = np.zeros_like(acc)
            if w[q] != 0 and b[d, q] < nwindows:
                term[int(b[d, q]):] = v[:nwindows - int(b[d, q]), :, q]
            acc = fmaf32(w[q], term, acc)
        y[:, :, d] = acc
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
