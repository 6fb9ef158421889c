"""Restatement of the long-segment FFT periodicity search (xengPlong*), written from the contract in include/xeng.h, "FFT periodicity
search with long segments".  Steps 1-6 and the stack are those of xengPeriod*, and tests/period_ref.py, which is size-agnostic,
restates them: series / segment_spectrum / stacks are its functions.  What is new is the bands: per level h = 2^l and band b the
record is the largest H_h[k] over h*kedge[b] <= k < min(h*kedge[b+1], N), among equal sums the smallest k, {+0, -1} where the band
is empty or all NaN.  harmonic_records takes ANY A and works in float32 in the contract's order, so on the device's own A it
reproduces the records bit for bit; harmonic_records_naive is the same one term at a time."""
import numpy as np

from tests.period_ref import NONE, harmonic_sums, segment_spectrum, series, stacks  # noqa: F401

RECORD = np.dtype([('H', '<f4'), ('k', '<i4')])


def band_range(kedge, b, level, N):
    """[lo, hi) of the top-harmonic bins of band b at level `level`."""
    h = 1 << level
    return h * int(kedge[b]), min(h * int(kedge[b + 1]), N)


def harmonic_records(A, nlevel, kedge):
    """The records [...][nlevel][nband] of a completed stack A [...][N]: dict of 'H' (float32) and 'k' (int32)."""
    A = np.asarray(A, np.float32)
    N, nband = A.shape[-1], len(kedge) - 1
    Hout = np.zeros(A.shape[:-1] + (nlevel, nband), np.float32)
    kout = np.full(A.shape[:-1] + (nlevel, nband), -1, np.int32)
    for lv in range(nlevel):
        k, H = harmonic_sums(A, lv, int(kedge[0]))              # k from h * kedge[0] to N - 1
        for b in range(nband):
            lo, hi = band_range(kedge, b, lv, N)
            if lo >= hi:
                continue
            Hb, kb = H[..., lo - k[0]:hi - k[0]], k[lo - k[0]:hi - k[0]]
            ok = ~np.isnan(Hb)
            key = np.where(ok, Hb, -np.inf)
            i = key.argmax(axis=-1)                             # (the first of equal maxima: the smallest k)
            any_ = ok.any(axis=-1)
            # (a band whose only numbers are -inf: the first of them)
            i = np.where(any_ & np.isneginf(np.take_along_axis(key, i[..., None], axis=-1)[..., 0]), ok.argmax(axis=-1), i)
            top = np.take_along_axis(Hb, i[..., None], axis=-1)[..., 0]
            Hout[..., lv, b] = np.where(any_, top, 0.0)
            kout[..., lv, b] = np.where(any_, kb[i], -1)
    return dict(H=Hout, k=kout)


def harmonic_records_naive(A, nlevel, kedge):
    """The same one term at a time: [[(H, k)] per band] per level for one series A [N]."""
    A = np.asarray(A, np.float32)
    N = A.shape[0]
    out = []
    for lv in range(nlevel):
        h = 1 << lv
        row = []
        for b in range(len(kedge) - 1):
            best = NONE
            for k in range(*band_range(kedge, b, lv, N)):
                H = A[(k + h // 2) // h]
                for j in range(2, h + 1):
                    H = np.float32(H + A[(j * k + h // 2) // h])
                if not np.isnan(H) and (best[1] < 0 or H > best[0]):
                    best = (H, k)
            row.append(best)
        out.append(row)
    return out


def plane_of(rec):
    out = np.zeros(rec['k'].shape, RECORD)
    out['H'], out['k'] = rec['H'], rec['k']
    return out


def float_gap(nt, nser, nwhite, seed):
    """The worst |A32 - A64| / max(1, A64) of the float32 numpy evaluation of the contract against the float64 one: one segment of
    nser series of chi^2 powers with mean / sigma = 55.  What the tolerance of the device tests is measured with."""
    rng = np.random.default_rng(seed)
    z = (rng.chisquare(2 * 55 ** 2, (nt, nser)) * rng.uniform(0.5, 1.5, nser)).astype(np.float32)
    (A64, _), = stacks(z, nt, 1, nwhite, None, np.float64)
    (A32, _), = stacks(z, nt, 1, nwhite, None, np.float32)
    return float((np.abs(A32.astype(np.float64) - A64) / np.maximum(1.0, A64)).max())
