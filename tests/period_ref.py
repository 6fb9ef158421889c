"""Restatement of the FFT periodicity search (xengPeriod*), written from the contract in include/xeng.h, "FFT periodicity search of
the dedispersed beams": the segment's spectrum (mean, real DFT, power, block whitening, mask), the stack, the harmonic sums and the
record.

segment_spectrum / stacks(..., dtype) go up to A.  dtype = np.float64 is the tolerance reference (numpy.fft.rfft on float64);
dtype = np.float32 is the same contract evaluated in single precision (numpy.fft.rfft stays in single precision on float32
input), which is what the tests' bar is measured with.  harmonic_records takes ANY A and works in float32 in the contract's
order -- plain adds, j ascending, integer index arithmetic -- so on the device's own A it reproduces the records bit for bit."""
import numpy as np

NONE = (0.0, -1)                    # the record of a series and level where nothing qualified


def series(x, dtype=np.float64):
    """z of the contract from the input layout [nwindows][...][nprod]: word 0, or word 0 + word 1 in one fp32 rounding."""
    x = np.asarray(x)
    if x.shape[-1] == 1:
        return x[..., 0].astype(dtype)
    return (x[..., 0].astype(np.float32) + x[..., 1].astype(np.float32)).astype(dtype)


def segment_spectrum(z, nwhite, keep=None, dtype=np.float64):
    """z: [NT][nser], one segment.  S [nser][NT/2] by steps 1-6 of the contract."""
    z = np.asarray(z).astype(dtype)
    NT, nser = z.shape
    N = NT // 2
    keep = np.ones(N, bool) if keep is None else np.asarray(keep).astype(bool)
    with np.errstate(all='ignore'):
        mean = z.mean(axis=0, dtype=dtype)
        x = (z - mean).astype(dtype)
        X = np.fft.rfft(x, axis=0)[:N].T                        # [nser][N]
        P = (X.real.astype(dtype) ** 2 + X.imag.astype(dtype) ** 2).astype(dtype)
        counts = keep.copy()
        counts[0] = False
        S = np.ones((nser, N), dtype)
        for b in range(N // nwhite):
            sl = slice(b * nwhite, (b + 1) * nwhite)
            c = counts[sl]
            if not c.any():
                continue
            mu = P[:, sl][:, c].mean(axis=1, dtype=dtype)
            good = np.isfinite(mu) & (mu > 0)
            S[:, sl] = np.where(good[:, None], P[:, sl] / np.where(good, mu, 1)[:, None], 1.0)
        S[:, ~keep] = 1.0
        S[~np.isfinite(mean)] = np.nan
        S[:, 0] = 0.0
    return S.astype(dtype)


def stacks(z, nt, nstack, nwhite, keep=None, dtype=np.float64):
    """z: [nwindows][nser] from a reset.  The list of A [nser][nt/2], one per completed segment in order (A as xengPeriodGetSpectrum
    would read it after that segment), with the number of segments it holds: [(A, nseg)]."""
    out, A = [], None
    for s in range(z.shape[0] // nt):
        S = segment_spectrum(z[s * nt:(s + 1) * nt], nwhite, keep, dtype)
        A = S if s % nstack == 0 else (A + S).astype(dtype)
        out.append((A, s % nstack + 1))
    return out


def harmonic_sums(A, level, kmin):
    """(k, H_h[k]) for h = 2^level over h*kmin <= k < N, float32 adds in ascending j.  A: [..., N]."""
    A = np.asarray(A, np.float32)
    N, h = A.shape[-1], 1 << level
    k = np.arange(h * kmin, N)
    with np.errstate(all='ignore'):
        H = A[..., (k + h // 2) // h]
        for j in range(2, h + 1):
            H = (H + A[..., (j * k + h // 2) // h]).astype(np.float32)
    return k, H


def harmonic_records(A, nlevel, kmin):
    """The records [...][nlevel] of a completed stack A [...][N]: dict of 'H' (float32) and 'k' (int32)."""
    A = np.asarray(A, np.float32)
    Hout = np.zeros(A.shape[:-1] + (nlevel,), np.float32)
    kout = np.full(A.shape[:-1] + (nlevel,), -1, np.int32)
    for lv in range(nlevel):
        k, H = harmonic_sums(A, lv, kmin)
        ok = ~np.isnan(H)
        key = np.where(ok, H, -np.inf)
        i = key.argmax(axis=-1)                                 # (the first of equal maxima: the smallest k)
        top = np.take_along_axis(H, i[..., None], axis=-1)[..., 0]
        any_ = ok.any(axis=-1)
        i = np.where(any_ & np.isneginf(np.take_along_axis(key, i[..., None], axis=-1)[..., 0]), ok.argmax(axis=-1), i)
        top = np.take_along_axis(H, i[..., None], axis=-1)[..., 0]
        Hout[..., lv] = np.where(any_, top, 0.0)
        kout[..., lv] = np.where(any_, k[i], -1)
    return dict(H=Hout, k=kout)


def harmonic_records_naive(A, nlevel, kmin):
    """The same one term at a time: [(H, k)] per level for one series A [N]."""
    A = np.asarray(A, np.float32)
    N = A.shape[0]
    out = []
    for lv in range(nlevel):
        h = 1 << lv
        best = NONE
        for k in range(h * kmin, N):
            H = A[(k + h // 2) // h]
            for j in range(2, h + 1):
                H = np.float32(H + A[(j * k + h // 2) // h])
            if not np.isnan(H) and (best[1] < 0 or H > best[0]):
                best = (H, k)
        out.append(best)
    return out
