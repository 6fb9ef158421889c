"""Float64 numpy restatement of the polyphase filter bank front end of UpchanBeamform and UpchanCorr (include/xeng.h
xengUpchanSetPfb), in the conventions of tests/upchan_ref.py and tests/upchan_corr_ref.py: what the PFB kernels must compute.

A stream is u8 [T][nchan][ninput]; a gulp is its samples [start, start + ntime); samples before `first` (the first one the
context has seen since its last reset) count as zero."""
import numpy as np

from oracle import xeng_oracle as orc


def pfb_frames(stream, nupchan, h, start, ntime, first=0):
    """y[f, n] = sum_k h[k*N + n] x[(f - P + 1 + k)*N + n] for the frames of the gulp, complex128 [nframe][nchan][ninput][N]."""
    N = nupchan
    h = np.asarray(h, np.float64).reshape(-1)
    P = h.size // N
    re, im = orc.decode(np.asarray(stream))
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    x[:max(0, first)] = 0
    nframe = ntime // N
    y = np.zeros((nframe, N) + x.shape[1:], np.complex128)
    for f in range(nframe):
        for k in range(P):
            t = start + (f - P + 1 + k) * N
            if t >= 0:
                y[f] += h[k * N:(k + 1) * N, None, None] * x[t:t + N]
    return y.transpose(0, 2, 3, 1)


def pfb_channelise(stream, nupchan, h, start, ntime, first=0):
    """channelise() of tests/upchan_ref.py with the PFB in front: complex128 X[nframe][nchan][ninput][N], fine channel
    j = (k + N/2) mod N."""
    return np.fft.fftshift(np.fft.fft(pfb_frames(stream, nupchan, h, start, ntime, first), axis=-1), axes=-1)


def upchan_beamform_pfb(stream, w, nupchan, nbeam, h, start, ntime, nframe_sum=0, first=0, dual_pol=False):
    """upchan_beamform() (and upchan_dual_pol()) of the gulp through the PFB: voltage complex128 [nframe][nbeam][nchan][N],
    power float64 [nframe / nframe_sum][nbeam][nchan][N], dual-pol float64 [nframe / nframe_sum][nbeam / 2][nchan][N][4]."""
    X = pfb_channelise(stream, nupchan, h, start, ntime, first)          # [f][c][i][j]
    nframe, nchan, ninput, N = X.shape
    w = np.asarray(w).reshape(nchan, N, nbeam, ninput).astype(np.complex128)
    v = np.einsum('cjbi,fcij->fbcj', w, X, optimize=True)
    if not nframe_sum:
        return v
    if dual_pol:
        v = v.reshape(nframe // nframe_sum, nframe_sum, nbeam // 2, 2, nchan, N)
        Xp, Yp = v[:, :, :, 0], v[:, :, :, 1]
        xy = (Xp * np.conj(Yp)).sum(axis=1)
        return np.stack([(np.abs(Xp) ** 2).sum(axis=1), (np.abs(Yp) ** 2).sum(axis=1), xy.real, xy.imag], axis=-1)
    return (np.abs(v) ** 2).reshape(nframe // nframe_sum, nframe_sum, nbeam, nchan, N).sum(axis=1)


def pfb_fine_select(stream, nupchan, h, start, ntime, fine_lo=0, fine_hi=None, first=0):
    """fine_select() of tests/upchan_corr_ref.py through the PFB: complex128 X[nframe][nfine][ninput]."""
    X = pfb_channelise(stream, nupchan, h, start, ntime, first)          # [f][c][i][j]
    nframe, nchan, ninput, N = X.shape
    X = X.transpose(0, 1, 3, 2).reshape(nframe, nchan * N, ninput)
    return X[:, fine_lo:fine_hi if fine_hi is not None else nchan * N]


def upchan_corr_pfb(Xs):
    """V[c', i, j] = sum_f X[f, c', i] conj(X[f, c', j]) over the frames of X[f][c'][i] (pfb_fine_select, concatenated over the
    gulps of an integration), with the scale of the fp32 tolerance, sum_f |X_i| |X_j|."""
    A = np.abs(Xs)
    return np.einsum('fci,fcj->cij', Xs, Xs.conj(), optimize=True), np.einsum('fci,fcj->cij', A, A, optimize=True)


def tone_leakage_db(h, nupchan, offsets=np.linspace(0.0, 0.5, 51)):
    """Steady-state leakage of a complex tone through the filter h (the plain FFT: h = ones(N)), in float64: a tone at
    `offset` fine channels above channel 0 gives channel k the response |sum_m h[m] exp(2 pi i (offset - k) m / N)|; the
    result is the worst over the offsets of the largest power in channels >= 2 away from channel 0, relative to the peak."""
    h = np.asarray(h, np.float64).reshape(-1)
    N = nupchan
    m = np.arange(h.size)
    k = np.arange(N)
    far = np.minimum(k, N - k) >= 2
    worst = -np.inf
    for d in offsets:
        r = np.abs(np.exp(2j * np.pi * (d - k[:, None]) * m[None, :] / N) @ h) ** 2
        worst = max(worst, 10 * np.log10(r[far].max() / r.max()))
    return worst
