"""Float64 numpy restatement of UpchanSumBeams (include/xeng.h "Fine-channel power beams from live beams"): what
xengUpchanSumBeamsRun must compute, written from the contract.

A stream of voltage beams is complex [nchan][nbeam][T] (gulps of Beamform's output, cf32 [nchan][nbeam][ntime], joined along
time); samples before `first` (the first one the context has seen since its last reset) count as zero."""
import numpy as np


def beam_frames(v, nupchan, h, start, ntime, first=0):
    """y[f, c, b, n] = sum_k h[k*N + n] v[c, b, start + (f - P + 1 + k)*N + n] for the frames of [start, start + ntime),
    complex128 [nframe][nchan][nbeam][N]; h = None: the plain frames (one tap of ones)."""
    N = nupchan
    h = np.ones(N) if h is None else np.asarray(h, np.float64).reshape(-1)
    P = h.size // N
    x = np.asarray(v).astype(np.complex128)
    x[..., :max(0, first)] = 0
    nframe = ntime // N
    y = np.zeros((nframe,) + x.shape[:2] + (N,), np.complex128)
    for f in range(nframe):
        for k in range(P):
            t = start + (f - P + 1 + k) * N
            if t >= 0:
                y[f] += h[k * N:(k + 1) * N] * x[..., t:t + N]
    return y


def beam_channelise(v, nupchan, h, start, ntime, first=0):
    """V[f, c, b, j], the forward unnormalised FFT of each frame, fine channel j = (k + N/2) mod N."""
    return np.fft.fftshift(np.fft.fft(beam_frames(v, nupchan, h, start, ntime, first), axis=-1), axes=-1)


def sum_beams(V, nframe_sum, pair0=0, npair=None):
    """[XX, YY, Re XY*, Im XY*] of X = V[., ., 2p], Y = V[., ., 2p+1] summed over windows of nframe_sum frames:
    float64 [nframe / nframe_sum][npair][nchan][N][4]."""
    nframe, nchan, nbeam, N = V.shape
    if npair is None:
        npair = nbeam // 2 - pair0
    X = V[:, :, 2 * pair0:2 * (pair0 + npair):2].reshape(nframe // nframe_sum, nframe_sum, nchan, npair, N)
    Y = V[:, :, 2 * pair0 + 1:2 * (pair0 + npair):2].reshape(X.shape)
    xy = (X * np.conj(Y)).sum(axis=1)
    out = np.stack([(np.abs(X) ** 2).sum(axis=1), (np.abs(Y) ** 2).sum(axis=1), xy.real, xy.imag], axis=-1)
    return out.transpose(0, 2, 1, 3, 4)


def upchan_sum_beams(v, nupchan, nframe_sum, start, ntime, h=None, pair0=0, npair=None, first=0):
    """The windows of the frames of [start, start + ntime) (whole windows: a window of G gulps is one call over G gulps)."""
    return sum_beams(beam_channelise(v, nupchan, h, start, ntime, first), nframe_sum, pair0, npair)
