"""Float64 / int64 numpy restatement of include/xeng.h "Per-input fine-channel spectra": what xengUpchanSpectra* must compute.

A stream is u8 [T][nchan][ninput]; a gulp (or a run of gulps) is its samples [start, start + ntime); with a PFB, samples before
`first` (the first one the context has seen since its last reset) count as zero.  Per frame, coarse channel, input and fine
channel j = (k + N/2) mod N:  p = |X|^2;  per window of W frames S1 = sum p, S2 = sum p^2."""
import numpy as np

from tests.upchan_corr_ref import int_dft
from tests.upchan_pfb_ref import pfb_channelise
from tests.upchan_ref import channelise


def channelised(stream, nupchan, start, ntime, h=None, first=0):
    """complex128 X[nframe][nchan][ninput][N] of the samples [start, start + ntime): the plain FFT (h None) or the PFB h in front."""
    if h is None:
        return channelise(np.asarray(stream)[start:start + ntime], nupchan)
    return pfb_channelise(stream, nupchan, h, start, ntime, first)


def moments(X, nframe_sum):
    """X[nframe][nchan][ninput][N] -> float64 [nframe / W][2][nchan][N][ninput]: plane 0 = sum |X|^2, plane 1 = sum |X|^4."""
    p = X.real ** 2 + X.imag ** 2
    nframe = p.shape[0]
    assert nframe % nframe_sum == 0
    p = p.reshape((nframe // nframe_sum, nframe_sum) + p.shape[1:])
    out = np.stack([p.sum(axis=1), (p * p).sum(axis=1)], axis=1)         # [w][2][c][i][j]
    return np.ascontiguousarray(out.transpose(0, 1, 2, 4, 3))


def upchan_spectra(stream, nupchan, nframe_sum, start, ntime, h=None, first=0, chans=None):
    """The windows of nframe_sum frames that tile the samples [start, start + ntime) (one gulp, part of one, or several),
    float64 [nwin][2][nchan][N][ninput]; chans: only these coarse channels (in that order).  Channel by channel: the full-size
    X would be gigabytes."""
    stream = np.asarray(stream)
    chans = range(stream.shape[1]) if chans is None else chans
    return np.concatenate([moments(channelised(stream[:, c:c + 1], nupchan, start, ntime, h, first), nframe_sum) for c in chans], axis=2)


def upchan_spectra_int(vin, nupchan, nframe_sum):
    """upchan_spectra of the whole of vin by the plain FFT in int64, N in {1, 2, 4}: [nwin][2][nchan][N][ninput]."""
    ntime, nchan, ninput = vin.shape
    xr, xi = int_dft(vin, nupchan)                              # [f][c*N + j][i]
    p = xr * xr + xi * xi
    nframe = ntime // nupchan
    assert nframe % nframe_sum == 0
    p = p.reshape(nframe // nframe_sum, nframe_sum, nchan, nupchan, ninput)
    return np.stack([p.sum(axis=1), (p * p).sum(axis=1)], axis=1)
