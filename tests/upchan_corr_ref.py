"""Float64 numpy restatement of the reference's upchannelised imaging chain (pipeline/scripts/lwa352-upchan-imag.py:95-106:
fft over fine_time, merge_axes(freq, fine_freq), FrequencySelectBlock, blocks.correlate), in the conventions of include/xeng.h
"Upchannelised correlator": what xengUpchanCorr* must compute."""
import numpy as np

from oracle import xeng_oracle as orc
from tests.upchan_ref import channelise


def fine_select(vin, nupchan, fine_lo=0, fine_hi=None):
    """u8[ntime][nchan][ninput] -> complex128 X[nframe][nfine][ninput]: channelise, merge (coarse, fine) into c*N + j, keep
    [fine_lo, fine_hi)."""
    ntime, nchan, ninput = vin.shape
    X = channelise(vin, nupchan)                                # [f][c][i][j]
    X = X.transpose(0, 1, 3, 2).reshape(ntime // nupchan, nchan * nupchan, ninput)
    return X[:, fine_lo:fine_hi if fine_hi is not None else nchan * nupchan]


def upchan_corr(vin, nupchan, fine_lo=0, fine_hi=None):
    """V[c', i, j] = sum_f X[f, c', i] conj(X[f, c', j]) over every frame of vin, complex128 [nfine][ninput][ninput]."""
    X = fine_select(vin, nupchan, fine_lo, fine_hi)
    return np.einsum('fci,fcj->cij', X, X.conj(), optimize=True)


def upchan_corr_scale(vin, nupchan, fine_lo=0, fine_hi=None):
    """sum_f |X_i| |X_j| per element, [nfine][ninput][ninput]: the scale of the fp32 tolerance."""
    A = np.abs(fine_select(vin, nupchan, fine_lo, fine_hi))
    return np.einsum('fci,fcj->cij', A, A, optimize=True)


def int_dft(vin, nupchan):
    """The same channelisation in int64 for N in {1, 2, 4}, whose twiddles are 1, -i, -1, i: (re, im) [nframe][nchan*N][ninput]."""
    assert nupchan in (1, 2, 4)
    ntime, nchan, ninput = vin.shape
    re, im = orc.decode(vin)
    x_re = re.astype(np.int64).reshape(ntime // nupchan, nupchan, nchan, ninput)
    x_im = im.astype(np.int64).reshape(ntime // nupchan, nupchan, nchan, ninput)
    out_re = np.zeros((ntime // nupchan, nchan, nupchan, ninput), np.int64)
    out_im = np.zeros_like(out_re)
    for j in range(nupchan):
        k = (j + nupchan // 2) % nupchan
        for n in range(nupchan):
            # exp(-2 pi i k n / N) = (-i)^(4 k n / N)
            q = (4 * k * n // nupchan) % 4
            wr, wi = [(1, 0), (0, -1), (-1, 0), (0, 1)][q]
            out_re[:, :, j] += wr * x_re[:, n] - wi * x_im[:, n]
            out_im[:, :, j] += wr * x_im[:, n] + wi * x_re[:, n]
    return out_re.reshape(ntime // nupchan, nchan * nupchan, ninput), out_im.reshape(ntime // nupchan, nchan * nupchan, ninput)


def upchan_corr_int(vin, nupchan, fine_lo=0, fine_hi=None):
    """upchan_corr in int64 for N in {1, 2, 4}: (re, im) [nfine][ninput][ninput]."""
    xr, xi = int_dft(vin, nupchan)
    sl = slice(fine_lo, fine_hi)
    xr, xi = xr[:, sl], xi[:, sl]
    re = np.einsum('fci,fcj->cij', xr, xr) + np.einsum('fci,fcj->cij', xi, xi)
    im = np.einsum('fci,fcj->cij', xi, xr) - np.einsum('fci,fcj->cij', xr, xi)
    return re, im


def fine_freqs(sfreq, bw_hz, nchan, nupchan, fine_lo=0, fine_hi=None):
    """Centre frequency of merged fine channel c*N + j: sfreq + c*d + (j - N/2)*d/N, d = bw_hz / nchan, for [fine_lo, fine_hi)."""
    d = bw_hz / nchan
    m = np.arange(nchan * nupchan)[fine_lo:fine_hi]
    return sfreq + d * (m // nupchan) + (m % nupchan - nupchan // 2) * d / nupchan
