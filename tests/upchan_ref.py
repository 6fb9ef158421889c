"""Float64 numpy restatement of the reference's upchannelising beamformer chain (pipeline/scripts/lwa352-upchan-bf.py:94-113
with pipeline/lwa352_pipeline/blocks/beamform_offline_block.py:211-245), in the conventions of include/xeng.h
"Upchannelising beamformer": what xengUpchan* must compute."""
import numpy as np

from oracle import xeng_oracle as orc


def channelise(vin, nupchan):
    """u8[ntime][nchan][ninput] -> complex128 X[nframe][nchan][ninput][nupchan] in fine-channel order j = (k + N/2) mod N.
    Decode (corr_block.py:270-275 via orc.decode), frames of nupchan consecutive samples (TrigBufSourceBlock(frame_size=
    NUPCHAN), :94), transpose the frame's samples to the last axis (blocks.transpose(..., 'fine_time'), :96), forward FFT over
    them (blocks.fft(axes='fine_time'), :97: exp(-2 pi i k n / N), no normalisation), then fftshift, so that fine channels
    ascend in frequency (the order the offline block's weights assume, beamform_offline_block.py:156)."""
    ntime, nchan, ninput = vin.shape
    re, im = orc.decode(vin)
    x = (re.astype(np.float64) + 1j * im.astype(np.float64)).reshape(ntime // nupchan, nupchan, nchan, ninput)
    X = np.fft.fft(x.transpose(0, 2, 3, 1), axis=-1)
    return np.fft.fftshift(X, axes=-1)


def upchan_beamform(vin, w, nupchan, nbeam, nframe_sum=0):
    """Beams: w cf32[nchan][nupchan][nbeam][ninput].  The weighting (BFmap "a = a * b", :242) and the sums over stand and
    pol (blocks.reduce, lwa352-upchan-bf.py:112-113) as one sum over inputs, with the beam axis filled in (the reference's
    TODO at :214-215).  nframe_sum 0: complex128 v[nframe][nbeam][nchan][nupchan]; > 0: sum of |v|^2 over nframe_sum
    consecutive frames, float64 [nframe / nframe_sum][nbeam][nchan][nupchan] (power, not the reference's np.abs)."""
    ntime, nchan, ninput = vin.shape
    nframe = ntime // nupchan
    w = np.asarray(w).reshape(nchan, nupchan, nbeam, ninput).astype(np.complex128)
    v = np.empty((nframe, nbeam, nchan, nupchan), np.complex128)
    for c in range(nchan):                      # (channel by channel: the full-size X would be 1 GB)
        X = channelise(vin[:, c:c + 1, :], nupchan)[:, 0]                   # [f][i][j]
        v[:, :, c, :] = np.einsum('jbi,fij->fbj', w[c], X, optimize=True)
    if not nframe_sum:
        return v
    p = (v.real ** 2 + v.imag ** 2).reshape(nframe // nframe_sum, nframe_sum, nbeam, nchan, nupchan)
    return p.sum(axis=1)


def fine_freqs(sfreq, bw_hz, nchan, nupchan):
    """Centre frequency of fine channel j of coarse channel c: sfreq + c*d + (j - N/2)*d/N, d = bw_hz / nchan; [nchan][N]."""
    d = bw_hz / nchan
    return sfreq + d * np.arange(nchan)[:, None] + (np.arange(nupchan)[None, :] - nupchan // 2) * d / nupchan


def upchan_weights(freqs, delays_ns, amps, cal):
    """UpchanBeamform's weight of one beam: amps * exp(2 pi i f tau 1e-9) * cal (Beamform's formula, beamform_block.py:340-342,
    at fine frequencies); freqs [nchan][N], delays / amps [ninput], cal [nchan][N][ninput] -> [nchan][N][ninput]."""
    return amps * np.exp(2j * np.pi * freqs[:, :, None] * np.asarray(delays_ns)[None, None, :] * 1e-9) * cal
