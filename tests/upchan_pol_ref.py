"""Float64 restatement of UpchanBeamform's dual-pol mode (include/xeng.h xengUpchanInitializeDualPol): the voltages of
tests/upchan_ref.py, beams 2p / 2p+1 taken as X / Y, and their 2x2 products summed over each window of frames in
BeamformSumBeams's convention (the reference's beamformer_sum_test.py:64-77)."""
import numpy as np

from tests.upchan_ref import upchan_beamform


def upchan_dual_pol(vin, w, nupchan, nbeam, nframe_sum):
    """float64 [nframe / nframe_sum][nbeam / 2][nchan][nupchan][4] = [XX, YY, Re(XY*), Im(XY*)], X = v[f, 2p, c, j],
    Y = v[f, 2p+1, c, j], each a sum over the nframe_sum frames of a window."""
    v = upchan_beamform(vin, w, nupchan, nbeam, 0)                      # [nframe][nbeam][nchan][N]
    nframe, _, nchan, N = v.shape
    v = v.reshape(nframe // nframe_sum, nframe_sum, nbeam // 2, 2, nchan, N)
    X, Y = v[:, :, :, 0], v[:, :, :, 1]
    xy = (X * np.conj(Y)).sum(axis=1)
    return np.stack([(np.abs(X) ** 2).sum(axis=1), (np.abs(Y) ** 2).sum(axis=1), xy.real, xy.imag], axis=-1)
