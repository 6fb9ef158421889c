"""The contract of xengCdedisp* (include/xeng.h, "Coherent dedispersion of the voltage beams") restated in numpy: float64 by
default, complex64 with a dtype argument (numpy's single-precision FFT), and a fake backend that serves the calls
BeamCoherentDedisperse makes from the restatement."""
import numpy as np

from tests.fake_backend import OracleBackend


def nblocks_after(nsamples, nfft, overlap):
    """Blocks complete once `nsamples` samples have arrived since the reset."""
    return 0 if nsamples < nfft else (nsamples - nfft) // (nfft - overlap) + 1


def select(x, pair0, npair):
    """[nchan][nbeam][n] -> the selected beams [nchan][2 npair][n]"""
    return x[:, 2 * pair0:2 * (pair0 + npair)]


def filter_blocks(rows, table, nfft, overlap, dtype=np.complex128, first=0, count=None):
    """rows: complex [nchan][2 npair][n], the selected beams from the reset on.  table: complex [npair][nchan][nfft], natural DFT
    order, 1/nfft included.  Returns [nblk][nchan][2 npair][L], blocks first .. first + count - 1 (all complete ones by default):
    block j is samples [j L, j L + nfft), transformed, multiplied, transformed back without a further scale, cut to
    [overlap/2, overlap/2 + L)."""
    dtype = np.dtype(dtype)
    nchan, nb, n = rows.shape
    L = nfft - overlap
    total = nblocks_after(n, nfft, overlap)
    count = total - first if count is None else count
    assert first + count <= total
    T = np.repeat(np.transpose(np.asarray(table), (1, 0, 2)), 2, axis=1).astype(dtype)       # [nchan][2 npair][nfft]
    out = np.empty((count, nchan, nb, L), dtype)
    for i in range(count):
        j = first + i
        x = np.ascontiguousarray(rows[:, :, j * L:j * L + nfft]).astype(dtype)
        with np.errstate(invalid='ignore', over='ignore'):
            X = np.fft.fft(x, axis=-1)
            assert X.dtype == dtype
            y = np.fft.ifft((X * T).astype(dtype), axis=-1, norm="forward")     # (norm="forward": the inverse is not scaled)
        assert y.dtype == dtype
        out[i] = y[:, :, overlap // 2:overlap // 2 + L]
    return out


def row_error(got, ref):
    """max |got - ref| / rms(ref) per (block, channel, beam) over the last axis; 0 where both are all zero."""
    ref = np.asarray(ref, np.complex128)
    d = np.max(np.abs(np.asarray(got, np.complex128) - ref), axis=-1)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1))
    return np.where(rms > 0, d / np.where(rms > 0, rms, 1), np.where(d > 0, np.inf, 0.0))


def float_gap(rows, table, nfft, overlap):
    """The worst row_error of the complex64 evaluation against the float64 one: a fifth of the float bar."""
    return float(np.max(row_error(filter_blocks(rows, table, nfft, overlap, np.complex64), filter_blocks(rows, table, nfft, overlap))))


def unit_tables(rng, npair, nchan, nfft):
    """Unit-modulus tables of random phase, 1/nfft included: complex64 [npair][nchan][nfft]"""
    return (np.exp(2j * np.pi * rng.uniform(size=(npair, nchan, nfft))) / nfft).astype(np.complex64)


def gaussian_rows(rng, nchan, nbeam, n, lo=0.5, hi=50.0):
    """Gaussian voltages, every (channel, beam) row at a scale of its own between lo and hi: complex64 [nchan][nbeam][n]"""
    scale = np.exp(rng.uniform(np.log(lo), np.log(hi), (nchan, nbeam, 1)))
    return ((rng.standard_normal((nchan, nbeam, n)) + 1j * rng.standard_normal((nchan, nbeam, n))) * scale).astype(np.complex64)


def disperse(x, freq_hz, chan_bw_hz, dm, kdm):
    """The interstellar medium on one coarse channel in float64: x complex [n] (a whole, circular record, critically sampled at
    chan_bw_hz around freq_hz) multiplied in the frequency domain by exp(+2 pi i KDM DM nu^2 / (f_c^2 (f_c + nu))) (nu, f_c in MHz,
    the seconds * MHz factor 10^6 applied): the conjugate of the filter chirp_table builds."""
    n = x.shape[-1]
    nu = np.fft.fftfreq(n) * chan_bw_hz * 1e-6
    fc = freq_hz * 1e-6
    H = np.exp(2j * np.pi * 1e6 * kdm * dm * nu ** 2 / (fc ** 2 * (fc + nu)))
    return np.fft.ifft(np.fft.fft(np.asarray(x, np.complex128)) * H)


class CdedispBackend(OracleBackend):
    """The oracle backend plus xengCdedisp* served by the complex64 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.cd, self.calls = None, []

    def cdedisp_initialize(self, gpu, nchan, nbeam, ntime, pair0, npair, nfft, overlap):
        self.cd = dict(nchan=nchan, nbeam=nbeam, ntime=ntime, pair0=pair0, npair=npair, nfft=nfft, overlap=overlap)
        self.table = np.full((npair, nchan, nfft), 1.0 / nfft, np.complex64)
        self.buf = np.zeros((nchan, 2 * npair, 0), np.complex64)
        self.nsamples = self.nblocks = 0
        self.calls.append('init')
        return 0

    def cdedisp_set_chirp(self, table):
        u = self.cd
        self.table = np.array(table, np.complex64).reshape(u['npair'], u['nchan'], u['nfft'])
        self.calls.append('chirp')
        return 0

    def cdedisp_info(self):
        u = self.cd
        L = u['nfft'] - u['overlap']
        return L, -(-u['ntime'] // L), self.nsamples, self.nblocks

    def cdedisp_run(self, in_arr, out_arr):
        u = self.cd
        L = u['nfft'] - u['overlap']
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.complex64).reshape(u['nchan'], u['nbeam'], u['ntime'])
        self.buf = np.concatenate([self.buf, select(x, u['pair0'], u['npair'])], axis=2)
        self.nsamples += u['ntime']
        nb = nblocks_after(self.nsamples, u['nfft'], u['overlap']) - self.nblocks
        if nb:
            y = filter_blocks(self.buf, self.table, u['nfft'], u['overlap'], np.complex64, 0, nb)
            out_arr.numpy().reshape(-1).view(np.uint8)[:y.nbytes] = y.reshape(-1).view(np.uint8)
            self.buf = self.buf[:, :, nb * L:]     # (block j + 1 starts L samples behind block j)
            self.nblocks += nb
        self.calls.append('run%d' % nb)
        return 0, nb

    def cdedisp_reset(self):
        u = self.cd
        self.buf = np.zeros((u['nchan'], 2 * u['npair'], 0), np.complex64)
        self.nsamples = self.nblocks = 0
        self.calls.append('reset')

    def cdedisp_mark(self):
        return self.beam_mark()

    def cdedisp_wait(self, ticket):
        self.beam_wait(ticket)

    def cdedisp_sync(self):
        pass
