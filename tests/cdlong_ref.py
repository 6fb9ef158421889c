"""The contract of xengCdlong* (include/xeng.h, "Coherent dedispersion with long transforms") is xengCdedisp*'s, so its float64
restatement is tests/cdedisp_ref.py's filter_blocks.  Here: the four-step route of csrc/cdlong_kernels.h restated in complex64 (numpy's
single-precision FFTs over the columns, a complex64 step twiddle, FFTs over the rows, the table, and back), whose gap from float64 is
the second figure of the bar; the bar itself; and a fake backend that serves the calls BeamCoherentDedisperseLong makes."""
import numpy as np

from tests.cdedisp_ref import CdedispBackend, filter_blocks, float_gap, nblocks_after, row_error


def split(nfft):
    """(N1, N2) of csrc/cdlong_kernels.h: N1 = 2^min(LN div 2, 9), N2 = nfft / N1"""
    ln = int(nfft).bit_length() - 1
    assert nfft == 1 << ln
    ln1 = min(ln // 2, 9)
    return 1 << ln1, 1 << (ln - ln1)


def filter_blocks_four_step(rows, table, nfft, overlap):
    """filter_blocks in complex64 by the four-step route, n = n1 N2 + n2 and k = k1 + N1 k2: FFT over n1, times
    exp(-2 pi i n2 k1 / nfft) (float64, rounded once to complex64), FFT over n2, times the table, inverse FFT over k2, times the
    conjugate step twiddle, inverse FFT over k1.  [nblk][nchan][2 npair][L], complex64."""
    c64 = np.complex64
    nchan, nb, n = rows.shape
    n1, n2 = split(nfft)
    L = nfft - overlap
    nblk = nblocks_after(n, nfft, overlap)
    step = np.exp(-2j * np.pi * np.outer(np.arange(n1), np.arange(n2)) / nfft).astype(c64)         # [k1][n2]
    T = np.repeat(np.transpose(np.asarray(table), (1, 0, 2)), 2, axis=1).astype(c64)                 # [nchan][2 npair][k]
    T = np.ascontiguousarray(np.swapaxes(T.reshape(nchan, nb, n2, n1), -1, -2))                      # [..][k1][k2]
    out = np.empty((nblk, nchan, nb, L), c64)
    for j in range(nblk):
        x = np.ascontiguousarray(rows[:, :, j * L:j * L + nfft]).astype(c64).reshape(nchan, nb, n1, n2)
        with np.errstate(invalid='ignore', over='ignore'):
            a = (np.fft.fft(x, axis=-2) * step).astype(c64)                                          # [k1][n2]
            y = (np.fft.fft(a, axis=-1) * T).astype(c64)                                             # [k1][k2]
            b = (np.fft.ifft(y, axis=-1, norm="forward") * np.conj(step)).astype(c64)                # [k1][n2]
            z = np.fft.ifft(b, axis=-2, norm="forward")                                              # [n1][n2]
        assert z.dtype == c64
        out[j] = z.reshape(nchan, nb, nfft)[:, :, overlap // 2:overlap // 2 + L]
    return out


def four_step_gap(rows, table, nfft, overlap, ref=None):
    """The worst row_error of the complex64 four-step evaluation against the float64 restatement."""
    ref = filter_blocks(rows, table, nfft, overlap) if ref is None else ref
    return float(np.max(row_error(filter_blocks_four_step(rows, table, nfft, overlap), ref)))


def gaps(rows, table, nfft, overlap, ref=None):
    """(the direct complex64 gap, the four-step complex64 gap): the bar is five times the larger."""
    return float_gap(rows, table, nfft, overlap), four_step_gap(rows, table, nfft, overlap, ref)


class CdlongBackend(CdedispBackend):
    """CdedispBackend's state served under the cdlong_* names, the table pair by pair."""

    def cdlong_initialize(self, *args):
        return self.cdedisp_initialize(*args)

    def cdlong_set_chirp(self, pair, table):
        u = self.cd
        assert 0 <= pair < u['npair']
        self.table = self.table.copy()
        self.table[pair] = np.array(table, np.complex64).reshape(u['nchan'], u['nfft'])
        self.calls.append('chirp%d' % pair)
        return 0

    def cdlong_info(self):
        return self.cdedisp_info()

    def cdlong_run(self, in_arr, out_arr):
        return self.cdedisp_run(in_arr, out_arr)

    def cdlong_reset(self):
        self.cdedisp_reset()

    def cdlong_mark(self):
        return self.beam_mark()

    def cdlong_wait(self, ticket):
        self.beam_wait(ticket)

    def cdlong_sync(self):
        pass
