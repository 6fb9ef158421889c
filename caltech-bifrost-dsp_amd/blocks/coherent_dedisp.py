"""Host side of BeamCoherentDedisperse: the chirp table of a dispersion measure, the sweep across a coarse channel and the choice
of the transform length and the overlap.  The library itself (xengCdedisp*, include/xeng.h) filters by whatever table it is given
and knows nothing of the dispersion constant.

A signal at the offset nu from a channel's centre f_c arrives KDM * DM * ((f_c + nu)**-2 - f_c**-2) seconds behind the centre
(dedisp.py): the interstellar medium multiplies the channel's spectrum by exp(+2 pi i KDM DM nu^2 / (f_c^2 (f_c + nu))) once the
constant and the term linear in nu -- the delay of the centre itself -- are dropped (frequencies in MHz, and a factor 10^6 for
seconds * MHz).  chirp_table is its conjugate: it aligns every frequency of a coarse channel to the channel's centre and leaves the
delays between the channels to the incoherent stages behind it.

Sign convention: the project's forward DFT exp(-2 pi i k n / N) puts a higher sky frequency at a higher k (fine channels ascend,
DESIGN.md 4.11), so the table's group delay -(1 / 2 pi) dphi/dnu is -KDM DM ((f_c + nu)**-2 - f_c**-2): what arrived late is moved
forward."""
import numpy as np

from .dedisp import KDM

NFFT_MIN, NFFT_MAX = 1 << 8, 1 << 13
NFFT_LONG_MIN, NFFT_LONG_MAX = 1 << 14, 1 << 20     # BeamCoherentDedisperseLong (cdedisp_plan_long)
GUARD_FACTOR = 1.5      # overlap / largest sweep (cdedisp_plan)


def _channels(who, freqs_hz, chan_bw_hz):
    f = np.asarray(freqs_hz, np.float64).reshape(-1)
    if f.size == 0 or not (np.all(np.isfinite(f)) and np.isfinite(chan_bw_hz) and chan_bw_hz > 0 and np.all(f - chan_bw_hz / 2 > 0)):
        raise ValueError("%s: channel centres must be finite and lie more than half a channel width (%r Hz) above 0" % (who, chan_bw_hz))
    return f


def chirp_table(freqs_hz, chan_bw_hz, dms, nfft):
    """complex64 [npair][nchan][nfft] for xengCdedispSetChirp, in natural DFT order (bin k is the offset nu = k * bw / nfft for
    k < nfft/2 and (k - nfft) * bw / nfft from there on), computed in float64 and rounded once:
        T = exp(-2 pi i * 1e6 * KDM * DM * nu**2 / (f_c**2 * (f_c + nu))) / nfft        (nu, f_c in MHz)
    freqs_hz are the centres of the coarse channels, chan_bw_hz their width (the sample rate of a channel), dms one DM per pair.
    DM 0 gives 1 / nfft exactly."""
    f = _channels("chirp_table", freqs_hz, chan_bw_hz) * 1e-6
    dm = np.asarray(dms, np.float64).reshape(-1)
    if dm.size == 0 or not np.all(np.isfinite(dm)):
        raise ValueError("chirp_table: the DMs must be finite numbers, one per pair")
    if not isinstance(nfft, (int, np.integer)) or nfft < 2 or nfft & (nfft - 1):
        raise ValueError("chirp_table: nfft %r is not a power of two" % (nfft,))
    nu = np.fft.fftfreq(int(nfft)) * (chan_bw_hz * 1e-6)
    turns = 1e6 * KDM * dm[:, None, None] * nu[None, None, :] ** 2 / (f[None, :, None] ** 2 * (f[None, :, None] + nu[None, None, :]))
    return (np.exp(-2j * np.pi * turns) / int(nfft)).astype(np.complex64)


def smear_samples(freqs_hz, chan_bw_hz, dm):
    """float64 [nchan]: KDM * |DM| * (f_lo**-2 - f_hi**-2) * chan_bw, the sweep of a pulse across each coarse channel in samples of
    that channel (f_lo, f_hi its edges in MHz)."""
    f = _channels("smear_samples", freqs_hz, chan_bw_hz)
    if not np.isfinite(dm):
        raise ValueError("smear_samples: DM %r is not finite" % (dm,))
    lo, hi = (f - chan_bw_hz / 2) * 1e-6, (f + chan_bw_hz / 2) * 1e-6
    return KDM * abs(float(dm)) * (lo ** -2 - hi ** -2) * float(chan_bw_hz)


def cdedisp_plan(freqs_hz, chan_bw_hz, dm_max, multiple_of=1):
    """(nfft, overlap) for a band and its largest DM: the smallest power of two from 2^8 to 2^13 that admits an even overlap M of at
    least GUARD_FACTOR = 1.5 times the largest sweep (smear_samples at dm_max) with M <= nfft/2 and a step L = nfft - M that is a
    multiple of `multiple_of` (the nupchan of an UpchanSumBeams behind the block); of those M the smallest.  ValueError when there
    is none: the sweep needs a transform beyond 2^13 points.

    Why 1.5: the chirp's response is as long as the sweep, but its spectrum is cut off at the channel's edges, which rings beyond
    that.  With half of M discarded on either side, 1.5 sweeps bring an impulse dispersed in float64 back with 0.9999 of its energy
    in one sample wherever it falls in a block (tests/test_cdedisp_cpu.py states the figures)."""
    return _plan("cdedisp_plan", NFFT_MIN, NFFT_MAX, freqs_hz, chan_bw_hz, dm_max, multiple_of)


def cdedisp_plan_long(freqs_hz, chan_bw_hz, dm_max, multiple_of=1):
    """(nfft, overlap) for BeamCoherentDedisperseLong: cdedisp_plan's rule over the powers of two from 2^14 to 2^20 (xengCdlong*),
    for the sweeps that cdedisp_plan refuses -- at 23.9 kHz channels and DM 10, 2^14 at 25 MHz, 2^15 at 20 MHz and 2^16 at 15 MHz.
    A sweep that would fit a shorter transform still gets 2^14 here.  ValueError when there is none."""
    return _plan("cdedisp_plan_long", NFFT_LONG_MIN, NFFT_LONG_MAX, freqs_hz, chan_bw_hz, dm_max, multiple_of)


def _plan(who, nfft_min, nfft_max, freqs_hz, chan_bw_hz, dm_max, multiple_of):
    if not isinstance(multiple_of, (int, np.integer)) or multiple_of < 1:
        raise ValueError("%s: multiple_of %r is not a positive integer" % (who, multiple_of))
    need = GUARD_FACTOR * float(np.max(smear_samples(freqs_hz, chan_bw_hz, dm_max)))
    nfft = nfft_min
    while nfft <= nfft_max:
        m = int(np.ceil(need))
        m += m & 1
        while m <= nfft // 2:
            if (nfft - m) % multiple_of == 0:
                return nfft, m
            m += 2
        nfft *= 2
    raise ValueError("%s: a sweep of %.0f samples needs an overlap of %.0f, more than half of the longest transform (%d points)%s"
                     % (who, need / GUARD_FACTOR, need, nfft_max, "" if multiple_of == 1 else ", with a step that is a multiple of %d" % multiple_of))
