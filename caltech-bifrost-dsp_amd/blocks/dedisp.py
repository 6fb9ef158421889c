"""The delay table of an incoherent dedisperser (host side of BeamDedisperse; the library itself takes integer delays and knows
nothing of the dispersion constant).

The cold-plasma delay of a pulse at frequency f against a reference f_ref is KDM * DM * (f**-2 - f_ref**-2), with f in MHz, DM in
pc cm^-3 and KDM = 4.148808e3 s MHz^2 pc^-1 cm^3: lower frequencies arrive later."""
import numpy as np

KDM = 4.148808e3        # s MHz^2 pc^-1 cm^3


def dm_delays(freqs_hz, dms, tsamp_s, f_ref_hz=None):
    """int32 [ndm][nfine]: rint(KDM * DM * (f**-2 - f_ref**-2) / tsamp) in float64, the delay of channel f behind f_ref in
    samples of tsamp_s seconds.  f_ref defaults to the highest channel, which then has delay 0 at every DM.  A negative delay
    (a channel above f_ref, a negative DM) is refused: the dedisperser's history only reaches back."""
    f = np.asarray(freqs_hz, np.float64).reshape(-1) * 1e-6
    dm = np.asarray(dms, np.float64).reshape(-1)
    if f.size == 0 or dm.size == 0:
        raise ValueError("dm_delays: no channels or no DM trials")
    if not (np.all(np.isfinite(f)) and np.all(f > 0) and np.all(np.isfinite(dm))):
        raise ValueError("dm_delays: frequencies must be positive and finite, DMs finite")
    if not (np.isfinite(tsamp_s) and tsamp_s > 0):
        raise ValueError("dm_delays: sampling time %r is not positive" % (tsamp_s,))
    f_ref = f.max() if f_ref_hz is None else float(f_ref_hz) * 1e-6
    if not (np.isfinite(f_ref) and f_ref > 0):
        raise ValueError("dm_delays: reference frequency %r is not positive" % (f_ref_hz,))
    s = np.rint(KDM * dm[:, None] * (f[None, :] ** -2 - f_ref ** -2) / float(tsamp_s))
    if s.min() < 0:
        raise ValueError("dm_delays: negative delay (%d samples): a channel above the reference frequency or a negative DM" % s.min())
    if s.max() > np.iinfo(np.int32).max:
        raise ValueError("dm_delays: a delay of %.3g samples does not fit an int32" % s.max())
    return s.astype(np.int32)
