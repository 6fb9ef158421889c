"""Host side of UpchanFlag's mask: the two shapes in which the downstream blocks take flags, and counts.

The mask is u8 [nfine][2][nstand] (include/xeng.h, "Outlier flags from the fine-channel visibilities"): bit 0 cross-power outlier,
bit 1 auto outlier, bit 2 channel flagged, bit 3 non-finite statistic, bit 4 weight 0.  UpchanCalApply takes one factor per (fine
channel, polarisation, stand), 0 where it is left out (flag_factors); UpchanGainCal, UpchanImage and UpchanPeel take one weight per
stand, 0 where it is not read (stand_weights)."""
import numpy as np

BIT_CROSS, BIT_AUTO, BIT_CHAN, BIT_NONFINITE, BIT_WEIGHT = 1, 2, 4, 8, 16
BIT_NAMES = ('cross', 'auto', 'chan', 'nonfinite', 'weight')
MAX_NSTAND = 512        # include/xeng.h XENG_FLAG_MAX_NSTAND
MAX_NFINE = 8192        # include/xeng.h XENG_FLAG_MAX_NFINE
MAX_WCHAN = 64          # include/xeng.h XENG_FLAG_MAX_WCHAN
DEFAULT_CONTROL = (6.0, 6.0, 6.0, 0)    # include/xeng.h XENG_FLAG_DEFAULT_*


def _checked_mask(mask):
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.ndim != 3 or m.shape[1] != 2:
        raise ValueError("the mask must be uint8 [nfine][2][nstand], not %s %r" % (m.dtype, m.shape))
    return m


def _checked_bits(bits):
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 0 <= bits <= 0xff:
        raise ValueError("bits %r is not an integer in [0, 255]" % (bits,))
    return np.uint8(bits)


def checked_control(who, control, quiet=False):
    """(nsig_cross, nsig_auto, nsig_chan, wchan) as the library takes them: three finite numbers >= 0 and an integer in [0, MAX_WCHAN];
    else ValueError, or None if `quiet`."""
    try:
        a, b, c, wchan = control
        ok = not isinstance(wchan, bool) and isinstance(wchan, (int, np.integer)) and 0 <= wchan <= MAX_WCHAN
        for v in (a, b, c):
            ok = ok and not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and bool(np.isfinite(v)) and v >= 0
    except (TypeError, ValueError):
        ok = False
    if ok:
        return float(a), float(b), float(c), int(wchan)
    if quiet:
        return None
    raise ValueError("%s: the control %r is not three finite numbers >= 0 and a window of 0 to %d channels" % (who, control, MAX_WCHAN))


def flag_factors(h, mask, bits=0x0f):
    """h [nfine][2][nstand] with 0 + 0i where the mask has one of `bits`: what UpchanCalApply.set_factors takes (complex64).  The
    default leaves bit 4 out: a stand of weight 0 was not judged."""
    m = _checked_mask(mask)
    h = np.asarray(h)
    if h.shape != m.shape:
        raise ValueError("factors %r for a mask %r" % (h.shape, m.shape))
    return np.ascontiguousarray(np.where(m & _checked_bits(bits), 0, h), np.complex64)


def stand_weights(mask, w, max_fraction=0.5, bits=0x0b):
    """w [nstand] with 0 where more than `max_fraction` of the stand's 2 nfine (channel, polarisation) cells have one of `bits`: what
    set_weights of UpchanGainCal, UpchanImage and UpchanPeel takes (float32).  The default leaves the channel bit out: a flagged
    channel says nothing about a stand."""
    m = _checked_mask(mask)
    w = np.asarray(w, np.float32)
    if w.shape != (m.shape[2],):
        raise ValueError("weights %r for a mask of %d stands" % (w.shape, m.shape[2]))
    if isinstance(max_fraction, bool) or not 0 <= max_fraction <= 1:
        raise ValueError("max_fraction %r is not in [0, 1]" % (max_fraction,))
    nflag = ((m & _checked_bits(bits)) != 0).sum(axis=(0, 1))
    return np.ascontiguousarray(np.where(nflag > max_fraction * (2 * m.shape[0]), 0, w), np.float32)


def flag_visibilities(V, mask, bits=0x0f):
    """A copy of V [nfine][nstand][2][nstand][2] with the rows and columns of every flagged (channel, polarisation, stand) zeroed"""
    m = _checked_mask(mask)
    V = np.array(V)
    if V.ndim != 5 or V.shape != (m.shape[0], m.shape[2], 2, m.shape[2], 2):
        raise ValueError("visibilities %r for a mask %r" % (V.shape, m.shape))
    bad = ((m & _checked_bits(bits)) != 0).transpose(0, 2, 1)          # [nfine][nstand][2]
    V[bad] = 0
    V.transpose(0, 3, 4, 1, 2)[bad] = 0
    return V


def flag_summary(mask):
    """Counts of the mask's cells: {'ncell', 'nflagged' (any bit), 'fraction', 'bits': {name: count}, 'per_channel' [nfine] and
    'per_stand' [nstand] (cells with any of the bits 0 to 3)}"""
    m = _checked_mask(mask)
    judged = (m & np.uint8(0x0f)) != 0
    return {'ncell': int(m.size), 'nflagged': int((m != 0).sum()), 'fraction': float((m != 0).mean()) if m.size else 0.0,
            'bits': {name: int(((m >> k) & 1).sum()) for k, name in enumerate(BIT_NAMES)},
            'per_channel': judged.sum(axis=(1, 2)), 'per_stand': judged.sum(axis=(0, 1))}
