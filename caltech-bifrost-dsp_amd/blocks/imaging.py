"""Host side of UpchanImage: direction lists, steering delays and the normalisation of the direct Fourier sum, all float64.

A direction is (l, m, n): l east, m north, n = sqrt(1 - l^2 - m^2) up, the direction cosines of the stands' local east-north-up
frame.  The delay of stand s towards x, relative to the origin of the positions and with the zenith as phase centre, is
  tau_s(x) = (x_s l + y_s m + z_s (n - 1)) / c
and xengImage* (include/xeng.h) forms I_pq(x) = norm * sum_{s,t} conj(b_s) V[s p][t q] b_t with b_s = w_s exp(-2 pi i f tau_s(x)):
the w-term is in the delay, so a non-coplanar array needs no correction.  The list is free: an all-sky grid (pixel_grid), patches
around sources (patch), or both concatenated."""
import numpy as np

C_M_S = 299792458.0


def _lmn(l, m):
    r2 = l * l + m * m
    up = r2 < 1.0
    n = np.sqrt(np.where(up, 1.0 - r2, 0.0))
    return l, m, n, up


def pixel_grid(npix_side, fov_deg=180.0):
    """An orthographic (sine-projection) grid of npix_side x npix_side pixel centres across `fov_deg` around the zenith: returns
    l, m, n, mask as [npix_side][npix_side] arrays, l ascending along the last axis and m along the first,
    l = sin(fov / 2) * (2 i + 1 - npix_side) / npix_side.  mask is True for the pixels above the horizon (l^2 + m^2 < 1): only
    those go into a direction list, as np.stack([l[mask], m[mask], n[mask]], -1); n is 0 where the mask is False."""
    if int(npix_side) != npix_side or npix_side <= 0:
        raise ValueError("pixel_grid: npix_side %r is not a positive integer" % (npix_side,))
    if not 0.0 < fov_deg <= 180.0:
        raise ValueError("pixel_grid: a field of view of %r degrees, not in (0, 180]" % (fov_deg,))
    half = np.sin(np.radians(np.float64(fov_deg)) / 2.0)
    ax = half * (2.0 * np.arange(int(npix_side), dtype=np.float64) + 1.0 - npix_side) / npix_side
    l, m = np.meshgrid(ax, ax)
    return _lmn(l, m)


def patch(l0, m0, npix_side, cell):
    """The same around the direction (l0, m0): pixel centres l0 + cell * (i - (npix_side - 1) / 2), likewise in m."""
    if int(npix_side) != npix_side or npix_side <= 0:
        raise ValueError("patch: npix_side %r is not a positive integer" % (npix_side,))
    if not (np.isfinite(l0) and np.isfinite(m0) and np.isfinite(cell) and cell > 0):
        raise ValueError("patch: centre (%r, %r) and cell %r must be finite, the cell positive" % (l0, m0, cell))
    off = np.float64(cell) * (np.arange(int(npix_side), dtype=np.float64) - (npix_side - 1) / 2.0)
    l, m = np.meshgrid(np.float64(l0) + off, np.float64(m0) + off)
    return _lmn(l, m)


def direction_list(l, m, n, mask):
    """The pixels above the horizon of a grid or patch as a list, float64 [npix][3], in row-major order of the grid."""
    return np.ascontiguousarray(np.stack([l[mask], m[mask], n[mask]], axis=-1), np.float64)


def steering_delays(positions_enu_m, lmn):
    """tau[npix][nstand] in seconds, float64, C-contiguous: positions_enu_m [nstand][3] (east, north, up in metres), lmn [npix][3]."""
    pos = np.asarray(positions_enu_m, np.float64)
    d = np.asarray(lmn, np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or d.ndim != 2 or d.shape[1] != 3 or not pos.size or not d.size:
        raise ValueError("steering_delays: positions [nstand][3] and directions [npix][3], got %r and %r" % (pos.shape, d.shape))
    if not (np.all(np.isfinite(pos)) and np.all(np.isfinite(d))):
        raise ValueError("steering_delays: positions and directions must be finite")
    return np.ascontiguousarray((d[:, None, 0] * pos[None, :, 0] + d[:, None, 1] * pos[None, :, 1] + (d[:, None, 2] - 1.0) * pos[None, :, 2]) / C_M_S)


def image_norm(w, autos, nfavg):
    """1 / (nfavg * sum_{s,t} w_s w_t), the sum over s != t without autos: a unit point source at a pixel then reads 1 there."""
    w = np.asarray(w, np.float64).reshape(-1)
    if not w.size or not np.all(np.isfinite(w)) or w.min() < 0:
        raise ValueError("image_norm: the weights must be finite numbers >= 0")
    if int(nfavg) != nfavg or nfavg <= 0:
        raise ValueError("image_norm: nfavg %r is not a positive integer" % (nfavg,))
    total = w.sum() ** 2 if autos else w.sum() ** 2 - (w * w).sum()
    if not total > 0:
        raise ValueError("image_norm: the weights leave no pair of stands")
    return 1.0 / (nfavg * total)


def stokes_i(image):
    """I = XX + YY of an image f32 [...][4][npix] -> [...][npix]."""
    image = np.asarray(image)
    return image[..., 0, :] + image[..., 1, :]
