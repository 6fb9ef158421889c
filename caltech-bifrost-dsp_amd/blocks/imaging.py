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


# ---- what the readers of UpchanCorr's ring (UpchanImage, UpchanGainCal, UpchanCalApply) and of UpchanImage's (UpchanClean) share
def check_fine_axis(who, ihdr):
    """The fine-channel frequencies (fine_sfreq, fine_bw_hz) and the integration length of a header; returns acc_len."""
    for k in ('fine_sfreq', 'fine_bw_hz'):
        v = ihdr.get(k)
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not np.isfinite(v) or (k == 'fine_bw_hz' and not v > 0):
            raise ValueError("%s: the header's '%s' is %r" % (who, k, v))
    acc_len = ihdr.get('acc_len', 1)
    if not isinstance(acc_len, int) or isinstance(acc_len, bool) or acc_len <= 0:
        raise ValueError("%s: the header's 'acc_len' is %r" % (who, acc_len))
    return acc_len


def check_visibility_header(who, ihdr, nstand, reject=()):
    """The header of UpchanCorr's dual-polarisation cf32 visibilities of `nstand` stands, with none of the keys in `reject` (what
    a block that has consumed visibilities adds); returns (nfine, acc_len)."""
    if ihdr.get('npol') != 2:
        raise ValueError("%s: npol %r in the header: dual-polarisation visibilities only" % (who, ihdr.get('npol')))
    if ihdr.get('nstand') != nstand:
        raise ValueError("%s: %r stands in the header, positions for %d" % (who, ihdr.get('nstand'), nstand))
    if ihdr.get('nbit') != 32 or not ihdr.get('complex'):
        raise ValueError("%s: the input is not cf32 visibilities (nbit %r, complex %r)" % (who, ihdr.get('nbit'), ihdr.get('complex')))
    if any(k in ihdr for k in reject):
        raise ValueError("%s: the input carries %s: it is an image or a gain solution, not visibilities" % (who, " or ".join("'%s'" % k for k in reject)))
    nfine = ihdr.get('nfine')
    if not isinstance(nfine, int) or isinstance(nfine, bool) or nfine <= 0:
        raise ValueError("%s: the header's 'nfine' is %r: not UpchanCorr's visibilities" % (who, nfine))
    return nfine, check_fine_axis(who, ihdr)


def fine_frequencies(ihdr, nfine):
    """The fine channels' centre frequencies of a sequence, float64 [nfine] Hz."""
    return np.ascontiguousarray(ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * np.arange(nfine, dtype=np.float64))


def checked_weights(who, w, nstand, pair=None, quiet=False):
    """Per-stand weights as the library takes them, f32 [nstand], finite and >= 0 and, with pair = (autos, nfavg), leaving a pair
    of stands for image_norm; else ValueError, or None if `quiet`."""
    try:
        a = np.ascontiguousarray(w, np.float32).reshape(-1)
        ok = a.size == nstand and bool(np.all(np.isfinite(a))) and bool(a.min() >= 0)
        if ok and pair is not None:
            image_norm(a, *pair)
    except (TypeError, ValueError):
        a, ok = None, False
    if ok:
        return a
    if quiet:
        return None
    raise ValueError("%s: the weights must be %d finite numbers >= 0%s" % (who, nstand, " that leave a pair of stands" if pair is not None else ""))


# ---- Hogbom CLEAN of the dirty images (UpchanClean; include/xeng.h "Hogbom CLEAN of the dirty images")
CLEAN_COMPONENT = np.dtype([('pixel', '<i4'), ('I', '<f4'), ('C', '<f4', (4,)), ('pad', '<u4', (2,))])      # 32 bytes: one record
CLEAN_STATS = np.dtype([('ncomp', '<i4'), ('reason', '<i4'), ('peak', '<f4'), ('pad', '<u4')])              # 16 bytes per channel group


def psf(freq, tau, w, autos, nfavg, x0):
    """The exact point-spread function of the direct Fourier sum: the response of UpchanImage, at every pixel of the list and in
    every channel group, to a unit point source at list pixel x0; float64 [nfine / nfavg][npix], the same for all four words.
      PSF_g(x, x0) = norm * sum_{c in g} ( |sum_s w_s exp(2 pi i (fr_c(x,s) - fr_c(x0,s)))|^2 - D ),  D = sum w_s^2 without autos, else 0
    with fr_c(x,s) the product freq[c] tau[x][s] minus its nearest integer; PSF_g(x0, x0) = 1."""
    freq, tau = np.asarray(freq, np.float64).reshape(-1), np.asarray(tau, np.float64)
    w = np.asarray(w, np.float64).reshape(-1)
    if tau.ndim != 2 or tau.shape[1] != w.size or not 0 <= int(x0) < tau.shape[0]:
        raise ValueError("psf: delays [npix][nstand] %r, %d weights, pixel %r" % (tau.shape, w.size, x0))
    norm = image_norm(w, autos, nfavg)
    if freq.size % int(nfavg):
        raise ValueError("psf: nfavg %d does not divide %d channels" % (nfavg, freq.size))
    turns = freq[:, None, None] * tau[None]
    fr = turns - np.rint(turns)
    S = (w * np.exp(2j * np.pi * (fr - fr[:, int(x0):int(x0) + 1, :]))).sum(axis=2)
    p = S.real ** 2 + S.imag ** 2 - (0.0 if autos else (w * w).sum())
    return norm * p.reshape(freq.size // int(nfavg), int(nfavg), -1).sum(axis=1)


def clean_layout(ngroup, niter, npix):
    """(comp_offset, stats_offset, span_bytes) of UpchanClean's span"""
    comp = 16 * int(ngroup) * int(npix)
    stats = comp + 32 * int(ngroup) * int(niter)
    return comp, stats, stats + 16 * int(ngroup)


def clean_components(span, ngroup, niter, npix):
    """One span of UpchanClean (any buffer of its bytes) taken apart, without a copy: (components CLEAN_COMPONENT [ngroup][niter],
    stats CLEAN_STATS [ngroup], residual f32 [ngroup][4][npix]).  stats['ncomp'][g] records of group g are filled; the rest hold
    pixel -1."""
    raw = np.asarray(span).reshape(-1).view(np.uint8)
    comp, stats, total = clean_layout(ngroup, niter, npix)
    if raw.size < total:
        raise ValueError("clean_components: %d bytes, a span of %d groups, %d iterations and %d pixels has %d" % (raw.size, ngroup, niter, npix, total))
    return (raw[comp:stats].view(CLEAN_COMPONENT).reshape(ngroup, niter), raw[stats:total].view(CLEAN_STATS).reshape(ngroup),
            raw[:comp].view(np.float32).reshape(ngroup, 4, npix))


def restore(residual, components, lmn, fwhm_rad):
    """The restored image, float64 [ngroup][4][npix]: the residual plus, per component, its four words times a Gaussian of full width
    at half maximum `fwhm_rad` in the angular distance between the component's direction and each pixel's (from the direction
    cosines: the angle between the two unit vectors), on the free pixel list."""
    d = np.asarray(lmn, np.float64)
    out = np.array(residual, np.float64)
    if out.ndim != 3 or out.shape[1] != 4 or d.shape != (out.shape[2], 3) or len(components) != out.shape[0]:
        raise ValueError("restore: residual [ngroup][4][npix] %r, components for %d groups, directions %r" % (out.shape, len(components), d.shape))
    if not (np.isfinite(fwhm_rad) and fwhm_rad > 0):
        raise ValueError("restore: a beam width of %r radians" % (fwhm_rad,))
    sigma = fwhm_rad / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    for g in range(out.shape[0]):
        for rec in components[g]:
            if rec['pixel'] < 0:
                continue
            x0 = d[rec['pixel']]
            # the angle from the chord: well conditioned for small separations, where arccos of the dot product is not
            ang = 2.0 * np.arcsin(np.minimum(np.linalg.norm(d - x0, axis=1) / 2.0, 1.0))
            out[g] += rec['C'].astype(np.float64)[:, None] * np.exp(-0.5 * (ang / sigma) ** 2)[None]
    return out


def components_to_model(components, lmn, nfavg, nsrc_max=32):
    """The sky model of a span's components, as UpchanGainCal and UpchanCalApply take it: (src_lmn float64 [nsrc][3], flux float32
    [nfine][nsrc]).  Components at the same pixel are merged: the flux of a pixel in a channel group is the sum of its (C_XX + C_YY) /
    2 there -- the unit point source of both polarisations images to XX = YY = 1.  The nsrc_max brightest pixels are kept, ranked by
    the sum over the groups of |flux| (ties: the lower pixel); a flux that comes out negative is set to 0 (the model's fluxes are >=
    0).  Each group's flux is repeated over its nfavg channels."""
    d = np.asarray(lmn, np.float64)
    ngroup = len(components)
    if int(nfavg) != nfavg or nfavg <= 0 or int(nsrc_max) != nsrc_max or nsrc_max <= 0:
        raise ValueError("components_to_model: nfavg %r and nsrc_max %r must be positive integers" % (nfavg, nsrc_max))
    per = {}
    for g in range(ngroup):
        for rec in components[g]:
            if rec['pixel'] >= 0:
                per.setdefault(int(rec['pixel']), np.zeros(ngroup))[g] += (float(rec['C'][0]) + float(rec['C'][1])) / 2.0
    pix = sorted(per, key=lambda x: (-np.abs(per[x]).sum(), x))[:int(nsrc_max)]
    flux = np.zeros((ngroup, len(pix)))
    for k, x in enumerate(pix):
        flux[:, k] = np.maximum(per[x], 0.0)
    return np.ascontiguousarray(d[pix].reshape(len(pix), 3)), np.ascontiguousarray(np.repeat(flux, int(nfavg), axis=0), np.float32)


# ---- component lists as visibilities (UpchanPredict; include/xeng.h "Component lists subtracted from the visibilities")
def component_visibilities(freq, tau, components, nfavg, cross=True):
    """The visibility model of component records, float64 on the host: complex128 [nfine][nstand][2][nstand][2], the whole Hermitian
    matrix.  components: CLEAN_COMPONENT [nfine / nfavg][n] (clean_components(span, ...)[0], or a catalogue in that layout), `pixel`
    an index into tau [ndir][nstand], -1 an empty record; each group's list serves its nfavg channels.  With a_ks = exp(-2 pi i
    frac(freq[c] tau[pixel_k][s])):
      M[c][s p][t p] = sum_k C_k^pp a_ks conj(a_kt)  (C^00 = C_XX, C^11 = C_YY), and with `cross`
      M[c][s 0][t 1] = sum_k (C_Re + i C_Im)_k a_ks conj(a_kt),  M[c][s 1][t 0] = sum_k (C_Re - i C_Im)_k a_ks conj(a_kt)
    the convention under which UpchanImage reads one component at its pixel as [C_XX, C_YY, C_Re, C_Im]: UpchanImage of V - M is
    UpchanClean's residual."""
    freq, tau = np.asarray(freq, np.float64).reshape(-1), np.asarray(tau, np.float64)
    comps = np.asarray(components)
    if int(nfavg) != nfavg or nfavg <= 0 or freq.size % int(nfavg):
        raise ValueError("component_visibilities: nfavg %r does not divide %d channels" % (nfavg, freq.size))
    nfavg = int(nfavg)
    if tau.ndim != 2 or comps.dtype != CLEAN_COMPONENT or comps.ndim != 2 or comps.shape[0] != freq.size // nfavg:
        raise ValueError("component_visibilities: delays [ndir][nstand] %r and CLEAN_COMPONENT records [%d][n], got %r %r"
                         % (tau.shape, freq.size // nfavg, comps.dtype, comps.shape))
    ndir, nstand = tau.shape
    M = np.zeros((freq.size, nstand, 2, nstand, 2), np.complex128)
    for g in range(comps.shape[0]):
        rec = comps[g][comps[g]['pixel'] != -1]
        if not rec.size:
            continue
        if rec['pixel'].min() < 0 or rec['pixel'].max() >= ndir:
            raise ValueError("component_visibilities: a pixel of group %d is outside [-1, %d)" % (g, ndir))
        C = rec['C'].astype(np.float64)
        if not np.all(np.isfinite(C if cross else C[:, :2])):
            raise ValueError("component_visibilities: a component of group %d is not finite" % g)
        ch = slice(g * nfavg, (g + 1) * nfavg)
        turns = freq[ch, None, None] * tau[rec['pixel']][None]
        a = np.exp(-2j * np.pi * (turns - np.rint(turns)))                        # [nfavg][k][nstand]
        M[ch, :, 0, :, 0] = np.einsum('k,cks,ckt->cst', C[:, 0], a, np.conj(a))
        M[ch, :, 1, :, 1] = np.einsum('k,cks,ckt->cst', C[:, 1], a, np.conj(a))
        if cross:
            M[ch, :, 0, :, 1] = np.einsum('k,cks,ckt->cst', C[:, 2] + 1j * C[:, 3], a, np.conj(a))
            M[ch, :, 1, :, 0] = np.einsum('k,cks,ckt->cst', C[:, 2] - 1j * C[:, 3], a, np.conj(a))
    return M
