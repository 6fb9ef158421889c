"""Host side of the dedispersed transient search of the images: the record plane xengImsearchRun writes per integration, the
frequency axis and the delay table the search runs on, and the thresholding and clustering of a plane over the sky.

A plane is [npix] records of 8 bytes {f32 snr, i16 idm, i16 iw} (include/xeng.h, "Dedispersed transient search of the images"): per
pixel the best scored (trial, boxcar) of the integration, idm = iw = -1 where nothing was scored.  A transient that is bright in
one pixel is above the threshold in its neighbours too (the point-spread function), so image_candidates takes the pixels above
the threshold in descending score and lets each join the brightest accepted candidate within `radius`.  Pure numpy; nothing here
groups in time across planes."""
import numpy as np

from .dedisp import dm_delays

IMSEARCH_RECORD = np.dtype([('snr', '<f4'), ('idm', '<i2'), ('iw', '<i2')])


def as_records(plane, npix=None):
    """A plane as an IMSEARCH_RECORD array [npix]: from such an array, or from raw bytes / words of npix * 8 bytes."""
    a = np.asarray(plane)
    if a.dtype != IMSEARCH_RECORD:
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size % IMSEARCH_RECORD.itemsize or (npix is not None and a.size != npix * IMSEARCH_RECORD.itemsize):
            raise ValueError("image_search: %d bytes are not %s records of 8 bytes" % (a.size, "whole" if npix is None else npix))
        a = a.view(IMSEARCH_RECORD)
    if a.ndim != 1 or (npix is not None and a.size != npix):
        raise ValueError("image_search: a plane is [npix] records, not %r" % (a.shape,))
    return a


def group_frequencies(ihdr, ngroup):
    """The channel groups' centre frequencies of a sequence of images, float64 [ngroup] Hz, from the header UpchanImage writes."""
    for k in ('image_sfreq', 'image_bw_hz'):
        v = ihdr.get(k)
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not np.isfinite(v) or (k == 'image_bw_hz' and not v > 0):
            raise ValueError("image_search: the header's '%s' is %r" % (k, v))
    return np.ascontiguousarray(ihdr['image_sfreq'] + ihdr['image_bw_hz'] * np.arange(ngroup, dtype=np.float64))


def image_dm_delays(freqs, dms, tint):
    """int32 [ndm][ngroup]: the delay of each channel group behind the highest one in integrations of tint seconds; dedisp.dm_delays."""
    return np.ascontiguousarray(dm_delays(freqs, dms, tint))


def kappa(weights):
    """(float32) 1 / sqrt(sum w^2): what turns the weighted sum of unit-variance series into one of unit variance."""
    w = np.asarray(weights, np.float64).reshape(-1)
    s = float((w * w).sum())
    if not (np.isfinite(s) and s > 0):
        raise ValueError("image_search: the weights have no finite positive norm")
    return np.float32(1.0 / np.sqrt(s))


class Candidates(list):
    """The candidates of a plane; `saturated`: more pixels passed the threshold than were looked at."""
    saturated = False


def image_candidates(plane, threshold, lmn, radius, dms, widths, max_above=4096):
    """plane: one plane (as_records takes it); lmn: float [npix][3], the pixels' unit vectors; radius in radians; dms: the ndm trial
    DMs; widths: the boxcar widths in integrations, widths[iw].  The pixels with a scored record of snr >= threshold are taken in
    descending snr, among equals by pixel index.  A pixel within `radius` of an accepted candidate (chords of the unit vectors are
    compared: |a - b| <= 2 sin(radius / 2)) joins the first, which is the brightest, such candidate; else it is accepted as a
    candidate of its own:
      dict(pixel, lmn, snr, idm, dm, iw, width, window, members) -- window is 0 (the plane is one integration), members the pixels
      of the cluster, the candidate's first.
    If more than max_above pixels pass, the max_above brightest are looked at and the list's `saturated` is True."""
    rec = as_records(plane)
    lmn = np.asarray(lmn, np.float64)
    if lmn.shape != (rec.size, 3):
        raise ValueError("image_search: lmn of shape %r for a plane of %d pixels" % (lmn.shape, rec.size))
    dms = np.asarray(dms, np.float64).reshape(-1)
    with np.errstate(invalid='ignore'):
        idx = np.flatnonzero((rec['idm'] >= 0) & (rec['snr'].astype(np.float64) >= float(threshold)))
    out = Candidates()
    if idx.size == 0:
        return out
    if (rec['idm'][idx] >= dms.size).any() or (rec['iw'][idx] >= len(widths)).any():
        raise ValueError("image_search: a record names a trial or a width beyond the %d DMs and %d widths" % (dms.size, len(widths)))
    idx = idx[np.argsort(-rec['snr'][idx].astype(np.float64), kind='stable')]      # (stable: equal scores stay in pixel order)
    if idx.size > max_above:
        idx, out.saturated = idx[:max_above], True
    chord2 = (2.0 * np.sin(min(float(radius), np.pi) / 2.0)) ** 2
    centres = np.empty((0, 3))
    for p in idx:
        if centres.shape[0]:
            near = np.flatnonzero(((centres - lmn[p]) ** 2).sum(axis=1) <= chord2)
            if near.size:
                out[int(near[0])]['members'].append(int(p))
                continue
        r = rec[p]
        out.append(dict(pixel=int(p), lmn=tuple(float(v) for v in lmn[p]), snr=float(r['snr']), idm=int(r['idm']), dm=float(dms[r['idm']]),
                        iw=int(r['iw']), width=int(widths[int(r['iw'])]), window=0, members=[int(p)]))
        centres = np.vstack([centres, lmn[p]])
    return out
