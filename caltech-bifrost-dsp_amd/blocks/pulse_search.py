"""Host side of the single-pulse search: the record plane xengPulseRun writes per call and its thresholding and grouping over DM.

A plane is [npair][ndm] records of four 32-bit words {f32 snr, i32 n_call, i32 iw, f32 B} (include/xeng.h, "Boxcar single-pulse
search of the dedispersed beams"): per series the best scored boxcar of the call, n_call = -1 where nothing was scored.  A
pulse that is bright at one DM trial is above the threshold at its neighbours too, so pulse_candidates cuts each pair's trials
above the threshold into runs of consecutive trial indices and reports one candidate per run.  Pure numpy; nothing here groups
in time, across spans or across pairs."""
import numpy as np

RECORD = np.dtype([('snr', '<f4'), ('n', '<i4'), ('iw', '<i4'), ('B', '<f4')])


def as_records(plane, npair=None, ndm=None):
    """A plane as a RECORD array [npair][ndm]: from a RECORD array, or from raw bytes / 32-bit words (then with npair, ndm, or
    with a shape [npair][ndm][4 words])."""
    a = np.asarray(plane)
    if a.dtype != RECORD:
        if npair is None:
            if a.ndim != 3 or a.shape[2] * a.dtype.itemsize != RECORD.itemsize:
                raise ValueError("pulse_search: a raw plane needs a shape [npair][ndm][16 bytes], or npair and ndm")
            npair, ndm = a.shape[:2]
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        if a.size != npair * ndm * RECORD.itemsize:
            raise ValueError("pulse_search: %d bytes are not %d x %d records" % (a.size, npair, ndm))
        a = a.view(RECORD).reshape(npair, ndm)
    if a.ndim != 2:
        raise ValueError("pulse_search: a plane is [npair][ndm] records, not %r" % (a.shape,))
    return a


def pulse_candidates(records, threshold, dms, widths):
    """records: one plane (as_records takes it); dms: the ndm trial DMs; widths: the boxcar widths in windows, widths[iw].
    Per pair, the trials with a scored record of snr >= threshold are cut into runs of consecutive trial indices; one candidate
    per run, its member with the largest snr (among equals the lowest trial):
      dict(pair, idm, dm, snr, window, iw, width, ntrial) -- window is n_call of the record, ntrial the length of the run.
    In order of pair, then trial."""
    rec = as_records(records)
    npair, ndm = rec.shape
    dms = np.asarray(dms, np.float64).reshape(-1)
    if dms.size != ndm:
        raise ValueError("pulse_search: %d DMs for a plane of %d trials" % (dms.size, ndm))
    with np.errstate(invalid='ignore'):
        above = (rec['n'] >= 0) & (rec['snr'].astype(np.float64) >= float(threshold))
    out = []
    for p in range(npair):
        idx = np.flatnonzero(above[p])
        if idx.size == 0:
            continue
        for run in np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1):
            d = int(run[np.argmax(rec['snr'][p, run])])             # (argmax: the first of equal maxima = the lowest trial)
            r = rec[p, d]
            out.append(dict(pair=p, idm=d, dm=float(dms[d]), snr=float(r['snr']), window=int(r['n']), iw=int(r['iw']),
                            width=int(widths[int(r['iw'])]), ntrial=int(run.size)))
    return out
