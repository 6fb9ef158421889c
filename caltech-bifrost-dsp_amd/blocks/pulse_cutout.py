"""Host side of the single-pulse cut-outs (BeamPulseCutout; xengCutout*, the definition is in include/xeng.h): the fine DM grid, the
sizes of a cut-out, requests from the candidates of BeamPulseSearch, the serving rule as the block mirrors it, the records of a
served span, and the float64 statement of what a cut-out holds.  The library knows integers only; the dispersion constant, time
and DM live here.  Pure numpy."""
import numpy as np

from .dedisp import dm_delays

CUTOUT_RECORD = np.dtype([('id', '<i4'), ('status', '<i4'), ('S', '<f4'), ('S0', '<f4'), ('i', '<i2'), ('iw', '<i2'), ('j', '<i2'), ('pad', '<i2'),
                          ('M', '<f4'), ('A', '<f4')])
CUTOUT_REQUEST = np.dtype([('id', '<i4'), ('pair', '<i4'), ('n_c', '<i8'), ('ic', '<i4'), ('dstep', '<i4')])
MAX_PENDING = 1024      # include/xeng.h XENG_CUTOUT_MAX_PENDING


def cutout_k_mad(k=1.0):
    """k_mad as the library takes it: 1.4826 MAD is the sigma of a normal distribution; float32."""
    return float(np.float32(1.4826 * k))


def cutout_fine_dms(dms, nsplit):
    """The search grid with every interval cut into nsplit: (ndm - 1) nsplit + 1 trials; search trial k is fine trial k nsplit."""
    dms = np.asarray(dms, np.float64).reshape(-1)
    if dms.size < 2 or not np.all(np.isfinite(dms)) or np.any(np.diff(dms) <= 0) or dms[0] < 0:
        raise ValueError("cutout_fine_dms: the search grid must be two or more increasing, finite, non-negative DMs")
    if not isinstance(nsplit, (int, np.integer)) or nsplit < 1:
        raise ValueError("cutout_fine_dms: nsplit %r is not a positive integer" % (nsplit,))
    k = np.arange((dms.size - 1) * nsplit + 1)
    lo = np.minimum(k // nsplit, dms.size - 2)
    return dms[lo] + (dms[lo + 1] - dms[lo]) * (k - lo * nsplit) / float(nsplit)


def cutout_plan(freqs_hz, fine_dms, tsamp_s, widest, dm_span, nt=256, late=0):
    """Sizes for pulses of up to `widest` windows and a plane `dm_span` (pc cm^-3) wide: dict(nt, tscr, ntu, ndmc, dstep, nhist, S).
    The cut-out is ntu = nt tscr windows long: eight times the widest pulse (the row's median and MAD are then the off-pulse
    level's) and four times the sweep that half the DM span adds across the band (the bow tie stays inside the plane), with tscr
    the smallest power of two up to 64 that reaches that.  ndmc is the odd number of fine trials, dstep apart, that cover
    dm_span (at most 255).  nhist = ntu + S + late: S the largest delay of the fine grid, late the windows by which a request
    may come after the last window it needs has passed (the search's own latency and the spans in flight)."""
    fine_dms = np.asarray(fine_dms, np.float64).reshape(-1)
    if nt % 2 or not 16 <= nt <= 1024 or widest < 1 or not dm_span > 0 or late < 0:
        raise ValueError("cutout_plan: nt %r not even in 16..1024, widest %r < 1, dm_span %r or late %r" % (nt, widest, dm_span, late))
    S = int(dm_delays(freqs_hz, [fine_dms.max()], tsamp_s).max())
    sweep = int(dm_delays(freqs_hz, [0.5 * dm_span], tsamp_s).max())
    need = max(8 * int(widest), 4 * sweep, nt)
    tscr = 1
    while nt * tscr < need and tscr < 64:
        tscr *= 2
    step = float(np.median(np.diff(fine_dms))) if fine_dms.size > 1 else dm_span
    rows = max(1, int(np.ceil(dm_span / step)))
    dstep = max(1, -(-rows // 254))
    ndmc = min(255, 2 * (-(-rows // (2 * dstep))) + 1)
    return dict(nt=nt, tscr=tscr, ntu=nt * tscr, ndmc=ndmc, dstep=dstep, nhist=nt * tscr + S + int(late), S=S)


def cutout_requests(cands, span_seq, dedisp_latency, acc_len, first_id=0):
    """From pulse_candidates dicts {pair, dm, window, width, ..} of the span whose first window has the beamformer-clock sample
    span_seq: dict(id, pair, dm, seq), seq the sample of the pulse at the top of the band -- the boxcar's last window less the
    dedisperser's latency, moved back by half the boxcar."""
    out = []
    for k, c in enumerate(cands):
        seq = int(span_seq) + (int(c['window']) - int(dedisp_latency)) * int(acc_len) - ((int(c['width']) - 1) * int(acc_len)) // 2
        out.append(dict(id=first_id + k, pair=int(c['pair']), dm=float(c['dm']), seq=seq))
    return out


class CutoutQueue(object):
    """The serving rule of include/xeng.h from the host's counts alone, as the library applies it: the block asks it whether a call
    will serve (only then does it reserve an output span) and checks the library's answer against it."""

    def __init__(self, delays, nhist, ntu, ndmc, nreq_max):
        self.smax = np.asarray(delays, np.int64).max(axis=1)
        self.ndmf, self.nhist, self.ntu, self.ndmc, self.nreq_max = self.smax.size, nhist, ntu, ndmc, nreq_max
        self.pending = []       # (id, first, last, request tuple)
        self.n = 0

    def reset(self):
        dropped = len(self.pending)
        self.pending, self.n = [], 0
        return dropped

    def add(self, rid, pair, n_c, ic, dstep=1):
        d = ic + (np.arange(self.ndmc) - self.ndmc // 2) * dstep
        d = d[(d >= 0) & (d < self.ndmf)]
        first = n_c - self.ntu // 2
        self.pending.append((rid, first, first + self.ntu - 1 + int(self.smax[d].max()), (rid, pair, n_c, ic, dstep)))

    def take(self, nwin_call):
        """The call of nwin_call windows: (served ids in slot order, expired ids); the rest wait."""
        self.n += nwin_call
        served, expired, keep = [], [], []
        for p in self.pending:
            if p[1] < self.n - self.nhist:
                expired.append(p[0])
            elif p[2] < self.n and len(served) < self.nreq_max:
                served.append(p[0])
            else:
                keep.append(p)
        self.pending = keep
        return served, expired


def cutout_offsets(nreq_max, nband, nt, ndmc):
    """(byte offset of the waterfalls, of the planes, bytes of a served span)."""
    a = CUTOUT_RECORD.itemsize * nreq_max
    b = a + 4 * nreq_max * nband * nt
    return a, b, b + 4 * nreq_max * ndmc * nt


def as_cutouts(span, nreq_max, nband, nt, ndmc):
    """A served span's bytes -> (CUTOUT_RECORD [nreq_max], W f32[nreq_max][nband][nt], P f32[nreq_max][ndmc][nt])."""
    raw = np.ascontiguousarray(span).reshape(-1).view(np.uint8)
    a, b, n = cutout_offsets(nreq_max, nband, nt, ndmc)
    if raw.size != n:
        raise ValueError("pulse_cutout: %d bytes are not a span of %d slots (%d bytes)" % (raw.size, nreq_max, n))
    return raw[:a].view(CUTOUT_RECORD), raw[a:b].view(np.float32).reshape(nreq_max, nband, nt), raw[b:].view(np.float32).reshape(nreq_max, ndmc, nt)


def cutout_refined(record, fine_dms, ic, dstep, ndmc, nt, tscr, seq_c, acc_len):
    """A scored record in physical units: dict(id, dm, width, seq, snr, snr0): dm the fine trial of the winning row, width the boxcar
    in windows, seq the beamformer-clock sample of the boxcar's middle at the top of the band (seq_c is the request's), snr in
    units of 1.4826 MAD of the row with the folded k_mad, snr0 the centre row's.  None for a record without a score."""
    if int(record['status']) != 0 or int(record['i']) < 0:
        return None
    d = int(ic) + (int(record['i']) - ndmc // 2) * int(dstep)
    w = 1 << int(record['iw'])
    # column j ends the boxcar: its scrunched windows are [(j - w + 1) tscr, (j + 1) tscr) of the cut-out, which begins ntu/2 before seq_c
    mid = ((int(record['j']) - w + 1) * tscr + (int(record['j']) + 1) * tscr) / 2.0 - (nt * tscr) // 2
    return dict(id=int(record['id']), dm=float(np.asarray(fine_dms)[d]), idm_fine=d, width=w * tscr, seq=int(round(seq_c + mid * acc_len)),
                snr=float(record['S']), snr0=float(record['S0']))


def cutout_reference(x, delays, pair, n_c, ic, dstep, nband, nt, tscr, ndmc, nwidth, k_mad, weights=None):
    """The float64 statement.  x [nwindows][npair][nfine][4], every window since the reset; returns dict(W [nband][nt],
    P [ndmc][nt], present bool [ndmc], S, S0, i, iw, j, M, A) with i = -1 without a score.  A row's median is the mean of the
    two middle values of the sorted row, its scale k_mad times the median of |P - M|; a row with a value that is not finite or a
    scale that is not positive and finite has no score.  Ties go to the smallest i, then iw, then j."""
    x = np.asarray(x, np.float64)
    s = np.asarray(delays, np.int64)
    ndmf, nfine = s.shape
    w = np.ones(nfine) if weights is None else np.asarray(weights, np.float64)
    ntu, c, Q = nt * tscr, ndmc // 2, nfine // nband
    first = n_c - ntu // 2
    I = np.zeros((x.shape[0], nfine))
    I[:, w != 0] = x[:, pair, w != 0, 0] + x[:, pair, w != 0, 1]
    W, P, present = np.zeros((nband, nt)), np.zeros((ndmc, nt)), np.zeros(ndmc, bool)
    for i in range(ndmc):
        d = ic + (i - c) * dstep
        if not 0 <= d < ndmf:
            continue
        present[i] = True
        for g in range(nband):
            D = np.zeros(ntu)
            for q in range(g * Q, (g + 1) * Q):
                n = first + np.arange(ntu) + s[d, q]
                D[n >= 0] += w[q] * I[n[n >= 0], q]
            P[i] += D.reshape(nt, tscr).sum(axis=1)
            if i == c:
                W[g] = D.reshape(nt, tscr).sum(axis=1)
    out = dict(W=W, P=P, present=present, S=0.0, S0=0.0, i=-1, iw=-1, j=-1, M=0.0, A=0.0)
    for i in np.flatnonzero(present):
        row = P[i]
        if not np.isfinite(row).all():
            continue
        srt = np.sort(row)
        M = 0.5 * (srt[nt // 2 - 1] + srt[nt // 2])
        dev = np.sort(np.abs(row - M))
        A = 0.5 * (dev[nt // 2 - 1] + dev[nt // 2])
        sc = float(k_mad) * A
        if not (sc > 0 and np.isfinite(sc)):
            continue
        B = row - M
        best = None
        for iw in range(nwidth):
            wd = 1 << iw
            C = B / sc * 2.0 ** (-0.5 * iw)
            j = int(np.argmax(C[wd - 1:])) + wd - 1
            if best is None or C[j] > best[0]:
                best = (float(C[j]), iw, j)
            if iw + 1 < nwidth:
                nxt = np.full(nt, -np.inf)
                nxt[2 * wd - 1:] = B[2 * wd - 1:] + B[wd - 1:nt - wd]
                B = nxt
        if i == c:
            out['S0'] = best[0]
        if out['i'] < 0 or best[0] > out['S']:
            out.update(S=best[0], i=int(i), iw=best[1], j=best[2], M=M, A=A)
    return out
