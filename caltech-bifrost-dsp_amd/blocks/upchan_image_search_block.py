"""UpchanImageSearch: dedispersed transient search of the images, every pixel a beam.

Reads the output ring of UpchanImage, or of UpchanClean, in device space: one span per integration,
  f32 [ngroup][4][npix] = [XX, YY, Re(XY), Im(XY)]       (a cleaned span's components and stats behind it are not read)
and writes one record plane per integration to a host-space output ring,
  [npix] x {f32 snr, i16 idm, i16 iw}                     (blocks/image_search.py IMSEARCH_RECORD)
per pixel the best boxcar over the DM trials: the channel groups are the frequency axis and the integrations the time axis.  Per
(group, pixel) a running baseline over blocks of nstat integrations normalises I = XX + YY; per (trial, pixel) the groups are summed
along the trial's delays; boxcars of 1, 2, 4 ... 2^(nwidth-1) integrations are scored in units of sigma (xengImsearch*,
csrc/imsearch_kernels.h; the definition is in include/xeng.h).  The baselines, the delayed series and the last sums live on the
device across spans.

The delay table is built per sequence from the header's group frequencies (image_sfreq, image_bw_hz) and the integration length
tint = acc_len * nchan / bw_hz, BeamDedisperse's window length; S = max delay is the block's latency in integrations
(`imsearch_latency`): output n is the event that reached the top of the band at integration n - S.  Once a plane's kernels have
completed the block thresholds it and clusters it over the sky (image_candidates), adds to each candidate
  sample = seq0 + (n_seq - S - width + 1) * acc_len,
the sample at which the boxcar begins at the top of the band (n_seq: the integration counted from the beginning of the input
sequence; `window` is n_seq), publishes `ncand`, the last plane's `candidates` and `saturated` through its stats and calls
on_candidates(list) when the list is not empty.  No reference counterpart: the reference has no detection stage.

A new sequence or a gap in the input resets the context; after a gap the output restarts in a sequence of its own.  `threshold` and
`weights` commands, and set_weights, hold from the next integration; no boxcar reaches back before new weights.

Not built: a robust baseline (a bright event in block k raises sigma for block k+1), a boxcar that crosses a block boundary uses
two baselines, fractional delays, Stokes other than I, pixels that track the sky (the list is fixed: the block baseline absorbs a
steady source only while it stays within a pixel over nstat integrations), clustering in time across planes, a trigger writer."""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from .beam_dedisperse_block import _number
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .image_search import IMSEARCH_RECORD, as_records, group_frequencies, image_candidates, image_dm_delays
from .imaging import check_fine_axis

MAX_NWIDTH = 6          # IS_MAX_NWIDTH
MAX_NDM = 1024


class UpchanImageSearch(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, lmn, dms, nwidth=4, nstat=64, threshold=8.0, radius=0.035, weights=None, max_delay=256, on_candidates=None,
                 max_above=4096, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanImageSearch, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_IMAGE_SEARCH"
        try:
            self.lmn = np.ascontiguousarray(lmn, np.float64)
            self.dms = np.ascontiguousarray(dms, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("%s: lmn and dms must be arrays of numbers" % who)
        if self.lmn.ndim != 2 or self.lmn.shape[1] != 3 or not self.lmn.shape[0] or not np.isfinite(self.lmn).all():
            raise ValueError("%s: lmn must be finite [npix][3], not %r" % (who, self.lmn.shape))
        if not 1 <= self.dms.size <= MAX_NDM or not np.isfinite(self.dms).all() or (self.dms < 0).any():
            raise ValueError("%s: 1 to %d finite DM trials >= 0 are required" % (who, MAX_NDM))
        if isinstance(nwidth, bool) or not isinstance(nwidth, (int, np.integer)) or not 1 <= nwidth <= MAX_NWIDTH:
            raise ValueError("%s: nwidth %r not 1 to %d" % (who, nwidth, MAX_NWIDTH))
        if isinstance(nstat, bool) or not isinstance(nstat, (int, np.integer)) or not 2 <= nstat <= 1 << 20 or 1 << (nwidth - 1) > nstat:
            raise ValueError("%s: nstat %r not 2 to 2^20, or below the widest boxcar of %d integrations" % (who, nstat, 1 << (nwidth - 1)))
        if not _number(threshold):
            raise ValueError("%s: threshold %r is not a finite number" % (who, threshold))
        if not _number(radius) or radius < 0:
            raise ValueError("%s: radius %r is not a finite number >= 0" % (who, radius))
        if isinstance(max_delay, bool) or not isinstance(max_delay, (int, np.integer)) or max_delay < 0:
            raise ValueError("%s: max_delay %r is not an integer >= 0" % (who, max_delay))
        if isinstance(max_above, bool) or not isinstance(max_above, (int, np.integer)) or max_above < 1:
            raise ValueError("%s: max_above %r is not a positive integer" % (who, max_above))
        if on_candidates is not None and not callable(on_candidates):
            raise ValueError("%s: on_candidates is not callable" % who)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the record planes go to a host-space ring" % (who, oring.space))
        self.npix, self.ndm = self.lmn.shape[0], self.dms.size
        self.nwidth, self.nstat, self.max_delay, self.max_above, self.gpu = int(nwidth), int(nstat), int(max_delay), int(max_above), gpu
        self.widths = [1 << iw for iw in range(self.nwidth)]
        self.threshold, self.radius = float(threshold), float(radius)
        self.on_candidates = on_candidates
        self._ngroup = None                     # ngroup of the sequence being read
        self._weights = None if weights is None else self._checked_weights(weights)     # None: all ones, whatever the group count
        self._next_weights = None               # set_weights: what the next integration takes
        self._weights_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('threshold', type=(int, float), condition=_number)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.update_stats({'nsearched': 0, 'ngap': 0, 'ncand': 0, 'candidates': [], 'saturated': False, 'threshold': self.threshold})
        self._ctx = None                        # ngroup of the live context

    def _checked_weights(self, w, quiet=False, ngroup=None):
        """f32 [ngroup], finite and >= 0 with one above 0 (of the sequence's length once one is being read); else ValueError, or
        None if `quiet`."""
        ngroup = self._ngroup if ngroup is None else ngroup
        try:
            a = np.ascontiguousarray(w, np.float32)
            ok = a.ndim == 1 and a.size > 0 and (ngroup is None or a.size == ngroup) and np.isfinite(a).all() and (a >= 0).all() and (a > 0).any()
        except (TypeError, ValueError):
            ok = False
        if not ok:
            if quiet:
                return None
            raise ValueError("UPCHAN_IMAGE_SEARCH: the weights must be%s finite numbers >= 0, one above 0" % ("" if ngroup is None else " %d" % ngroup))
        return a

    def set_weights(self, w):
        """Per-group weights from the next integration on (0: the group is left out)."""
        a = self._checked_weights(w)
        with self._weights_lock:
            self._next_weights = a

    def _check_header(self, ihdr):
        """UpchanImage's output or UpchanClean's; returns (ngroup, acc_len, tint, span_bytes)."""
        who = "UPCHAN_IMAGE_SEARCH"
        if ihdr.get('npix') != self.npix:
            raise ValueError("%s: 'npix' is %r in the header, %d directions here: not UpchanImage's images of this list" % (who, ihdr.get('npix'), self.npix))
        if ihdr.get('nprod') != 4:
            raise ValueError("%s: 'nprod' is %r in the header: four-word images only" % (who, ihdr.get('nprod')))
        if ihdr.get('nbit') != 32 or ihdr.get('complex'):
            raise ValueError("%s: the input is not f32 images (nbit %r, complex %r)" % (who, ihdr.get('nbit'), ihdr.get('complex')))
        nfine, nfavg = ihdr.get('nfine'), ihdr.get('nfavg')
        for k, v in (('nfine', nfine), ('nfavg', nfavg)):
            if not isinstance(v, int) or isinstance(v, bool) or v <= 0:
                raise ValueError("%s: the header's '%s' is %r: not UpchanImage's images" % (who, k, v))
        if nfine % nfavg:
            raise ValueError("%s: the header's nfavg %d does not divide its nfine %d" % (who, nfavg, nfine))
        ngroup = nfine // nfavg
        acc_len = check_fine_axis(who, ihdr)
        for k in ('nchan', 'bw_hz'):
            if not _number(ihdr.get(k)) or not ihdr[k] > 0:
                raise ValueError("%s: the header's '%s' is %r: no integration length in seconds" % (who, k, ihdr.get(k)))
        span_bytes = ngroup * 4 * self.npix * 4
        if ihdr.get('cleaned'):                 # (the residual is at the front, and the header says where the span ends)
            so = ihdr.get('stats_offset')
            if not isinstance(so, int) or isinstance(so, bool) or so < span_bytes:
                raise ValueError("%s: a cleaned input whose 'stats_offset' is %r" % (who, so))
            span_bytes = max(so + 16 * ngroup, ihdr.get('span_bytes', 0))
        return ngroup, acc_len, acc_len * ihdr['nchan'] / ihdr['bw_hz'], span_bytes

    def output_header(self, ihdr, start, S, tint):
        ohdr = ihdr.copy()
        ohdr.update(ndm=self.ndm, dms=self.dms.tolist(), nwidth=self.nwidth, widths=list(self.widths), nstat=self.nstat, imsearch_latency=int(S),
                    tint=tint, threshold=self.threshold, seq0=start)
        return ohdr

    def _finish(self, osp, meta):
        """A plane whose kernels (and copy) have completed: threshold it, cluster it over the sky, publish; then commit the span."""
        try:
            threshold, n_seq, seq0, S, acc_len = meta
            plane = as_records(osp.data.numpy().copy(), self.npix)
            cands = image_candidates(plane, threshold, self.lmn, self.radius, self.dms, self.widths, self.max_above)
            for c in cands:
                c['window'] = n_seq
                c['sample'] = seq0 + (n_seq - S - c['width'] + 1) * acc_len
            self.update_stats({'ncand': self.stats['ncand'] + len(cands), 'candidates': list(cands), 'saturated': bool(cands.saturated)})
            if cands and self.on_candidates is not None:
                self.on_candidates(list(cands))
        finally:
            osp.close()

    def _load_pending(self):
        """set_weights and the commands: the weights on the device before the next integration is enqueued (SetWeights waits for
        the integrations in flight, so each of those keeps the weights it was enqueued with)."""
        with self._weights_lock:
            w, self._next_weights = self._next_weights, None
        if self.update_pending:
            cmd = self.take_commands(('threshold', 'weights'))
            if cmd.get('threshold') is not None:
                self.threshold = float(cmd['threshold'])
            if cmd.get('weights') is not None:
                w = self._checked_weights(cmd['weights'])
            self.update_stats({'threshold': self.threshold})    # (a taken command leaves None in the stats)
        if w is not None:
            self._weights = self._checked_weights(w)
            self._call('imsearch_set_weights', self._weights)

    def main(self):
        self.bind()
        ogulp_size = self.npix * IMSEARCH_RECORD.itemsize
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        ospace = getattr(self.oring, 'space', 'system')
        direct = ospace in (self._bf.space_in, 'cuda_host')     # (the kernel can write the span itself)
        staged = spans_outlive_release(self.iring, self.oring) and ospace == 'cuda_host' and hasattr(self._bf, 'copy_async')
        streaming = spans_outlive_release(self.iring, self.oring) and (direct or staged)
        with InFlight(self._bf.imsearch_wait, self._bf.imsearch_sync, self._bf, finish=self._finish, mark=self._bf.imsearch_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_IMAGE_SEARCH", inflight, oring, streaming, staged, gap_note=": the search starts again")
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _sequence(self, iseq, loop, ogulp_size):
        who = "UPCHAN_IMAGE_SEARCH"
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        ngroup, acc_len, tint, span_bytes = self._check_header(ihdr)
        try:
            table = image_dm_delays(group_frequencies(ihdr, ngroup), self.dms, tint)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        S = int(table.max())
        if S > self.max_delay:
            raise ValueError("%s: DM %g needs a delay of %d integrations of %g s, max_delay is %d" % (who, self.dms.max(), S, tint, self.max_delay))
        if self._weights is not None and self._weights.size != ngroup:
            raise ValueError("%s: %d weights for the header's %d channel groups" % (who, self._weights.size, ngroup))
        loop.inflight.retire(0)
        self._ngroup = ngroup
        if self._ctx != ngroup:
            self._call('imsearch_initialize', self.gpu, self.npix, ngroup, self.ndm, self.max_delay, self.nwidth, self.nstat)
            self._ctx = ngroup
        self._call('imsearch_set_weights', np.ones(ngroup, np.float32) if self._weights is None else self._weights)
        self._call('imsearch_set_delays', table)        # (resets: a new sequence starts from nothing)
        seq0 = ihdr['seq0']

        def pending(t):
            if self.update_pending or self._next_weights is not None:
                self._load_pending()

        def search(t, held, out):
            self._call('imsearch_run', held, out.target((self.threshold, (t - seq0) // acc_len, seq0, S, acc_len)))
            return {'nsearched': self.stats['nsearched'] + 1}

        # (after a gap the baselines, the delayed series and the last sums do not line up with what comes now)
        loop.run(iseq, seq0, span_bytes, acc_len, ogulp_size, lambda t: self.output_header(ihdr, t, S, tint), search, before=pending,
                 on_gap=self._bf.imsearch_reset)
