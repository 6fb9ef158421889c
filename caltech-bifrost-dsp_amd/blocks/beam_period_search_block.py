"""BeamPeriodSearch: FFT periodicity search of the dedispersed beams.

Reads the output ring of BeamDedisperse in device space: spans of
  f32 [nwin][npair][ndm][nprod]        (nprod = 1: I; nprod = 4: I = XX + YY is formed from the first two words)
and writes one record plane per completed STACK to a host-space output ring,
  [npair][ndm][nlevel] x {f32 H, i32 k}      (blocks/period_search.py RECORD)
per series (pair, trial) and harmonic level the largest harmonic sum of the stack and the bin of its top harmonic: segments of nt
windows are transformed, whitened by block means of nwhite bins and stacked nstack at a time on the device, and the call that
brings the last window of a stack forms the sums of 1, 2 ... 2^(nlevel-1) harmonics (xengPeriod*, csrc/period_kernels.h; the
definition is in include/xeng.h).  Only that call reserves and commits an output span; the block counts windows itself to know
which one it is.  Once a plane's kernel has completed the block thresholds it and groups it over DM (period_candidates),
publishes `ncand` and the last plane's `candidates` through its stats and calls on_candidates(list) when the list is not empty.
No reference counterpart: the reference has no detection stage.

The first dedisp_latency windows of a dedispersed sequence are partial sums, a ramp that would put power into the lowest bins of
the first segment: whole spans are skipped (counted in `nstartup`) until dedisp_latency windows of the sequence have passed, and
the first stack starts on whole sums.  The output sequence begins there: its header's `seq0` is the beamformer-clock sample of
the first stack's first window, and plane j of the sequence covers the nt * nstack windows from seq0 + j * nt * nstack * acc_len.

A new sequence or a gap in the input (spans this reader never saw) resets the context; a gap drops the partial stack (counted
in `ndropped`) and the output restarts in a sequence of its own.  A `threshold` command takes effect at the next plane; a `mask`
command, a list of [k_lo, k_hi) bin ranges to zap, is applied through xengPeriodSetMask before the next span and holds from the
next segment to complete.

Not built: acceleration search, median whitening, more than one peak per series and level, sifting of harmonically related
candidates, segments beyond 2^14 windows."""
import json

import numpy as np

from ..backend import default_backend
from .beam_dedisperse_block import _number, check_dedispersed_header
from .block_base import SKIP, Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .period_search import RECORD, as_records, period_candidates


def _ranges(v):
    return isinstance(v, list) and all(isinstance(r, list) and len(r) == 2 and all(isinstance(k, int) and not isinstance(k, bool) for k in r) and
                                       0 <= r[0] <= r[1] for r in v)


class BeamPeriodSearch(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, ndm, nwin, nt, nstack=1, nlevel=5, nwhite=64, kmin=2, threshold=6.0, on_candidates=None,
                 guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamPeriodSearch, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_PERIOD_SEARCH"
        if min(npair, ndm, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r ndm=%r nwin=%r must be positive" % (who, npair, ndm, nwin))
        if not isinstance(nt, int) or not 1 << 8 <= nt <= 1 << 14 or nt & (nt - 1):
            raise ValueError("%s: nt %r is not a power of two from 2^8 to 2^14" % (who, nt))
        if nwin > nt:
            raise ValueError("%s: spans of %r windows are longer than a segment of %d" % (who, nwin, nt))
        if not isinstance(nstack, int) or nstack < 1:
            raise ValueError("%s: nstack %r is not a positive count" % (who, nstack))
        if not 1 <= nlevel <= 5:
            raise ValueError("%s: nlevel %r not 1 to 5" % (who, nlevel))
        if not isinstance(nwhite, int) or not 8 <= nwhite <= nt // 2 or nwhite & (nwhite - 1):
            raise ValueError("%s: nwhite %r is not a power of two from 8 to nt/2" % (who, nwhite))
        if not 1 <= kmin < nt // 32:
            raise ValueError("%s: kmin %r not in 1 .. nt/32 - 1" % (who, kmin))
        if not _number(threshold):
            raise ValueError("%s: threshold %r is not a finite number" % (who, threshold))
        if on_candidates is not None and not callable(on_candidates):
            raise ValueError("%s: on_candidates is not callable" % who)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the record planes go to a host-space ring" % (who, oring.space))
        self.npair, self.ndm, self.nwin, self.gpu = npair, ndm, nwin, gpu
        self.nt, self.nstack, self.nlevel, self.nwhite, self.kmin = nt, nstack, nlevel, nwhite, kmin
        self.threshold = float(threshold)
        self.on_candidates = on_candidates
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('threshold', type=(int, float), condition=_number)
        self.define_command_key('mask', type=list, condition=_ranges)
        self.update_stats({'nwindow': 0, 'nstack_done': 0, 'ndropped': 0, 'ncand': 0, 'nstartup': 0, 'candidates': [], 'threshold': self.threshold})
        self._ctx_nprod = None                  # nprod of the live context
        self._mask = None                       # the ranges in force (None: all kept)
        self._nwindows = 0                      # windows given to the context since its last reset

    def _initialize(self, nprod):
        self._call('period_initialize', self.gpu, self.npair, self.ndm, self.nwin, nprod, self.nt, self.nstack, self.nlevel, self.nwhite, self.kmin)
        self._ctx_nprod = nprod
        self._nwindows = 0
        if self._mask:
            self._set_mask(self._mask)          # (a new context keeps everything)

    def _set_mask(self, ranges):
        keep = np.ones(self.nt // 2, np.uint8)
        for lo, hi in ranges:
            keep[lo:hi] = 0
        self._call('period_set_mask', keep)
        self._mask = ranges

    def _reset(self):
        self._bf.period_reset()
        self._nwindows = 0

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(nt=self.nt, nstack=self.nstack, nlevel=self.nlevel, nwhite=self.nwhite, kmin=self.kmin, threshold=self.threshold, seq0=start)
        return ohdr

    def _finish(self, osp, meta):
        """A plane whose kernel (and copy) has completed: threshold it, group it over DM, publish; then commit the span."""
        try:
            threshold, dms, tsamp = meta
            plane = as_records(osp.data.numpy().copy(), self.npair, self.ndm, self.nlevel)
            cands = period_candidates(plane, threshold, dms, self.nt, self.nstack, tsamp)
            self.update_stats({'ncand': self.stats['ncand'] + len(cands), 'candidates': cands, 'nstack_done': self.stats['nstack_done'] + 1})
            if cands and self.on_candidates is not None:
                self.on_candidates(cands)
        finally:
            osp.close()

    def main(self):
        self.bind()
        ogulp_size = self.npair * self.ndm * self.nlevel * RECORD.itemsize
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        ospace = getattr(self.oring, 'space', 'system')
        direct = ospace in (self._bf.space_in, 'cuda_host')     # (the kernel can write the span itself)
        staged = spans_outlive_release(self.iring, self.oring) and ospace == 'cuda_host' and hasattr(self._bf, 'copy_async')
        streaming = spans_outlive_release(self.iring, self.oring) and (direct or staged)
        with InFlight(self._bf.period_wait, self._bf.period_sync, self._bf, finish=self._finish, mark=self._bf.period_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_PERIOD_SEARCH", inflight, oring, streaming, staged, gap_note=": the stack starts again", count_gaps=False)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _load_pending_commands(self):
        self.update_command_vals()
        if self.command_vals.get('threshold') is not None:
            self.threshold = float(self.command_vals['threshold'])
        if self.command_vals.get('mask') is not None and self.command_vals['mask'] != self._mask:
            if any(hi > self.nt // 2 for _, hi in self.command_vals['mask']):
                self.log.warning("BEAM_PERIOD_SEARCH >> a mask beyond bin %d is ignored" % (self.nt // 2))
            else:
                self._set_mask(self.command_vals['mask'])

    def _sequence(self, iseq, loop, ogulp_size):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nprod, acc_len, S, dms, tsamp = check_dedispersed_header("BEAM_PERIOD_SEARCH", ihdr, self.npair, self.ndm)
        loop.inflight.retire(0)
        if self._ctx_nprod != nprod:
            self._initialize(nprod)
        else:
            self._reset()                       # (a new sequence starts from nothing: no partial segment, no partial stack)
        seq0 = ihdr['seq0']
        nstack_win = self.nt * self.nstack      # windows of a stack

        def gap():
            # windows this reader never saw: the segment and the stack in progress do not line up with what comes now
            if self._nwindows % nstack_win:
                self.update_stats({'ndropped': self.stats['ndropped'] + 1})
            self._reset()

        def pending(t):
            if self.update_pending:
                self._load_pending_commands()
            if (t - seq0) // acc_len < S:
                self.update_stats({'nstartup': self.stats['nstartup'] + 1})
                return SKIP                     # (the span begins inside the dedisperser's partial sums)

        def search(t, held, out):
            # only the call that completes a stack reserves and writes an output span
            completes = (self._nwindows + self.nwin) // nstack_win > self._nwindows // nstack_win
            rv, completed = self._bf.period_run(held, self.nwin, out.target((self.threshold, dms, tsamp)) if completes else None)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("period_run returned %d: %s" % (rv, self._bf.last_error()))
            if bool(completed) != completes:
                raise RuntimeError("BEAM_PERIOD_SEARCH: the context and the block disagree on which call completes a stack")
            self._nwindows += self.nwin
            return {'nwindow': self.stats['nwindow'] + self.nwin}

        # (a span is nwin windows of acc_len samples of the beamformer's clock)
        loop.run(iseq, seq0, self.nwin * self.npair * self.ndm * nprod * 4, self.nwin * acc_len, ogulp_size, lambda t: self.output_header(ihdr, t),
                 search, before=pending, on_gap=gap)
