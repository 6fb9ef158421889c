"""BeamPulseSearch: boxcar single-pulse search of the dedispersed beams.

Reads the output ring of BeamDedisperse in device space: spans of
  f32 [nwin][npair][ndm][nprod]        (nprod = 1: I; nprod = 4: I = XX + YY is formed from the first two words)
and writes one record plane per input span to a host-space output ring,
  [npair][ndm] x {f32 snr, i32 n_call, i32 iw, f32 B}      (blocks/pulse_search.py RECORD)
per series (pair, trial) the best boxcar of the span: a running baseline over blocks of nstat windows, boxcars of 1, 2, 4 ...
2^(nwidth-1) windows, the score in units of the previous block's sigma (xengPulse*, csrc/pulse_kernels.h; the definition is in
include/xeng.h).  The baseline and the last windows live on the device across spans.  Once a plane's kernel has completed the
block thresholds it and groups it over DM (pulse_candidates), adds to each candidate
  sample = seq0 + (n_seq - dedisp_latency - width + 1) * acc_len,
the beamformer-clock sample at which the boxcar begins at the top of the band (n_seq: the boxcar's last window counted from the
beginning of the input sequence), publishes `ncand` and the last span's `candidates` through its stats and calls
on_candidates(list) when the list is not empty.  No reference counterpart: the reference has no detection stage.

The first dedisp_latency windows of a dedispersed sequence are partial sums: the baseline blocks that hold them sit too low, and
the block after them is measured against that.  A record whose boxcar begins before window (ceil(dedisp_latency / nstat) + 1) *
nstat of the sequence -- the first window whose previous block holds whole sums only -- is left out of the candidates (counted in
`nstartup`); the planes in the output ring are what the kernel wrote.

A new sequence or a gap in the input (spans this reader never saw) resets the context; after a gap the output restarts in a
sequence of its own (UpchanSumBeams' rule, as in BeamDedisperse).  A `threshold` command takes effect at the next span.

Not built: a robust baseline (a bright pulse in block k raises sigma for block k+1), clustering in time across spans, and a
trigger writer."""
import json

import numpy as np

from ..backend import default_backend
from .beam_dedisperse_block import _number, check_dedispersed_header
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .pulse_search import RECORD, as_records, pulse_candidates


class BeamPulseSearch(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, ndm, nwin, nwidth=8, nstat=256, threshold=8.0, on_candidates=None, guarantee=True, core=-1,
                 gpu=-1, etcd_client=None, backend=None):
        super(BeamPulseSearch, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_PULSE_SEARCH"
        if min(npair, ndm, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r ndm=%r nwin=%r must be positive" % (who, npair, ndm, nwin))
        if not 1 <= nwidth <= 8:
            raise ValueError("%s: nwidth %r not 1 to 8" % (who, nwidth))
        if not 2 <= nstat <= 1 << 20 or 1 << (nwidth - 1) > nstat:
            raise ValueError("%s: nstat %r not 2 to 2^20, or below the widest boxcar of %d windows" % (who, nstat, 1 << (nwidth - 1)))
        if not _number(threshold):
            raise ValueError("%s: threshold %r is not a finite number" % (who, threshold))
        if on_candidates is not None and not callable(on_candidates):
            raise ValueError("%s: on_candidates is not callable" % who)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the record planes go to a host-space ring" % (who, oring.space))
        self.npair, self.ndm, self.nwin, self.nwidth, self.nstat, self.gpu = npair, ndm, nwin, nwidth, nstat, gpu
        self.widths = [1 << iw for iw in range(nwidth)]
        self.threshold = float(threshold)
        self.on_candidates = on_candidates
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('threshold', type=(int, float), condition=_number)
        self.update_stats({'nwindow': 0, 'ngap': 0, 'ncand': 0, 'nstartup': 0, 'candidates': [], 'threshold': self.threshold})
        self._ctx_nprod = None                  # nprod of the live context

    def _initialize(self, nprod):
        self._call('pulse_initialize', self.gpu, self.npair, self.ndm, self.nwin, nprod, self.nwidth, self.nstat)
        self._ctx_nprod = nprod

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(nwidth=self.nwidth, nstat=self.nstat, widths=list(self.widths), threshold=self.threshold, seq0=start)
        return ohdr

    def _finish(self, osp, meta):
        """A plane whose kernel (and copy) has completed: threshold it, group it over DM, publish; then commit the span."""
        try:
            threshold, n0_seq, seq0, S, acc_len, dms = meta
            plane = as_records(osp.data.numpy().copy(), self.npair, self.ndm)
            trust = (-(-S // self.nstat) + 1) * self.nstat          # the first window whose previous block holds whole sums only
            if n0_seq < trust + self.widths[-1]:
                early = (plane['n'] >= 0) & (n0_seq + plane['n'] - np.left_shift(1, np.maximum(plane['iw'], 0)) + 1 < trust)
                plane['n'][early] = -1
                self.update_stats({'nstartup': self.stats['nstartup'] + int(early.sum())})
            cands = pulse_candidates(plane, threshold, dms, self.widths)
            for c in cands:
                c['sample'] = seq0 + (n0_seq + c['window'] - S - c['width'] + 1) * acc_len
            self.update_stats({'ncand': self.stats['ncand'] + len(cands), 'candidates': cands})
            if cands and self.on_candidates is not None:
                self.on_candidates(cands)
        finally:
            osp.close()

    def main(self):
        self.bind()
        ogulp_size = self.npair * self.ndm * RECORD.itemsize
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        ospace = getattr(self.oring, 'space', 'system')
        direct = ospace in (self._bf.space_in, 'cuda_host')     # (the kernel can write the span itself)
        staged = spans_outlive_release(self.iring, self.oring) and ospace == 'cuda_host' and hasattr(self._bf, 'copy_async')
        streaming = spans_outlive_release(self.iring, self.oring) and (direct or staged)
        with InFlight(self._bf.pulse_wait, self._bf.pulse_sync, self._bf, finish=self._finish, mark=self._bf.pulse_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_PULSE_SEARCH", inflight, oring, streaming, staged, gap_note=": the baseline starts again")
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _sequence(self, iseq, loop, ogulp_size):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nprod, acc_len, S, dms, _ = check_dedispersed_header("BEAM_PULSE_SEARCH", ihdr, self.npair, self.ndm)
        loop.inflight.retire(0)
        if self._ctx_nprod != nprod:
            self._initialize(nprod)
        else:
            self._bf.pulse_reset()              # (a new sequence starts from nothing: no baseline, no boxcar reaches back)
        seq0 = ihdr['seq0']

        def pending(t):
            if self.update_pending:
                self.update_command_vals()
                if self.command_vals.get('threshold') is not None:
                    self.threshold = float(self.command_vals['threshold'])

        def search(t, held, out):
            self._call('pulse_run', held, self.nwin, out.target((self.threshold, (t - seq0) // acc_len, seq0, S, acc_len, dms)))
            return {'nwindow': self.stats['nwindow'] + self.nwin}

        # (a span is nwin windows of acc_len samples of the beamformer's clock; after a gap the baseline and the last windows do
        # not line up with what comes now)
        loop.run(iseq, seq0, self.nwin * self.npair * self.ndm * nprod * 4, self.nwin * acc_len, ogulp_size, lambda t: self.output_header(ihdr, t),
                 search, before=pending, on_gap=self._bf.pulse_reset)
