"""BeamDetrend: running-median baseline removal of the dedispersed beams.

Reads the output ring of BeamDedisperse, in device space: spans of
  f32 [nwin][npair][ndm][nprod]
and writes a ring of f32 [nwin][npair][ndm] with a header that check_dedispersed_header accepts (nprod = 1), so that BeamPulseSearch,
BeamPeriodSearch(Long), BeamAccelSearch, BeamFfaSearch and BeamCandFold read it unchanged (BeamRfiClean and BeamCoherentDedisperse
stand in their rings the same way).  Per (pair, trial) series and per block of nblk windows the median and the median absolute
deviation make a knot; every window loses the line between the two knots around it and, with `normalise`, is scaled to units of
1.4826 MAD by the line between the knots' reciprocal scales (xengDetrend*, csrc/detrend_kernels.h; the definition is in
include/xeng.h).  Excised data is +0.  No reference counterpart.

The engine's output is D = 3 nblk / 2 windows late; the block hides that as BeamRfiClean does: it enqueues every span and does not
commit the first D / nwin outputs.  It also drops the start-up: the dedisperser's first dedisp_latency windows are partial sums, and
every window that lies against a knot that saw some is left out (detrend_startup spans; the header's detrend_nskipped, in
windows).  The output sequence begins at the first kept span's time tag, and seq0 is advanced to it: output span j is the
detrended input span detrend_startup + j under that span's own time.  The last D windows of a sequence are not flushed.  A new
sequence or a gap in the input resets the context; after a gap the output restarts in a sequence of its own, short by the same
spans.  knots() returns the newest decided block's tables.
"""
import json

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray
from .beam_dedisperse_block import check_dedispersed_header
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .detrend import NBLK_MAX, NBLK_MIN, detrend_k_mad, detrend_startup


def _count(v):
    return isinstance(v, int) and not isinstance(v, bool)


class BeamDetrend(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, ndm, nwin, nblk, normalise=True, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamDetrend, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_DETREND"
        if not all(_count(v) for v in (npair, ndm, nwin, nblk)) or min(npair, ndm, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r ndm=%r nwin=%r nblk=%r must be positive integers" % (who, npair, ndm, nwin, nblk))
        if npair * ndm > 1 << 24:
            raise ValueError("%s: %d pairs x %d trials are more than 2^24 series" % (who, npair, ndm))
        if nblk % 2 or not NBLK_MIN <= nblk <= NBLK_MAX or nwin > nblk:
            raise ValueError("%s: blocks of nblk=%r windows, not an even number from %d to %d and at least nwin=%r" % (who, nblk, NBLK_MIN, NBLK_MAX, nwin))
        if (3 * nblk // 2) % nwin:
            raise ValueError("%s: the latency of 3 nblk / 2 = %d windows is not a whole number of spans of nwin=%r" % (who, 3 * nblk // 2, nwin))
        if not isinstance(normalise, (bool, int)):
            raise ValueError("%s: normalise %r is not a truth value" % (who, normalise))
        if (3 * nblk // 2 + nwin) * npair * ndm * 4 >= 1 << 32:
            raise ValueError("%s: a history of %d + %d windows of %d x %d series is 4 GiB or more" % (who, 3 * nblk // 2, nwin, npair, ndm))
        self.npair, self.ndm, self.nwin, self.nblk, self.normalise, self.gpu = npair, ndm, nwin, nblk, bool(normalise), gpu
        self.nhead = (3 * nblk // 2) // nwin        # spans of a sequence whose output lies before it
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.update_stats({'nwindow': 0, 'ngap': 0, 'nblock': 0})
        self._live = None                       # the nprod the context was made for
        self._scratch = None                    # where the outputs that are not committed go

    def knots(self):
        """(M, A float32, valid uint8, each [npair][ndm]) of the newest decided block; waits for the context's work."""
        return self._bf.detrend_knots(self.npair, self.ndm)

    def output_header(self, ihdr, start, nstart):
        ohdr = ihdr.copy()
        ohdr.update(nprod=1, detrended=True, detrend_nblk=self.nblk, detrend_normalised=self.normalise, detrend_nskipped=nstart * self.nwin, seq0=start)
        return ohdr

    def main(self):
        self.bind()
        ogulp_size = self.nwin * self.npair * self.ndm * 4
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        streaming = spans_outlive_release(self.iring, self.oring)
        staged = streaming and self.oring.space == 'cuda_host' and hasattr(self._bf, 'copy_async')
        with InFlight(self._bf.detrend_wait, self._bf.detrend_sync, self._bf, mark=self._bf.detrend_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_DETREND", inflight, oring, streaming, staged, gap_note=": the baseline starts again")
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _sequence(self, iseq, loop, ogulp_size):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nprod, acc_len, S, _, _ = check_dedispersed_header("BEAM_DETREND", ihdr, self.npair, self.ndm)
        if ihdr.get('detrended'):
            raise ValueError("BEAM_DETREND: the input carries 'detrended': its baseline has been removed already")
        loop.inflight.retire(0)
        if self._live != nprod:
            self._call('detrend_initialize', self.gpu, self.npair, self.ndm, self.nwin, nprod, self.nblk, int(self.normalise), detrend_k_mad())
            self._live = nprod
        else:
            self._bf.detrend_reset()
        if self._scratch is None:
            self._scratch = XArray(shape=(ogulp_size,), dtype=np.uint8, space=self._bf.space_in)
        nstart = detrend_startup(S, self.nblk, self.nwin)
        state = {'n': 0}                        # spans given to the context since its last reset
        step = self.nwin * acc_len
        igulp_size = ogulp_size * nprod

        def gap():
            self._bf.detrend_reset()
            state['n'] = 0

        def detrend(t, held, out):
            head = state['n'] < self.nhead + nstart
            rv, decided = self._bf.detrend_run(held, self.nwin, self._scratch if head else out.target())
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("detrend_run returned %d: %s" % (rv, self._bf.last_error()))
            state['n'] += 1
            return {'nwindow': self.stats['nwindow'] + self.nwin, 'nblock': self.stats['nblock'] + int(bool(decided))}

        # (a span is nwin windows of acc_len samples of the beamformer's clock.  SpanLoop begins the output sequence at the first
        # input span, under the time tag of the span nstart later; the first output span is reserved nhead + nstart spans later
        # and is that span, detrended)
        loop.run(iseq, ihdr['seq0'], igulp_size, step, ogulp_size, lambda t: self.output_header(ihdr, t, nstart), detrend, on_gap=gap,
                 tag_offset=nstart * step)
