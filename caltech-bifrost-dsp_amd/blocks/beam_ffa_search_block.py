"""BeamFfaSearch: fast-folding search of the dedispersed beams for long-period pulsars.

Reads the output ring of BeamDedisperse in device space: spans of
  f32 [nwin][npair][ndm][nprod]        (nprod = 1: I; nprod = 4: I = XX + YY is formed from the first two words)
and writes one record plane per completed SEGMENT to a host-space output ring,
  [npair][ndm][noct][nwidth] x {f32 snr, i32 p, i32 i, i32 j}      (blocks/ffa_search.py RECORD)
per series (pair, trial), octave and boxcar width the largest matched-filter score over the folds of the segment: windows are
summed nds at a time into samples, segments of nt samples are folded on the device at every base period pmin..pmax and the
fractional periods between, in noct octaves of the time resolution, and a circular boxcar of 1, 2 ... 2^(nwidth-1) samples runs
over every profile (xengFfa*, csrc/ffa_kernels.h; the definition is in include/xeng.h).  Only the call that brings the last
window of a segment reserves and commits an output span; the block counts windows itself to know which one it is.  Once a
plane's kernels have completed the block thresholds it and groups it over DM, octaves and widths (ffa_candidates), publishes
`ncand` and the last plane's `candidates` through its stats and calls on_candidates(list) when the list is not empty.  No
reference counterpart: the reference has no detection stage.

The first dedisp_latency windows of a dedispersed sequence are partial sums, a ramp that would fold up at every period: whole
spans are skipped (counted in `nstartup`) until dedisp_latency windows of the sequence have passed, and the first segment starts
on whole sums.  The output sequence begins there: its header's `seq0` is the beamformer-clock sample of the first segment's first
window, and plane j of the sequence covers the nt * nds windows from seq0 + j * nt * nds * acc_len.

A new sequence or a gap in the input (spans this reader never saw) resets the context; a gap drops the partial segment (counted
in `ndropped`) and the output restarts in a sequence of its own.  A `threshold` command takes effect at the next plane.

Not built: general M (the head / tail fold: up to half a segment is unread where the segment holds just under a power of two of
periods), red-noise detrending by a running median, more than one peak per (series, octave, width), segments beyond 2^14 samples,
harmonic sifting beyond the grouping of ffa_candidates."""
import json

from ..backend import default_backend
from .beam_dedisperse_block import _number, check_dedispersed_header
from .block_base import SKIP, Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .ffa_search import RECORD, as_records, ffa_candidates


def _count(v):
    return isinstance(v, int) and not isinstance(v, bool)


class BeamFfaSearch(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, ndm, nwin, nt, pmin, pmax, nds=1, noct=1, nwidth=4, threshold=8.0, on_candidates=None,
                 guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamFfaSearch, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_FFA_SEARCH"
        if min(npair, ndm, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r ndm=%r nwin=%r must be positive" % (who, npair, ndm, nwin))
        if not _count(nds) or not 1 <= nds <= 65536:
            raise ValueError("%s: nds %r is not a count of windows from 1 to 65536" % (who, nds))
        if not _count(noct) or not 1 <= noct <= 6:
            raise ValueError("%s: noct %r not 1 to 6" % (who, noct))
        if not _count(nt) or not 1 << 8 <= nt <= 1 << 14 or nt % (1 << (noct - 1)):
            raise ValueError("%s: nt %r is not a multiple of 2^(noct-1) from 2^8 to 2^14" % (who, nt))
        if nwin > nt * nds:
            raise ValueError("%s: spans of %r windows are longer than a segment of %d x %d" % (who, nwin, nt, nds))
        if not _count(pmin) or not _count(pmax) or not 16 <= pmin <= pmax or 2 * pmax > nt >> (noct - 1):
            raise ValueError("%s: base periods %r..%r, not 16 <= pmin <= pmax <= %d, half the top octave's segment" % (who, pmin, pmax,
                                                                                                                     (nt >> (noct - 1)) // 2))
        if not _count(nwidth) or not 1 <= nwidth <= 8 or 1 << (nwidth - 1) > pmin // 2:
            raise ValueError("%s: nwidth %r not 1 to 8 with 2^(nwidth-1) <= pmin/2" % (who, nwidth))
        if not _number(threshold):
            raise ValueError("%s: threshold %r is not a finite number" % (who, threshold))
        if on_candidates is not None and not callable(on_candidates):
            raise ValueError("%s: on_candidates is not callable" % who)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the record planes go to a host-space ring" % (who, oring.space))
        self.npair, self.ndm, self.nwin, self.gpu = npair, ndm, nwin, gpu
        self.nds, self.nt, self.noct, self.pmin, self.pmax, self.nwidth = nds, nt, noct, pmin, pmax, nwidth
        self.threshold = float(threshold)
        self.on_candidates = on_candidates
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('threshold', type=(int, float), condition=_number)
        self.update_stats({'nwindow': 0, 'nsegment_done': 0, 'ndropped': 0, 'ncand': 0, 'nstartup': 0, 'candidates': [], 'threshold': self.threshold})
        self._ctx_nprod = None                  # nprod of the live context
        self._nwindows = 0                      # windows given to the context since its last reset

    def _initialize(self, nprod):
        self._call('ffa_initialize', self.gpu, self.npair, self.ndm, self.nwin, nprod, self.nds, self.nt, self.noct, self.pmin, self.pmax, self.nwidth)
        self._ctx_nprod = nprod
        self._nwindows = 0

    def _reset(self):
        self._bf.ffa_reset()
        self._nwindows = 0

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(nds=self.nds, nt=self.nt, noct=self.noct, pmin=self.pmin, pmax=self.pmax, nwidth=self.nwidth, threshold=self.threshold, seq0=start)
        return ohdr

    def _finish(self, osp, meta):
        """A plane whose kernels (and copy) have completed: threshold it, group it, publish; then commit the span."""
        try:
            threshold, dms, tsamp = meta
            plane = as_records(osp.data.numpy().copy(), self.npair, self.ndm, self.noct, self.nwidth)
            cands = ffa_candidates(plane, threshold, dms, self.nt, self.nds, tsamp)
            self.update_stats({'ncand': self.stats['ncand'] + len(cands), 'candidates': cands, 'nsegment_done': self.stats['nsegment_done'] + 1})
            if cands and self.on_candidates is not None:
                self.on_candidates(cands)
        finally:
            osp.close()

    def main(self):
        self.bind()
        ogulp_size = self.npair * self.ndm * self.noct * self.nwidth * RECORD.itemsize
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        ospace = getattr(self.oring, 'space', 'system')
        direct = ospace in (self._bf.space_in, 'cuda_host')     # (the kernel can write the span itself)
        staged = spans_outlive_release(self.iring, self.oring) and ospace == 'cuda_host' and hasattr(self._bf, 'copy_async')
        streaming = spans_outlive_release(self.iring, self.oring) and (direct or staged)
        with InFlight(self._bf.ffa_wait, self._bf.ffa_sync, self._bf, finish=self._finish, mark=self._bf.ffa_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_FFA_SEARCH", inflight, oring, streaming, staged, gap_note=": the segment starts again", count_gaps=False)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _load_pending_commands(self):
        self.update_command_vals()
        if self.command_vals.get('threshold') is not None:
            self.threshold = float(self.command_vals['threshold'])

    def _sequence(self, iseq, loop, ogulp_size):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nprod, acc_len, S, dms, tsamp = check_dedispersed_header("BEAM_FFA_SEARCH", ihdr, self.npair, self.ndm)
        loop.inflight.retire(0)
        if self._ctx_nprod != nprod:
            self._initialize(nprod)
        else:
            self._reset()                       # (a new sequence starts from nothing: no partial sample, no partial segment)
        seq0 = ihdr['seq0']
        nseg_win = self.nt * self.nds           # windows of a segment

        def gap():
            # windows this reader never saw: the segment in progress does not line up with what comes now
            if self._nwindows % nseg_win:
                self.update_stats({'ndropped': self.stats['ndropped'] + 1})
            self._reset()

        def pending(t):
            if self.update_pending:
                self._load_pending_commands()
            if (t - seq0) // acc_len < S:
                self.update_stats({'nstartup': self.stats['nstartup'] + 1})
                return SKIP                     # (the span begins inside the dedisperser's partial sums)

        def search(t, held, out):
            # only the call that completes a segment reserves and writes an output span
            completes = (self._nwindows + self.nwin) // nseg_win > self._nwindows // nseg_win
            rv, completed = self._bf.ffa_run(held, self.nwin, out.target((self.threshold, dms, tsamp)) if completes else None)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("ffa_run returned %d: %s" % (rv, self._bf.last_error()))
            if bool(completed) != completes:
                raise RuntimeError("BEAM_FFA_SEARCH: the context and the block disagree on which call completes a segment")
            self._nwindows += self.nwin
            return {'nwindow': self.stats['nwindow'] + self.nwin}

        # (a span is nwin windows of acc_len samples of the beamformer's clock)
        loop.run(iseq, seq0, self.nwin * self.npair * self.ndm * nprod * 4, self.nwin * acc_len, ogulp_size, lambda t: self.output_header(ihdr, t),
                 search, before=pending, on_gap=gap)
