"""BeamCandFold: folds the candidates of the searches and refines their period and period derivative.

Reads the output ring of BeamDedisperse in device space: spans of
  f32 [nwin][npair][ndm][nprod]        (nprod = 1: I; nprod = 4: I = XX + YY is formed from the first two words)
and writes one span per completed SEGMENT of nsub * nsubwin windows to a host-space output ring,
  ncand_max x {f32 S, f32 S0, i16 it, i16 iw, i16 j, i16 pad}     (blocks/cand_fold.py CANDFOLD_RECORD)
  f32 [ncand_max][nbin]                                            the best profiles, at the header's `profile_offset`
Every candidate is folded from its own (pair, trial) series at its own frequency (and derivative) into nsub sub-integrations x nbin
phase bins; when a segment is full the device searches the (2 ndrift + 1) x (2 ncurve + 1) table of drift / bow offsets
(candfold_trials) and boxcar widths 1, 2 .. 2^(nwidth-1) bins over the folded cube, and one record and one best profile per
candidate come out (xengCandfold*, csrc/candfold_kernels.h; the definition is in include/xeng.h).  Only the call that brings the
last window of a segment reserves and commits an output span.  The block then fetches the segment's cube for a robust sigma per
candidate (candfold_sigma: the call waits for that segment's kernels, once per segment), and once the span's kernels have completed
it expresses the records in sigma, publishes `nfolded` and the refined list `folded` through its stats and calls on_folded(list)
when the list is not empty.  No reference counterpart: the reference has no detection stage.

Candidates come from period_candidates[_long], accel_candidates, ffa_candidates or period_sift: dicts with `pair`, `idm` and `freq`
or `period`, optionally `accel` (m/s^2) and `seq_mid`, the beamformer-clock sample of the middle of the segment they were found
in; `freq` is the spin frequency there (candfold_oscillators derives why an accel_candidates entry's is).  Without `seq_mid` the
frequency is taken to hold at the window the set starts at.  Candidates found in one segment are
folded in the segments that FOLLOW: the searches report a segment when it is over, and this block folds what comes after a set was
given, never what has passed.  `candidates=` at construction holds from the first segment; a `candidates` command or
set_candidates() holds from the next segment: the segment in progress is finished with the set it began with, and the output
goes on in a sequence of its own whose header carries the new list.  At most ncand_max candidates; an empty list is refused.

The first dedisp_latency windows of a dedispersed sequence are partial sums: whole spans are skipped (counted in `nstartup`) until
they have passed, and the output sequence begins there: its header's `seq0` is the beamformer-clock sample of the first segment's
first window.  A new sequence or a gap in the input resets the context; a gap drops the partial segment (counted in `ndropped`).
A segment is a whole number of spans (nsub * nsubwin is a multiple of nwin).

Not built: DM refinement (it needs the channelised data, which BeamFold has), interpolated (sub-bin) shifts, a chi^2 statistic,
plots or archive output, and a second derivative of the period (jerk)."""
import json

from ..backend import default_backend
from .beam_dedisperse_block import _number, check_dedispersed_header
from .block_base import RESTART, SKIP, Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .cand_fold import CANDFOLD_RECORD, as_records_candfold, candfold_candidates, candfold_gains, candfold_oscillators, candfold_sigma, candfold_trials


def _count(v):
    return isinstance(v, int) and not isinstance(v, bool)


class BeamCandFold(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, ndm, nwin, ncand_max, nbin, nsub, nsubwin, nwidth=4, ndrift=8, ncurve=4, step=16, candidates=None,
                 threshold=8.0, on_folded=None, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamCandFold, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_CAND_FOLD"
        if min(npair, ndm, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r ndm=%r nwin=%r must be positive" % (who, npair, ndm, nwin))
        if not _count(ncand_max) or not 1 <= ncand_max <= 4096:
            raise ValueError("%s: ncand_max %r not 1 to 4096" % (who, ncand_max))
        if not _count(nbin) or not 16 <= nbin <= 256 or nbin & (nbin - 1):
            raise ValueError("%s: nbin %r is not a power of two from 16 to 256" % (who, nbin))
        if not _count(nsub) or not 2 <= nsub <= 64 or nsub * nbin > 8192:
            raise ValueError("%s: nsub %r not 2 to 64 with nsub * nbin <= 8192" % (who, nsub))
        if not _count(nsubwin) or nsubwin < 1 or nsub * nsubwin >= 1 << 31:
            raise ValueError("%s: nsubwin %r is not a count of windows with nsub * nsubwin < 2^31" % (who, nsubwin))
        if (nsub * nsubwin) % nwin:
            raise ValueError("%s: a segment of %d x %d windows is not a whole number of spans of %r" % (who, nsub, nsubwin, nwin))
        if not _count(nwidth) or nwidth < 1 or 1 << (nwidth - 1) > nbin // 2:
            raise ValueError("%s: nwidth %r not 1 or more with 2^(nwidth-1) <= nbin/2" % (who, nwidth))
        try:
            self.d1, self.d2 = candfold_trials(ndrift, ncurve, step)
        except (TypeError, ValueError) as e:
            raise ValueError("%s: %s" % (who, e))
        if not _number(threshold):
            raise ValueError("%s: threshold %r is not a finite number" % (who, threshold))
        if on_folded is not None and not callable(on_folded):
            raise ValueError("%s: on_folded is not callable" % who)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the records go to a host-space ring" % (who, oring.space))
        self.npair, self.ndm, self.nwin, self.gpu = npair, ndm, nwin, gpu
        self.ncand_max, self.nbin, self.nsub, self.nsubwin, self.nwidth = ncand_max, nbin, nsub, nsubwin, nwidth
        self.nt = nsub * nsubwin
        self.gains = candfold_gains(nbin, nwidth)
        self.threshold = float(threshold)
        self.on_folded = on_folded
        self._waiting = None                    # a candidate list that holds from the next segment
        if candidates is not None:
            self._waiting = self._checked(candidates)
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('threshold', type=(int, float), condition=_number)
        self.define_command_key('candidates', type=list, condition=self._candidates_ok)
        self.update_stats({'nwindow': 0, 'nsegment_done': 0, 'ndropped': 0, 'nfolded': 0, 'nstartup': 0, 'folded': [], 'threshold': self.threshold, 'ncand': 0})
        self._ctx_nprod = None                  # nprod of the live context
        self._nwindows = 0                      # windows given to the context since its last reset
        self._cands, self._oscs = [], []        # the set in force and its oscillators

    def _checked(self, cands):
        who = "BEAM_CAND_FOLD"
        if not isinstance(cands, (list, tuple)) or not 1 <= len(cands) <= self.ncand_max:
            raise ValueError("%s: candidates are not a list of 1 to %d" % (who, self.ncand_max))
        out = []
        for c in cands:
            if not isinstance(c, dict) or not _count(c.get('pair')) or not _count(c.get('idm')) or not 0 <= c['pair'] < self.npair or not 0 <= c['idm'] < self.ndm:
                raise ValueError("%s: a candidate needs a pair below %d and a trial idm below %d: %r" % (who, self.npair, self.ndm, c))
            f = c.get('freq', None)
            if f is None and _number(c.get('period')) and c['period'] > 0:
                f = 1.0 / c['period']
            if not _number(f) or not f > 0 or ('accel' in c and not _number(c['accel'])) or ('seq_mid' in c and not _count(c['seq_mid'])):
                raise ValueError("%s: a candidate needs a positive freq or period, a finite accel and an integer seq_mid: %r" % (who, c))
            keep = dict(pair=c['pair'], idm=c['idm'], freq=float(f))
            for k in ('accel', 'seq_mid'):
                if k in c:
                    keep[k] = c[k]
            out.append(keep)
        return out

    def _candidates_ok(self, v):
        try:
            self._checked(v)
            return True
        except ValueError:
            return False

    def set_candidates(self, candidates):
        """The list that holds from the next segment (checked here; ValueError)."""
        cands = self._checked(candidates)
        self.acquire_control_lock()
        try:
            self._waiting = cands
            self.update_pending = True
        finally:
            self.release_control_lock()

    def _initialize(self, nprod):
        self._call('candfold_initialize', self.gpu, self.npair, self.ndm, self.nwin, nprod, self.ncand_max, self.nbin, self.nsub, self.nsubwin, self.nwidth,
                   self.d1, self.d2, self.gains)
        self._ctx_nprod = nprod
        self._nwindows = 0
        self._cands, self._oscs = [], []

    def _reset(self):
        self._bf.candfold_reset()
        self._nwindows = 0

    def _apply(self, cands, t, acc_len, tsamp):
        """The set that starts at the window of beamformer-clock sample t (the context's count stands on a segment boundary)."""
        half = self.nt * tsamp / 2
        oscs = []
        for c in cands:
            # (candfold_oscillators counts time from the start of a segment of nt windows whose middle the frequency belongs to)
            t0 = half + (t - c['seq_mid']) / float(acc_len) * tsamp if 'seq_mid' in c else half
            oscs += candfold_oscillators([c], t0, tsamp, self.nt)
        self._call('candfold_set_candidates', [o['pair'] * self.ndm + o['idm'] for o in oscs], [o['phi0'] for o in oscs], [o['dphi'] for o in oscs],
                   [o['ddphi'] for o in oscs], [1] * len(oscs))
        self._cands, self._oscs = cands, oscs
        self.update_stats({'ncand': len(cands)})

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(ncand=len(self._cands), ncand_max=self.ncand_max, nbin=self.nbin, nsub=self.nsub, nsubwin=self.nsubwin, nwidth=self.nwidth,
                    d1=self.d1.tolist(), d2=self.d2.tolist(), profile_offset=self.ncand_max * CANDFOLD_RECORD.itemsize,
                    candidates=[dict(c, f0=o['f0'], f1=o['f1']) for c, o in zip(self._cands, self._oscs)], threshold=self.threshold, seq0=start)
        return ohdr

    def _finish(self, osp, meta):
        """A span whose kernels (and copy) have completed: express it in sigma, publish; then commit the span."""
        try:
            threshold, oscs, sigma, tsamp, segment = meta
            rec, prof = as_records_candfold(osp.data.numpy().copy(), self.ncand_max, self.nbin)
            found = candfold_candidates(rec, prof, oscs, sigma, self.d1, self.d2, self.nbin, self.nt, tsamp, threshold, segment)
            pub = [dict((k, v) for k, v in c.items() if k != 'profile') for c in found]
            self.update_stats({'nfolded': self.stats['nfolded'] + len(found), 'folded': pub, 'nsegment_done': self.stats['nsegment_done'] + 1})
            if found and self.on_folded is not None:
                self.on_folded(found)
        finally:
            osp.close()

    def main(self):
        self.bind()
        ogulp_size = self.ncand_max * (CANDFOLD_RECORD.itemsize + 4 * self.nbin)
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        ospace = getattr(self.oring, 'space', 'system')
        direct = ospace in (self._bf.space_in, 'cuda_host')     # (the kernel can write the span itself)
        staged = spans_outlive_release(self.iring, self.oring) and ospace == 'cuda_host' and hasattr(self._bf, 'copy_async')
        streaming = spans_outlive_release(self.iring, self.oring) and (direct or staged)
        with InFlight(self._bf.candfold_wait, self._bf.candfold_sync, self._bf, finish=self._finish, mark=self._bf.candfold_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_CAND_FOLD", inflight, oring, streaming, staged, gap_note=": the segment starts again", count_gaps=False)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _load_pending_commands(self):
        cmds = self.take_commands(('threshold', 'candidates'))
        if 'threshold' in cmds:
            self.threshold = float(cmds['threshold'])
        if 'candidates' in cmds:
            self._waiting = self._checked(cmds['candidates'])

    def _sequence(self, iseq, loop, ogulp_size):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nprod, acc_len, S, dms, tsamp = check_dedispersed_header("BEAM_CAND_FOLD", ihdr, self.npair, self.ndm)
        loop.inflight.retire(0)
        if self._waiting is None and self._cands:
            self._waiting = self._cands         # (a new context or a reset count: the set starts again at the first window)
        if self._ctx_nprod != nprod:
            self._initialize(nprod)
        else:
            self._reset()
        seq0 = ihdr['seq0']
        state = {'first': None}                 # the beamformer-clock sample of the first window of the set in force

        def gap():
            # windows this reader never saw: the segment in progress does not line up with what comes now
            if self._nwindows % self.nt:
                self.update_stats({'ndropped': self.stats['ndropped'] + 1})
            self._reset()
            if self._waiting is None:
                self._waiting = self._cands     # (m = 0 again at the next window: the oscillators are made for it)

        def pending(t):
            if self.update_pending:
                self._load_pending_commands()
            if (t - seq0) // acc_len < S:
                self.update_stats({'nstartup': self.stats['nstartup'] + 1})
                return SKIP                     # (the span begins inside the dedisperser's partial sums)
            if self._waiting is not None and self._nwindows % self.nt == 0:
                loop.inflight.retire(0)         # (the setter waits for the stream: the spans in flight are finished first)
                had = bool(self._cands) and self._nwindows > 0
                cands, self._waiting = self._waiting, None
                self._apply(cands, t, acc_len, tsamp)
                state['first'] = t
                if had:
                    return RESTART              # (another list: the output goes on in a sequence of its own)
            if not self._cands:
                raise RuntimeError("BEAM_CAND_FOLD: no candidates (candidates= at construction, a `candidates` command or set_candidates())")

        def fold(t, held, out):
            # only the call that completes a segment reserves and writes an output span
            completes = (self._nwindows + self.nwin) // self.nt > self._nwindows // self.nt
            target = None
            if completes:
                segment = ((t - state['first']) // acc_len) // self.nt
                meta = [self.threshold, self._oscs, None, tsamp, segment]
                target = out.target(meta)
            rv, completed = self._bf.candfold_run(held, self.nwin, target)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("candfold_run returned %d: %s" % (rv, self._bf.last_error()))
            if bool(completed) != completes:
                raise RuntimeError("BEAM_CAND_FOLD: the context and the block disagree on which call completes a segment")
            if completes:
                meta[2] = candfold_sigma(*self._bf.candfold_cube(self.ncand_max, self.nsub, self.nbin))
            self._nwindows += self.nwin
            return {'nwindow': self.stats['nwindow'] + self.nwin}

        # (a span is nwin windows of acc_len samples of the beamformer's clock)
        loop.run(iseq, seq0, self.nwin * self.npair * self.ndm * nprod * 4, self.nwin * acc_len, ogulp_size, lambda t: self.output_header(ihdr, t),
                 fold, before=pending, on_gap=gap)
