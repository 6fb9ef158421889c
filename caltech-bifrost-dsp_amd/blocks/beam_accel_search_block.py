"""BeamAccelSearch: acceleration search of the dedispersed beams over segments of 2^15 to 2^20 windows.

BeamPeriodSearchLong without stacks and with trial accelerations: xengAccel* (csrc/accel_kernels.h; the definition is in
include/xeng.h, "Acceleration search of the long-segment spectra") in the place of xengPlong*.  It reads the same spans,
  f32 [nwin][npair][ndm][nprod]        (nprod = 1: I; nprod = 4: I = XX + YY is formed from the first two words)
and writes one record plane per completed SEGMENT to a host-space output ring,
  [npair][ndm][nlevel][nband] x {f32 H, i32 k, i32 ia, f32 H0}      (blocks/accel_search.py ACCEL_RECORD)
per series, harmonic level and band of fundamental frequency the largest harmonic sum over all trials, the bin of its top
harmonic, the trial it was found in and what the unaccelerated trial found.  The trials are `alphas` (the coefficients of the index
map, accel_search.accel_alpha; at most 256, |alpha| * nt <= 0.5), or, with amax= and fmax=, accel_trials(amax, tsamp, nt, fmax,
zstep) made from the `tsamp` of the first sequence's header.  A completed plane is thresholded and grouped over DM
(accel_candidates) and, with sift = True, sifted (period_sift); every candidate carries ia, accel, H0 and z.

Everything else is BeamPeriodSearch's and is inherited unchanged: the header checks, the skip of the dedisperser's first
dedisp_latency windows, the reset on a new sequence or a gap, the `threshold` and `mask` commands, the stats (a "stack" is one
segment here).  The output header carries `ntrial`, `alpha`, `accel` (m/s^2), `nband` and `kedge` beside nt, nlevel and nwhite (and nstack = 1).

Not built: jerk trials, a Fourier-domain (correlation) search, interpolating resampling, stacking of segments."""
import json

import numpy as np

from ..backend import default_backend
from .accel_search import ACCEL_RECORD, MAX_TRIALS, accel_candidates, accel_of, accel_trials, as_records_accel
from .beam_dedisperse_block import _number
from .beam_period_search_block import BeamPeriodSearch, _ranges
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .period_search import period_bands, period_sift


class _AsPeriod:
    """The backend as BeamPeriodSearch calls it: period_<x> is accel_<x>, everything else the backend's own."""

    def __init__(self, backend):
        self._backend = backend

    def __getattr__(self, name):
        return getattr(self._backend, "accel_" + name[7:] if name.startswith("period_") else name)


class BeamAccelSearch(BeamPeriodSearch):
    def __init__(self, log, iring, oring, npair, ndm, nwin, nt, alphas=None, amax=None, fmax=None, zstep=1.0, nlevel=5, nwhite=64, kmin=2, nband=8,
                 kedge=None, threshold=6.0, sift=True, on_candidates=None, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        Block.__init__(self, log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_ACCEL_SEARCH"
        if min(npair, ndm, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r ndm=%r nwin=%r must be positive" % (who, npair, ndm, nwin))
        if not isinstance(nt, int) or not 1 << 15 <= nt <= 1 << 20 or nt & (nt - 1):
            raise ValueError("%s: nt %r is not a power of two from 2^15 to 2^20" % (who, nt))
        if nwin > nt:
            raise ValueError("%s: spans of %r windows are longer than a segment of %d" % (who, nwin, nt))
        if not 1 <= nlevel <= 5:
            raise ValueError("%s: nlevel %r not 1 to 5" % (who, nlevel))
        if not isinstance(nwhite, int) or not 8 <= nwhite <= 1 << 13 or nwhite & (nwhite - 1):
            raise ValueError("%s: nwhite %r is not a power of two from 8 to 2^13" % (who, nwhite))
        if kedge is None:
            kedge = period_bands(nt, nband, kmin)
        kedge = [int(k) for k in kedge]
        if not 2 <= len(kedge) <= 33 or not 1 <= kedge[0] < nt // 32 or kedge[-1] > nt // 2 or any(b <= a for a, b in zip(kedge, kedge[1:])):
            raise ValueError("%s: kedge %r is not 2 to 33 strictly ascending bins from 1 .. nt/32 - 1 up to nt/2 at most" % (who, kedge))
        if (alphas is None) == (amax is None):
            raise ValueError("%s: give the trials as alphas=, or amax= and fmax= for accel_trials" % who)
        if alphas is not None:
            alphas = np.array(alphas, np.float64).reshape(-1)
            if not 1 <= alphas.size <= MAX_TRIALS or not np.isfinite(alphas).all() or np.abs(alphas).max() * nt > 0.5:
                raise ValueError("%s: alphas are not 1 to %d finite numbers with |alpha| * nt <= 0.5" % (who, MAX_TRIALS))
        elif not (_number(amax) and amax >= 0 and _number(fmax) and fmax > 0 and _number(zstep) and zstep > 0):
            raise ValueError("%s: amax %r, fmax %r and zstep %r are not a range of accelerations, a top frequency and a step in bins" % (who, amax, fmax, zstep))
        if not _number(threshold):
            raise ValueError("%s: threshold %r is not a finite number" % (who, threshold))
        if on_candidates is not None and not callable(on_candidates):
            raise ValueError("%s: on_candidates is not callable" % who)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the record planes go to a host-space ring" % (who, oring.space))
        self.npair, self.ndm, self.nwin, self.gpu = npair, ndm, nwin, gpu
        self.nt, self.nstack, self.nlevel, self.nwhite = nt, 1, nlevel, nwhite
        self.kedge, self.nband, self.kmin, self.sift = kedge, len(kedge) - 1, kedge[0], bool(sift)
        self.alphas, self._trial_spec = alphas, (amax, fmax, zstep)
        self.threshold = float(threshold)
        self.on_candidates = on_candidates
        self._bf = _AsPeriod(backend if backend is not None else default_backend())
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('threshold', type=(int, float), condition=_number)
        self.define_command_key('mask', type=list, condition=_ranges)
        self.update_stats({'nwindow': 0, 'nstack_done': 0, 'ndropped': 0, 'ncand': 0, 'nstartup': 0, 'candidates': [], 'threshold': self.threshold})
        self._ctx_nprod = None                  # nprod of the live context
        self._ctx_alphas = None                 # the trials of the live context
        self._mask = None                       # the ranges in force (None: all kept)
        self._nwindows = 0                      # windows given to the context since its last reset

    def _trials(self, tsamp):
        """The trial table at the window length of the sequence that begins."""
        if self.alphas is not None:
            return self.alphas
        amax, fmax, zstep = self._trial_spec
        return accel_trials(amax, tsamp, self.nt, fmax, zstep)

    def _initialize(self, nprod):
        self._call('period_initialize', self.gpu, self.npair, self.ndm, self.nwin, nprod, self.nt, self.nlevel, self.nwhite, self.kedge, self._ctx_alphas)
        self._ctx_nprod = nprod
        self._nwindows = 0
        if self._mask:
            self._set_mask(self._mask)          # (a new context keeps everything)

    def _sequence(self, iseq, loop, ogulp_size):
        # the trials depend on the header's tsamp when they were given as a range of accelerations: a sequence with another
        # window length gets a context of its own
        tsamp = json.loads(iseq.header.tostring()).get('tsamp')
        if _number(tsamp) and tsamp > 0:
            alphas = self._trials(float(tsamp))
            if self._ctx_alphas is None or alphas.tobytes() != self._ctx_alphas.tobytes():
                loop.inflight.retire(0)
                self._ctx_alphas, self._ctx_nprod = alphas, None
        BeamPeriodSearch._sequence(self, iseq, loop, ogulp_size)

    def output_header(self, ihdr, start):
        ohdr = BeamPeriodSearch.output_header(self, ihdr, start)
        ohdr.update(nband=self.nband, kedge=list(self.kedge), ntrial=int(self._ctx_alphas.size), alpha=[float(a) for a in self._ctx_alphas],
                    accel=[float(a) for a in accel_of(self._ctx_alphas, ihdr['tsamp'])])
        return ohdr

    def _finish(self, osp, meta):
        """A plane whose kernels (and copy) have completed: threshold it, group it over DM, sift it, publish; then commit the span."""
        try:
            threshold, dms, tsamp = meta
            plane = as_records_accel(osp.data.numpy().copy(), self.npair, self.ndm, self.nlevel, self.nband)
            cands = accel_candidates(plane, threshold, dms, self.nt, tsamp, self.kedge, self._ctx_alphas)
            if self.sift:
                cands = period_sift(cands, self.nt)
            self.update_stats({'ncand': self.stats['ncand'] + len(cands), 'candidates': cands, 'nstack_done': self.stats['nstack_done'] + 1})
            if cands and self.on_candidates is not None:
                self.on_candidates(cands)
        finally:
            osp.close()

    def main(self):
        self.bind()
        ogulp_size = self.npair * self.ndm * self.nlevel * self.nband * ACCEL_RECORD.itemsize
        self.oring.resize(ogulp_size)
        ospace = getattr(self.oring, 'space', 'system')
        direct = ospace in (self._bf.space_in, 'cuda_host')     # (the kernel can write the span itself)
        staged = spans_outlive_release(self.iring, self.oring) and ospace == 'cuda_host' and hasattr(self._bf, 'copy_async')
        streaming = spans_outlive_release(self.iring, self.oring) and (direct or staged)
        with InFlight(self._bf.period_wait, self._bf.period_sync, self._bf, finish=self._finish, mark=self._bf.period_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_ACCEL_SEARCH", inflight, oring, streaming, staged, gap_note=": the segment starts again", count_gaps=False)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)
