"""UpchanGainCal: per-stand complex gains from the fine-channel visibilities, by StEFCal against a point-source sky model on the GPU.

Reads the output ring of UpchanCorr in device space: one span per integration,
  cf32 [nfine][nstand][npol = 2][nstand][npol]
and writes one output span per input span: the gains followed by the solver's statistics,
  cf32 [nfine][2][nstand]                 one gain per (fine channel, polarisation, stand), phase referenced to `refant`
  f32  [nfine][2][4]                      {iterations run, last delta, stands solved, converged 0/1}, `stats_offset` bytes in
(xengGaincal*, csrc/gaincal_kernels.h; the definition is in include/xeng.h).  The sky model is `nsrc` <= 32 point sources: their
directions `src_lmn` [nsrc][3] are fixed for the block's life, their fluxes `flux` [nsrc] or [nfine][nsrc] may change; `positions`
[nstand][3] are the stands' east-north-up coordinates in metres.  The model (steering_delays, the fine-channel frequencies from the
header's fine_sfreq / fine_bw_hz, the fluxes) is set per sequence.  A stand with weight 0 is not read at all, so a flagged input
may hold anything, and its gain is 0.  With warm_start every (channel, pol) starts from the solution of the integration before
where that one converged.  Only the parallel hands are solved: the X-Y phase stays undetermined.  What a caller does with the
gains is in calibration.py (apply_gains, inverse_gains).  No reference counterpart: the reference leaves calibration to offline
packages that read its visibility files.

A gap in the input (spans this reader never saw) loses those integrations, restarts the output in a sequence of its own so that
every span's time follows from its place, and forces a cold start.  set_weights(w), set_refant(s) and set_flux(F) (or the commands
`weights`, `refant` and `flux`) take effect at the next integration; each forgets the warm start.
"""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from .block_base import RESTART, Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .calibration import MAX_NSRC, MAX_NSTAND, checked_flux, model_flux
from .imaging import check_visibility_header, checked_weights, fine_frequencies, steering_delays

MAX_NITER = 1024        # include/xeng.h XENG_GAINCAL_MAX_NITER


class UpchanGainCal(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, positions, src_lmn, flux, weights=None, refant=0, niter=60, tol=1e-5, warm_start=True, guarantee=True,
                 core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanGainCal, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_GAINCAL"
        try:
            self.tau = steering_delays(positions, src_lmn)  # [nsrc][nstand]
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        self.nsrc, self.nstand = self.tau.shape
        if self.nsrc > MAX_NSRC or self.nstand > MAX_NSTAND:
            raise ValueError("%s: %d sources and %d stands, %d and %d at the most" % (who, self.nsrc, self.nstand, MAX_NSRC, MAX_NSTAND))
        if isinstance(niter, bool) or not isinstance(niter, (int, np.integer)) or not 0 <= niter <= MAX_NITER:
            raise ValueError("%s: niter %r is not an integer in [0, %d]" % (who, niter, MAX_NITER))
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating)) or not np.isfinite(tol) or tol < 0:
            raise ValueError("%s: tol %r is not a finite number >= 0" % (who, tol))
        self.niter, self.tol, self.warm_start, self.gpu = int(niter), float(tol), bool(warm_start), gpu
        self._nfine = None                      # of the sequence being read
        self._flux = self._checked_flux(flux)               # [nsrc] or [nfine][nsrc], float64
        self._weights = self._checked_weights(np.ones(self.nstand, np.float32) if weights is None else weights)
        self._refant = self._checked_refant(refant, self._weights)
        self._next = {}                         # set_weights / set_refant / set_flux: what the next integration takes
        self._next_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.define_command_key('refant', type=int, condition=lambda v: not isinstance(v, bool) and 0 <= v < self.nstand)
        self.define_command_key('flux', type=list, condition=lambda v: self._checked_flux(v, quiet=True) is not None)
        self.update_stats({'nsolve': 0, 'ngap': 0})
        self._ctx = None                        # (nstand, nfine) of the live context
        self._warm = False                      # the integration before this one was solved, in this output sequence

    def _checked_weights(self, w, quiet=False):
        """f32 [nstand], finite and >= 0; else ValueError, or None if `quiet`."""
        return checked_weights("UPCHAN_GAINCAL", w, self.nstand, quiet=quiet)

    def _checked_refant(self, refant, w):
        if isinstance(refant, bool) or not isinstance(refant, (int, np.integer)) or not 0 <= refant < self.nstand:
            raise ValueError("UPCHAN_GAINCAL: the reference stand %r is not one of %d" % (refant, self.nstand))
        if not w[refant] > 0:
            raise ValueError("UPCHAN_GAINCAL: the reference stand %d has weight 0" % refant)
        return int(refant)

    def _checked_flux(self, flux, quiet=False):
        """float64 [nsrc] or [nfine][nsrc], finite and >= 0 (nfine is checked against the sequence); else ValueError or None."""
        return checked_flux("UPCHAN_GAINCAL", flux, self.nsrc, self._nfine, quiet)

    def set_weights(self, w):
        """Per-stand weights from the next integration on (0: the stand is not read and its gain is 0)."""
        a = self._checked_weights(w)
        with self._next_lock:
            self._next['weights'] = a

    def set_refant(self, refant):
        """The reference stand from the next integration on (checked against the weights in force then)."""
        if isinstance(refant, bool) or not isinstance(refant, (int, np.integer)) or not 0 <= refant < self.nstand:
            raise ValueError("UPCHAN_GAINCAL: the reference stand %r is not one of %d" % (refant, self.nstand))
        with self._next_lock:
            self._next['refant'] = int(refant)

    def set_flux(self, flux):
        """The sources' fluxes, [nsrc] or [nfine][nsrc], from the next integration on."""
        F = self._checked_flux(flux)
        with self._next_lock:
            self._next['flux'] = F

    def _check_header(self, ihdr):
        """UpchanCorr's output only; returns (nfine, acc_len)."""
        who = "UPCHAN_GAINCAL"
        nfine, acc_len = check_visibility_header(who, ihdr, self.nstand, reject=('npix', 'nsrc'))
        if self._flux.ndim == 2 and self._flux.shape[0] != nfine:
            raise ValueError("%s: fluxes for %d fine channels, the header's nfine is %d" % (who, self._flux.shape[0], nfine))
        return nfine, acc_len

    def output_header(self, ihdr, start, nfine):
        ohdr = ihdr.copy()
        ohdr.update(nsrc=self.nsrc, refant=self._refant, niter=self.niter, tol=self.tol, stats_offset=nfine * 2 * self.nstand * 8, nbit=32, complex=True,
                    seq0=start)
        return ohdr

    def _set_model(self, ihdr, nfine):
        self._call('gaincal_set_model', self.tau, fine_frequencies(ihdr, nfine), np.ascontiguousarray(model_flux(self._flux, nfine, self.nsrc), np.float32))

    def _set_weights(self):
        self._call('gaincal_set_weights', self._weights, self._refant)

    def _load_pending(self, ihdr, nfine):
        """set_* or a command: on the device before the next integration is enqueued (SetWeights and SetModel wait for the
        integrations in flight, so each of those keeps what it was enqueued with).  Returns (something was set, so the next
        integration starts cold; the reference stand changed)."""
        with self._next_lock:
            nxt, self._next = self._next, {}
        if self.update_pending:
            nxt.update(self.take_commands(('weights', 'refant', 'flux')))
        w = self._checked_weights(nxt['weights']) if 'weights' in nxt else self._weights
        ref = nxt.get('refant', self._refant)
        changed = ref != self._refant
        applied = False
        if 'weights' in nxt or 'refant' in nxt:
            try:
                ref = self._checked_refant(ref, w)
            except ValueError as e:
                self.log.warning("%s: the weights and the reference stand stay as they were" % e)
                changed = False
            else:
                self._weights, self._refant = w, ref
                self._set_weights()
                applied = True
        if 'flux' in nxt:
            F = self._checked_flux(nxt['flux'], quiet=True)
            if F is None:
                self.log.warning("UPCHAN_GAINCAL: the fluxes are not [%d] or [%d][%d] finite numbers >= 0: they stay as they were" % (self.nsrc, nfine, self.nsrc))
            else:
                self._flux = F
                self._set_model(ihdr, nfine)
                applied = True
        return applied, changed

    def main(self):
        self.bind()
        # Streaming and tickets: InFlight, the loop over the spans: SpanLoop (block_base.py).  The output size follows the header's
        # nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.gaincal_wait, self._bf.gaincal_sync, mark=self._bf.gaincal_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_GAINCAL", inflight, oring, streaming)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop)

    def _sequence(self, iseq, loop):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, acc_len = self._check_header(ihdr)
        loop.inflight.retire(0)
        if self._ctx != (self.nstand, nfine):
            self._call('gaincal_initialize', self.gpu, self.nstand, nfine, self.nsrc)
            self._ctx = (self.nstand, nfine)
            self._call('gaincal_set_solver', self.niter, self.tol)
            self._set_weights()
        self._nfine = nfine
        self._set_model(ihdr, nfine)            # (forgets the warm start: a new sequence starts cold)
        self._warm = False
        stats_offset = nfine * 2 * self.nstand * 8
        ogulp_size = stats_offset + nfine * 2 * 4 * 4
        self.oring.resize(ogulp_size)

        def gap():
            self._warm = False                  # (the kept solution is older than one integration: the next one starts cold)

        def pending(t):
            if self.update_pending or self._next:
                applied, new_ref = self._load_pending(ihdr, nfine)
                if applied:
                    self._warm = False          # (SetWeights and SetModel have forgotten the kept solution)
                if new_ref:
                    return RESTART              # the header names the reference stand: a sequence of its own from here

        def solve(t, held, out):
            self._call('gaincal_run', held, out.target(), stats_offset, self.warm_start and self._warm)
            self._warm = True
            return {'nsolve': self.stats['nsolve'] + 1}

        loop.run(iseq, ihdr['seq0'], nfine * (2 * self.nstand) ** 2 * 8, acc_len, ogulp_size, lambda t: self.output_header(ihdr, t, nfine), solve,
                 before=pending, on_gap=gap)
