"""UpchanPeel: direction-dependent gains for a few bright sources, solved per integration, and those sources taken out of the
fine-channel visibilities with their own gains (peeling), on the GPU.

Reads a ring of UpchanCorr's format in device space -- normally UpchanCalApply's output -- one span per integration,
  cf32 [nfine][nstand][npol = 2][nstand][npol]
and writes one output span per input span, of the same size and format:
  out[c][s p][t p] = V[c][s p][t p] - sum_d F_d u_ds conj(u_dt),   u_ds = g_ds a_ds;   the cross hands are copied
Hermitian bit for bit (xengPeel*, csrc/peel_kernels.h; the definition is in include/xeng.h), so UpchanImage, UpchanGainCal and a
further UpchanCalApply read it unchanged.  g [nfine][2][ndir][nstand] is one complex gain per (fine channel, polarisation,
direction, stand), solved from the span itself by StEFCal steps that visit the directions in the order given, each against the
others' newest gains: list the brightest source first; nothing is sorted.  The sky model is `ndir` <= 8 point sources: their
directions `src_lmn` [ndir][3] are fixed for the block's life, their fluxes `flux` [ndir] or [nfine][ndir] may change (a flux of
0 switches a direction off); `positions` [nstand][3] are the stands' east-north-up coordinates in metres.  A stand with weight 0 is
not read by the solve, its gains are 0 and its rows and columns pass through unchanged.

The iteration starts from g = 1 (or, with warm_start, from the integration before where that one converged): it converges for the
gains that are left behind a calibration -- amplitudes within some 20 % of 1, phases of half a radian -- and DIVERGES for gains of
arbitrary phase.  Uncalibrated input is accepted (the header need not say `calibrated`) but only makes sense where the instrument's
gains are already near 1: the block belongs behind UpchanCalApply.  No reference counterpart: the reference leaves calibration and
source subtraction to offline packages.

The ring carries visibilities only.  The gains and the solver's statistics of each finished integration are copied to the host and
offered by solution() -> (seq, gains complex64 [nfine][2][ndir][nstand], stats float32 [nfine][2][4] = {sweeps, last delta, stands
solved, converged}) of the newest one, or None before the first.  The output header is the input's plus `npeeled` = ndir and
`nsubtracted`, the input's count plus ndir.

A gap in the input (spans this reader never saw) loses those integrations, restarts the output in a sequence of its own so that
every span's time follows from its place, and forces a cold start.  set_flux(F), set_weights(w), set_refant(s) (or the commands
`flux`, `weights`, `refant`) take effect at the next integration; each forgets the warm start.  Not built: the gains on a second
ring, sorting or choosing the directions, cross-hand terms, smoothing of the gains over time or frequency, extended sources.
"""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .calibration import MAX_NDIR, MAX_NSTAND, checked_flux, model_flux
from .imaging import check_visibility_header, checked_weights, fine_frequencies, steering_delays

MAX_NITER = 1024        # include/xeng.h XENG_PEEL_MAX_NITER


class UpchanPeel(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, positions, src_lmn, flux, weights=None, refant=0, niter=60, tol=1e-5, warm_start=True, guarantee=True,
                 core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanPeel, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_PEEL"
        try:
            self.tau = steering_delays(positions, src_lmn)  # [ndir][nstand]
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        self.ndir, self.nstand = self.tau.shape
        if self.ndir > MAX_NDIR or self.nstand > MAX_NSTAND:
            raise ValueError("%s: %d directions and %d stands, %d and %d at the most" % (who, self.ndir, self.nstand, MAX_NDIR, MAX_NSTAND))
        if isinstance(niter, bool) or not isinstance(niter, (int, np.integer)) or not 0 <= niter <= MAX_NITER:
            raise ValueError("%s: niter %r is not an integer in [0, %d]" % (who, niter, MAX_NITER))
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating)) or not np.isfinite(tol) or tol < 0:
            raise ValueError("%s: tol %r is not a finite number >= 0" % (who, tol))
        self.niter, self.tol, self.warm_start, self.gpu = int(niter), float(tol), bool(warm_start), gpu
        self._nfine = None                      # of the sequence being read
        self._flux = self._checked_flux(flux)               # [ndir] or [nfine][ndir], float64
        self._weights = self._checked_weights(np.ones(self.nstand, np.float32) if weights is None else weights)
        self._refant = self._checked_refant(refant, self._weights)
        self._next = {}                         # set_weights / set_refant / set_flux: what the next integration takes
        self._next_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.define_command_key('refant', type=int, condition=lambda v: not isinstance(v, bool) and 0 <= v < self.nstand)
        self.define_command_key('flux', type=list, condition=lambda v: self._checked_flux(v, quiet=True) is not None)
        self.update_stats({'npeel': 0, 'ngap': 0})
        self._ctx = None                        # (nstand, nfine) of the live context
        self._warm = False                      # the integration before this one was solved, in this output sequence
        self._solution = None                   # (seq, gains, stats) of the newest finished integration
        self._solution_lock = Lock()
        self._sol_pool = []                     # device buffers for the gains and stats of a call

    def _checked_weights(self, w, quiet=False):
        """f32 [nstand], finite and >= 0; else ValueError, or None if `quiet`."""
        return checked_weights("UPCHAN_PEEL", w, self.nstand, quiet=quiet)

    def _checked_refant(self, refant, w):
        if isinstance(refant, bool) or not isinstance(refant, (int, np.integer)) or not 0 <= refant < self.nstand:
            raise ValueError("UPCHAN_PEEL: the reference stand %r is not one of %d" % (refant, self.nstand))
        if not w[refant] > 0:
            raise ValueError("UPCHAN_PEEL: the reference stand %d has weight 0" % refant)
        return int(refant)

    def _checked_flux(self, flux, quiet=False):
        """float64 [ndir] or [nfine][ndir], finite and >= 0 (nfine is checked against the sequence); else ValueError or None."""
        return checked_flux("UPCHAN_PEEL", flux, self.ndir, self._nfine, quiet)

    def set_weights(self, w):
        """Per-stand weights from the next integration on (0: the stand is not read by the solve and its gains are 0)."""
        a = self._checked_weights(w)
        with self._next_lock:
            self._next['weights'] = a

    def set_refant(self, refant):
        """The reference stand from the next integration on (checked against the weights in force then)."""
        if isinstance(refant, bool) or not isinstance(refant, (int, np.integer)) or not 0 <= refant < self.nstand:
            raise ValueError("UPCHAN_PEEL: the reference stand %r is not one of %d" % (refant, self.nstand))
        with self._next_lock:
            self._next['refant'] = int(refant)

    def set_flux(self, flux):
        """The sources' fluxes, [ndir] or [nfine][ndir], from the next integration on (0: the direction is off)."""
        F = self._checked_flux(flux)
        with self._next_lock:
            self._next['flux'] = F

    def solution(self):
        """(seq, gains complex64 [nfine][2][ndir][nstand], stats float32 [nfine][2][4]) of the newest finished integration -- seq is
        its first sample -- or None before the first."""
        with self._solution_lock:
            return self._solution

    def _check_header(self, ihdr):
        """UpchanCorr's output, calibrated or not; returns (nfine, acc_len)."""
        who = "UPCHAN_PEEL"
        nfine, acc_len = check_visibility_header(who, ihdr, self.nstand, reject=('npix', 'nsrc'))
        if self._flux.ndim == 2 and self._flux.shape[0] != nfine:
            raise ValueError("%s: fluxes for %d fine channels, the header's nfine is %d" % (who, self._flux.shape[0], nfine))
        nsub = ihdr.get('nsubtracted', 0)
        if not isinstance(nsub, int) or isinstance(nsub, bool) or nsub < 0:
            raise ValueError("%s: the header's 'nsubtracted' is %r" % (who, nsub))
        return nfine, acc_len

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(npeeled=self.ndir, nsubtracted=ihdr.get('nsubtracted', 0) + self.ndir, nbit=32, complex=True, seq0=start)
        return ohdr

    def _set_model(self, ihdr, nfine):
        self._call('peel_set_model', self.tau, fine_frequencies(ihdr, nfine), np.ascontiguousarray(model_flux(self._flux, nfine, self.ndir), np.float32))

    def _set_weights(self):
        self._call('peel_set_weights', self._weights, self._refant)

    def _load_pending(self, ihdr, nfine):
        """set_* or a command: on the device before the next integration is enqueued (SetWeights and SetModel wait for the
        integrations in flight, so each of those keeps what it was enqueued with).  Returns whether something was set, so that the
        next integration starts cold."""
        with self._next_lock:
            nxt, self._next = self._next, {}
        if self.update_pending:
            nxt.update(self.take_commands(('weights', 'refant', 'flux')))
        applied = False
        if 'weights' in nxt or 'refant' in nxt:
            w = self._checked_weights(nxt['weights']) if 'weights' in nxt else self._weights
            try:
                ref = self._checked_refant(nxt.get('refant', self._refant), w)
            except ValueError as e:
                self.log.warning("%s: the weights and the reference stand stay as they were" % e)
            else:
                self._weights, self._refant = w, ref
                self._set_weights()
                applied = True
        if 'flux' in nxt:
            F = self._checked_flux(nxt['flux'], quiet=True)
            if F is None:
                self.log.warning("UPCHAN_PEEL: the fluxes are not [%d] or [%d][%d] finite numbers >= 0: they stay as they were" % (self.ndir, nfine, self.ndir))
            else:
                self._flux = F
                self._set_model(ihdr, nfine)
                applied = True
        return applied

    def _finish(self, ospan, meta):
        """A call's kernels have completed: its gains and stats go to the host, then its span is committed."""
        try:
            if meta is not None:
                t, sol, nfine = meta
                raw = np.array(sol.numpy(), copy=True).reshape(-1)
                self._sol_pool.append(sol)
                ngain = nfine * 2 * self.ndir * self.nstand * 8
                with self._solution_lock:
                    self._solution = (t, raw[:ngain].view(np.complex64).reshape(nfine, 2, self.ndir, self.nstand), raw[ngain:].view(np.float32).reshape(nfine, 2, 4))
        finally:
            ospan.close()

    def main(self):
        self.bind()
        # Streaming and tickets: InFlight, the loop over the spans: SpanLoop (block_base.py).  The span size follows the header's
        # nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.peel_wait, self._bf.peel_sync, finish=self._finish, mark=self._bf.peel_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_PEEL", inflight, oring, streaming)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop)

    def _sequence(self, iseq, loop):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, acc_len = self._check_header(ihdr)
        loop.inflight.retire(0)
        if self._ctx != (self.nstand, nfine):
            self._call('peel_initialize', self.gpu, self.nstand, nfine, self.ndir)
            self._ctx = (self.nstand, nfine)
            self._call('peel_set_solver', self.niter, self.tol)
            self._set_weights()
            self._sol_pool = []
        self._nfine = nfine
        self._set_model(ihdr, nfine)            # (forgets the warm start: a new sequence starts cold)
        self._warm = False
        gulp_size = nfine * (2 * self.nstand) ** 2 * 8
        stats_offset = nfine * 2 * self.ndir * self.nstand * 8
        sol_size = stats_offset + nfine * 2 * 4 * 4
        self.oring.resize(gulp_size)

        def gap():
            self._warm = False                  # (the kept solution is older than one integration: the next one starts cold)

        def pending(t):
            if (self.update_pending or self._next) and self._load_pending(ihdr, nfine):
                self._warm = False              # (SetWeights and SetModel have forgotten the kept solution)

        def peel(t, held, out):
            sol = self._sol_pool.pop() if self._sol_pool else XArray(shape=(sol_size,), dtype=np.uint8, space=self._bf.space_in)
            self._call('peel_run', held, out.target((t, sol, nfine)), sol, stats_offset, self.warm_start and self._warm)
            self._warm = True
            return {'npeel': self.stats['npeel'] + 1}

        loop.run(iseq, ihdr['seq0'], gulp_size, acc_len, gulp_size, lambda t: self.output_header(ihdr, t), peel, before=pending, on_gap=gap)
