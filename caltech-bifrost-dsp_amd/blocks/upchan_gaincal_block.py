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
import time
from threading import Lock

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray
from .block_base import Block, InFlight, declare_streams, gulp_time, spans_outlive_release
from .calibration import model_flux
from .imaging import steering_delays

MAX_NSRC, MAX_NSTAND, MAX_NITER = 32, 512, 1024        # include/xeng.h XENG_GAINCAL_MAX_*


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
        self._nfine = None

    def _checked_weights(self, w, quiet=False):
        """f32 [nstand], finite and >= 0; else ValueError, or None if `quiet`."""
        try:
            a = np.ascontiguousarray(w, np.float32).reshape(-1)
            ok = a.size == self.nstand and bool(np.all(np.isfinite(a))) and bool(a.min() >= 0)
        except (TypeError, ValueError):
            a, ok = None, False
        if ok:
            return a
        if quiet:
            return None
        raise ValueError("UPCHAN_GAINCAL: the weights must be %d finite numbers >= 0" % self.nstand)

    def _checked_refant(self, refant, w):
        if isinstance(refant, bool) or not isinstance(refant, (int, np.integer)) or not 0 <= refant < self.nstand:
            raise ValueError("UPCHAN_GAINCAL: the reference stand %r is not one of %d" % (refant, self.nstand))
        if not w[refant] > 0:
            raise ValueError("UPCHAN_GAINCAL: the reference stand %d has weight 0" % refant)
        return int(refant)

    def _checked_flux(self, flux, quiet=False):
        """float64 [nsrc] or [nfine][nsrc], finite and >= 0 (nfine is checked against the sequence); else ValueError or None."""
        try:
            F = np.asarray(flux, np.float64)
            ok = F.ndim in (1, 2) and F.shape[-1] == self.nsrc and F.size > 0 and bool(np.all(np.isfinite(F))) and bool(F.min() >= 0)
            if ok and F.ndim == 2 and getattr(self, '_nfine', None) is not None:
                ok = F.shape[0] == self._nfine
        except (TypeError, ValueError):
            F, ok = None, False
        if ok:
            return F
        if quiet:
            return None
        raise ValueError("UPCHAN_GAINCAL: the fluxes must be [%d] or [nfine][%d] finite numbers >= 0" % (self.nsrc, self.nsrc))

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
        if ihdr.get('npol') != 2:
            raise ValueError("%s: npol %r in the header: dual-polarisation visibilities only" % (who, ihdr.get('npol')))
        if ihdr.get('nstand') != self.nstand:
            raise ValueError("%s: %r stands in the header, positions for %d" % (who, ihdr.get('nstand'), self.nstand))
        if ihdr.get('nbit') != 32 or not ihdr.get('complex'):
            raise ValueError("%s: the input is not cf32 visibilities (nbit %r, complex %r)" % (who, ihdr.get('nbit'), ihdr.get('complex')))
        if 'npix' in ihdr or 'nsrc' in ihdr:
            raise ValueError("%s: the input carries 'npix' or 'nsrc': it is an image or a gain solution, not visibilities" % who)
        nfine = ihdr.get('nfine')
        if not isinstance(nfine, int) or isinstance(nfine, bool) or nfine <= 0:
            raise ValueError("%s: the header's 'nfine' is %r: not UpchanCorr's visibilities" % (who, nfine))
        if self._flux.ndim == 2 and self._flux.shape[0] != nfine:
            raise ValueError("%s: fluxes for %d fine channels, the header's nfine is %d" % (who, self._flux.shape[0], nfine))
        for k in ('fine_sfreq', 'fine_bw_hz'):
            v = ihdr.get(k)
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not np.isfinite(v) or (k == 'fine_bw_hz' and not v > 0):
                raise ValueError("%s: the header's '%s' is %r" % (who, k, v))
        acc_len = ihdr.get('acc_len', 1)
        if not isinstance(acc_len, int) or isinstance(acc_len, bool) or acc_len <= 0:
            raise ValueError("%s: the header's 'acc_len' is %r" % (who, acc_len))
        return nfine, acc_len

    def frequencies(self, ihdr, nfine):
        """The fine channels' centre frequencies of a sequence, float64 [nfine] Hz."""
        return np.ascontiguousarray(ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * np.arange(nfine, dtype=np.float64))

    def output_header(self, ihdr, start, nfine):
        ohdr = ihdr.copy()
        ohdr.update(nsrc=self.nsrc, refant=self._refant, niter=self.niter, tol=self.tol, stats_offset=nfine * 2 * self.nstand * 8, nbit=32, complex=True,
                    seq0=start)
        return ohdr

    def _set_model(self, ihdr, nfine):
        self._call('gaincal_set_model', self.tau, self.frequencies(ihdr, nfine), np.ascontiguousarray(model_flux(self._flux, nfine, self.nsrc), np.float32))

    def _set_weights(self):
        self._call('gaincal_set_weights', self._weights, self._refant)

    def _load_pending(self, ihdr, nfine):
        """set_* or a command: on the device before the next integration is enqueued (SetWeights and SetModel wait for the
        integrations in flight, so each of those keeps what it was enqueued with).  Returns (something was set, so the next
        integration starts cold; the reference stand changed)."""
        with self._next_lock:
            nxt, self._next = self._next, {}
        if self.update_pending:
            self.update_command_vals()
            with self._control_lock:
                # a command is taken once: left in place, a later command for another key would bring it back over a set_*() since
                for k in ('weights', 'refant', 'flux'):
                    cmd = self.command_vals.get(k)
                    if cmd is not None:
                        nxt[k] = cmd
                        self.command_vals[k] = None
                        if self._pending_command_vals.get(k) is cmd:
                            self._pending_command_vals[k] = None
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
        # Streaming and tickets: InFlight (block_base.py).  The output size follows the header's nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.gaincal_wait, self._bf.gaincal_sync) as inflight, self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, oring, streaming, inflight)

    def _sequence(self, iseq, oring, streaming, inflight):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, acc_len = self._check_header(ihdr)
        inflight.retire(0)
        if self._ctx != (self.nstand, nfine):
            self._call('gaincal_initialize', self.gpu, self.nstand, nfine, self.nsrc)
            self._ctx = (self.nstand, nfine)
            self._call('gaincal_set_solver', self.niter, self.tol)
            self._set_weights()
        self._nfine = nfine
        self._set_model(ihdr, nfine)            # (forgets the warm start: a new sequence starts cold)
        stats_offset = nfine * 2 * self.nstand * 8
        ogulp_size = stats_offset + nfine * 2 * 4 * 4
        self.oring.resize(ogulp_size)
        dev = None if streaming else XArray(shape=(ogulp_size,), dtype=np.uint8, space=self._bf.space_in)
        seq0 = ihdr['seq0']
        igulp_size = nfine * (2 * self.nstand) ** 2 * 8
        this_gulp_time = seq0
        expected = seq0
        oseq = None
        warm = False                            # the integration before this one was solved, in this output sequence
        try:
            prev_time = time.time()
            for ispan in iseq.read(igulp_size):
                if ispan.size < igulp_size:
                    continue                    # a short final span is skipped (as the reference's gulp_nframe reader does)
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, acc_len, this_gulp_time)
                if this_gulp_time != expected:
                    # integrations this reader never saw: the kept solution is older than one integration, so the next one starts cold
                    self.update_stats({'ngap': self.stats['ngap'] + 1})
                    self.log.warning("UPCHAN_GAINCAL >> samples [%d, %d) were not read" % (expected, this_gulp_time))
                    warm = False
                    if oseq is not None:
                        inflight.retire(0)
                        oseq.end()
                        oseq = None
                expected = this_gulp_time + acc_len
                self.update_stats({'curr_sample': this_gulp_time})
                if self.update_pending or self._next:
                    applied, new_ref = self._load_pending(ihdr, nfine)
                    if applied:
                        warm = False            # (SetWeights and SetModel have forgotten the kept solution)
                    if new_ref and oseq is not None:
                        inflight.retire(0)      # the header names the reference stand: a sequence of its own from here
                        oseq.end()
                        oseq = None
                held = ispan.data
                if oseq is None:
                    oseq = oring.begin_sequence(time_tag=this_gulp_time, header=json.dumps(self.output_header(ihdr, this_gulp_time, nfine)))
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                ospan = oseq.reserve(ogulp_size)
                try:
                    self._call('gaincal_run', held, ospan.data if streaming else dev, stats_offset, self.warm_start and warm)
                    warm = True
                    self.update_stats({'nsolve': self.stats['nsolve'] + 1, 'last_end_sample': this_gulp_time + acc_len})
                    osp, ospan = ospan, None
                    if streaming:
                        inflight.push(self._bf.gaincal_mark(), osp, held)
                        inflight.retire(self.STREAM_DEPTH)
                    else:
                        self._bf.gaincal_sync()
                        try:
                            osp.data_view(np.uint8).reshape(-1)[...] = dev               # (synchronous copy)
                        finally:
                            osp.close()
                finally:
                    if ospan is not None:
                        ospan.close()
                curr_time = time.time()
                process_time = curr_time - prev_time
                prev_time = curr_time
                self.perf_proclog.update({'acquire_time': acquire_time, 'reserve_time': 0.0, 'process_time': process_time})
        finally:
            inflight.retire(0)                  # every call in flight is complete (and every output span committed) first
            if oseq is not None:
                oseq.end()
