"""UpchanCalApply: calibrated, source-subtracted fine-channel visibilities -- a gain solution applied to UpchanCorr's matrix and a
point-source model taken out of it, on the GPU.

Reads the output ring of UpchanCorr in device space: one span per integration,
  cf32 [nfine][nstand][npol = 2][nstand][npol]
and writes one output span per input span, of the same size and format:
  out[c][s p][t q] = h_ps conj(h_qt) V[c][s p][t q] - delta_pq sum_k F_k a_ks conj(a_kt)
Hermitian bit for bit as UpchanCorr's own output is (xengCalapply*, csrc/calapply_kernels.h; the definition is in include/xeng.h),
so UpchanImage and a second UpchanGainCal (a residual solve) read it unchanged.  The apply factors h [nfine][2][nstand] are 1 / g of
a gain solution (calibration.py inverse_gains, float64 on the host, rounded once) and 0 where a (stand, polarisation) has none: such
rows and columns are not read and are written as zeros.  The sky model is `nsrc` <= 32 point sources: their directions `src_lmn`
[nsrc][3] are fixed for the block's life, their fluxes `flux` [nsrc] or [nfine][nsrc] may change; `positions` [nstand][3] are the
stands' east-north-up coordinates in metres.  Without `src_lmn` nothing is subtracted (calibration only); without `gains` every
factor is 1 (subtraction only).  The output header is the input's plus `calibrated` and `nsubtracted`, the input's count plus nsrc:
an input that is already calibrated is accepted, so a second pass can peel further sources.  No reference counterpart: the
reference leaves calibration to offline packages that read its visibility files.

A gap in the input (spans this reader never saw) loses those integrations and restarts the output in a sequence of its own so that
every span's time follows from its place.  set_gains(g), set_factors(h) and set_flux(F) (or the command `flux`) take effect at the
next integration.  Not built: gains arriving on a second ring, flux fitting per integration (the host solves the nsrc x nsrc system
from UpchanImage at the sources' directions and calls set_flux), direction-dependent gains, sources that move within the block's
life, cross-hand model terms.
"""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .calibration import MAX_NSRC, MAX_NSTAND, checked_flux, inverse_gains, model_flux
from .imaging import check_visibility_header, fine_frequencies, steering_delays


class UpchanCalApply(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, positions, src_lmn=None, flux=None, gains=None, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanCalApply, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_CALAPPLY"
        try:
            # (without sources the zenith stands in, so that the positions are checked all the same)
            tau = steering_delays(positions, [[0.0, 0.0, 1.0]] if src_lmn is None else src_lmn)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        self.tau = np.ascontiguousarray(tau[:0] if src_lmn is None else tau)      # [nsrc][nstand]
        self.nsrc, self.nstand = self.tau.shape
        if self.nsrc > MAX_NSRC or self.nstand > MAX_NSTAND:
            raise ValueError("%s: %d sources and %d stands, %d and %d at the most" % (who, self.nsrc, self.nstand, MAX_NSRC, MAX_NSTAND))
        self.gpu = gpu
        self._nfine = None
        if self.nsrc == 0 and flux is not None:
            raise ValueError("%s: fluxes without source directions" % who)
        self._flux = self._checked_flux(flux) if self.nsrc else np.zeros(0)       # [nsrc] or [nfine][nsrc], float64
        self._factors = None if gains is None else self._checked_factors(self._from_gains(gains))      # None: every factor is 1
        self._next = {}                         # set_gains / set_factors / set_flux: what the next integration takes
        self._next_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('flux', type=list, condition=lambda v: self._checked_flux(v, quiet=True) is not None)
        self.update_stats({'napply': 0, 'ngap': 0})
        self._ctx = None                        # (nstand, nfine) of the live context

    def _from_gains(self, g):
        try:
            g = np.asarray(g, np.complex128)
            if not np.all(np.isfinite(g)):
                raise ValueError("not finite")
            h = inverse_gains(g)                # [nfine][2 nstand], input 2 s + p
        except (TypeError, ValueError):
            raise ValueError("UPCHAN_CALAPPLY: the gains must be [nfine][2][%d] finite complex numbers" % self.nstand)
        return h.reshape(h.shape[0], -1, 2).transpose(0, 2, 1)

    def _checked_factors(self, h, quiet=False):
        """complex64 [nfine][2][nstand], finite (nfine is checked against the sequence); else ValueError, or None if `quiet`."""
        try:
            a = np.ascontiguousarray(np.asarray(h, np.complex128).astype(np.complex64))
            ok = a.ndim == 3 and a.shape[1:] == (2, self.nstand) and a.shape[0] > 0 and bool(np.all(np.isfinite(a.view(np.float32))))
            if ok and self._nfine is not None:
                ok = a.shape[0] == self._nfine
        except (TypeError, ValueError):
            a, ok = None, False
        if ok:
            return a
        if quiet:
            return None
        raise ValueError("UPCHAN_CALAPPLY: the factors must be [nfine][2][%d] finite complex numbers" % self.nstand)

    def _checked_flux(self, flux, quiet=False):
        """float64 [nsrc] or [nfine][nsrc], finite and >= 0 (nfine is checked against the sequence); else ValueError or None."""
        return checked_flux("UPCHAN_CALAPPLY", flux, self.nsrc, self._nfine, quiet)

    def set_gains(self, g):
        """A gain solution [nfine][2][nstand] (UpchanGainCal's output span) from the next integration on: the factors are
        inverse_gains(g), 0 where the gain is 0."""
        h = self._checked_factors(self._from_gains(g))
        with self._next_lock:
            self._next['factors'] = h

    def set_factors(self, h):
        """The apply factors [nfine][2][nstand] themselves from the next integration on (0: left out)."""
        h = self._checked_factors(h)
        with self._next_lock:
            self._next['factors'] = h

    def set_flux(self, flux):
        """The sources' fluxes, [nsrc] or [nfine][nsrc], from the next integration on."""
        F = self._checked_flux(flux)
        with self._next_lock:
            self._next['flux'] = F

    def _check_header(self, ihdr):
        """UpchanCorr's output, or this block's own; returns (nfine, acc_len)."""
        who = "UPCHAN_CALAPPLY"
        nfine, acc_len = check_visibility_header(who, ihdr, self.nstand, reject=('npix', 'nsrc'))
        if self._flux.ndim == 2 and self._flux.shape[0] != nfine:
            raise ValueError("%s: fluxes for %d fine channels, the header's nfine is %d" % (who, self._flux.shape[0], nfine))
        if self._factors is not None and self._factors.shape[0] != nfine:
            raise ValueError("%s: factors for %d fine channels, the header's nfine is %d" % (who, self._factors.shape[0], nfine))
        nsub = ihdr.get('nsubtracted', 0)
        if not isinstance(nsub, int) or isinstance(nsub, bool) or nsub < 0:
            raise ValueError("%s: the header's 'nsubtracted' is %r" % (who, nsub))
        return nfine, acc_len

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(calibrated=True, nsubtracted=ihdr.get('nsubtracted', 0) + self.nsrc, nbit=32, complex=True, seq0=start)
        return ohdr

    def _set_model(self, ihdr, nfine):
        if self.nsrc:
            self._call('calapply_set_model', self.tau, fine_frequencies(ihdr, nfine), np.ascontiguousarray(model_flux(self._flux, nfine, self.nsrc), np.float32))
        else:
            self._call('calapply_set_model', None, fine_frequencies(ihdr, nfine), None)

    def _set_factors(self, nfine):
        self._call('calapply_set_factors', self._factors if self._factors is not None else np.ones((nfine, 2, self.nstand), np.complex64))

    def _load_pending(self, ihdr, nfine):
        """set_* or a command: on the device before the next integration is enqueued (SetFactors and SetModel wait for the
        integrations in flight, so each of those keeps what it was enqueued with)."""
        with self._next_lock:
            nxt, self._next = self._next, {}
        if self.update_pending:
            nxt.update(self.take_commands(('flux',)))
        if 'factors' in nxt:
            h = self._checked_factors(nxt['factors'], quiet=True)
            if h is None:
                self.log.warning("UPCHAN_CALAPPLY: the factors are not [%d][2][%d] finite complex numbers: they stay as they were" % (nfine, self.nstand))
            else:
                self._factors = h
                self._set_factors(nfine)
        if 'flux' in nxt:
            F = self._checked_flux(nxt['flux'], quiet=True)
            if F is None:
                self.log.warning("UPCHAN_CALAPPLY: the fluxes are not [%d] or [%d][%d] finite numbers >= 0: they stay as they were" % (self.nsrc, nfine, self.nsrc))
            else:
                self._flux = F
                self._set_model(ihdr, nfine)

    def main(self):
        self.bind()
        # Streaming and tickets: InFlight, the loop over the spans: SpanLoop (block_base.py).  The span size follows the header's
        # nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.calapply_wait, self._bf.calapply_sync, mark=self._bf.calapply_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_CALAPPLY", inflight, oring, streaming)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop)

    def _sequence(self, iseq, loop):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, acc_len = self._check_header(ihdr)
        loop.inflight.retire(0)
        if self._ctx != (self.nstand, nfine):
            self._call('calapply_initialize', self.gpu, self.nstand, nfine, self.nsrc)
            self._ctx = (self.nstand, nfine)
            self._set_factors(nfine)
        self._nfine = nfine
        self._set_model(ihdr, nfine)            # (the frequencies are the sequence's)
        gulp_size = nfine * (2 * self.nstand) ** 2 * 8
        self.oring.resize(gulp_size)

        def pending(t):
            if self.update_pending or self._next:
                self._load_pending(ihdr, nfine)

        def apply(t, held, out):
            self._call('calapply_run', held, out.target())
            return {'napply': self.stats['napply'] + 1}

        loop.run(iseq, ihdr['seq0'], gulp_size, acc_len, gulp_size, lambda t: self.output_header(ihdr, t), apply, before=pending)
