"""UpchanPredict: component lists taken out of the fine-channel visibilities on the GPU -- the major cycle of a Cotton-Schwab CLEAN,
and the subtraction of a sky catalogue of thousands of sources.

Reads a ring of UpchanCorr's format in device space (its own, UpchanCalApply's or UpchanPeel's): one span per integration,
  cf32 [nfine][nstand][npol = 2][nstand][npol]
and writes one output span per input span, of the same size and format:
  out[c][s p][t q] = V[c][s p][t q] - M[c][s p][t q]          (mode 'subtract';  'model': out = M)
  M[c][s p][t p] = sum_k C_k^pp a_ks conj(a_kt),  with cross: M[c][s 0][t 1] = sum_k (C_Re + i C_Im)_k a_ks conj(a_kt) and its mirror
Hermitian bit for bit (xengPredict*, csrc/predict_kernels.h; the definition is in include/xeng.h), so UpchanImage reads it
unchanged: with the records of one UpchanClean span, UpchanImage of the output is that span's residual, in all four words.  The
components are UpchanClean's own records, imaging.CLEAN_COMPONENT [nfine / nfavg][n <= ncomp_max] with `pixel` an index into `lmn`
[ndir][3] -- the imager's pixel list, or the directions of any catalogue -- and -1 an empty record; up to 4096 per channel group, of
either sign, each group's list serving its nfavg channels.  `positions` [nstand][3] are the stands' east-north-up coordinates in
metres.  The steering words are formed inside the kernel and never stored; the device keeps the delays and the records.  Without
`cross` the cross-hand words pass through.  The output header is the input's plus `ncomponents`, the filled records of the longest
list, and `nsubtracted`, the input's count plus that.  No reference counterpart: the reference leaves deconvolution to offline
packages.

A gap in the input (spans this reader never saw) loses those integrations and restarts the output in a sequence of its own so that
every span's time follows from its place.  set_components(records) and set_mode(mode) take effect at the next integration, which
begins an output sequence of its own (the header names the count).  Not built: components arriving on a second ring (the host calls
set_components), Gaussian or extended components, per-stand weights, a primary beam, the loop of several major cycles (the caller
chains UpchanImage, UpchanClean and UpchanPredict).
"""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from .block_base import RESTART, Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .imaging import CLEAN_COMPONENT, check_visibility_header, fine_frequencies, steering_delays

MAX_NCOMP = 4096            # XENG_PREDICT_MAX_NCOMP
MAX_NSTAND = 512            # XENG_PREDICT_MAX_NSTAND
MODES = {'subtract': 0, 'model': 1}


class UpchanPredict(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, positions, lmn, nfavg=1, ncomp_max=MAX_NCOMP, components=None, mode='subtract', cross=True, guarantee=True, core=-1,
                 gpu=-1, etcd_client=None, backend=None):
        super(UpchanPredict, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_PREDICT"
        try:
            self.tau = np.ascontiguousarray(steering_delays(positions, lmn))      # [ndir][nstand]
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        self.ndir, self.nstand = self.tau.shape
        if self.nstand > MAX_NSTAND or self.ndir > 1 << 24 or self.tau.nbytes > 1 << 31:
            raise ValueError("%s: %d stands and %d directions, %d stands, 2^24 directions and 2 GiB of delays at the most" % (who, self.nstand, self.ndir, MAX_NSTAND))
        for name, v, top in (('nfavg', nfavg, None), ('ncomp_max', ncomp_max, MAX_NCOMP)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0 or (top is not None and v > top):
                raise ValueError("%s: %s %r is not a positive integer%s" % (who, name, v, "" if top is None else " up to %d" % top))
        self.nfavg, self.ncomp_max, self.cross = int(nfavg), int(ncomp_max), bool(cross)
        self.gpu = gpu
        self._ngroup = None
        self._mode = self._checked_mode(mode)
        self._components = None if components is None else self._checked_components(components)       # None: every record empty
        self._next = {}                         # set_components / set_mode: what the next integration takes
        self._next_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.update_stats({'npredict': 0, 'ngap': 0})
        self._ctx = None                        # (nstand, nfine) of the live context

    @staticmethod
    def _checked_mode(mode):
        if mode not in MODES:
            raise ValueError("UPCHAN_PREDICT: mode %r is not 'subtract' or 'model'" % (mode,))
        return mode

    def _checked_components(self, records, quiet=False):
        """CLEAN_COMPONENT [ngroup][ncomp_max], padded with empty records: pixels in [-1, ndir), the words of the filled records
        finite (ngroup is checked against the sequence); else ValueError, or None if `quiet`."""
        a, ok = None, False
        try:
            r = np.asarray(records)
            ok = r.dtype == CLEAN_COMPONENT and r.ndim == 2 and r.shape[0] > 0 and r.shape[1] <= self.ncomp_max
            if ok and self._ngroup is not None:
                ok = r.shape[0] == self._ngroup
            if ok:
                filled = r['pixel'] != -1
                C = r['C'] if self.cross else r['C'][:, :, :2]
                ok = bool(np.all((r['pixel'] >= -1) & (r['pixel'] < self.ndir))) and bool(np.all(np.isfinite(C[filled])))
            if ok:
                a = np.zeros((r.shape[0], self.ncomp_max), CLEAN_COMPONENT)
                a['pixel'] = -1
                a[:, :r.shape[1]] = r
        except (TypeError, ValueError):
            a, ok = None, False
        if ok:
            return a
        if quiet:
            return None
        raise ValueError("UPCHAN_PREDICT: the components must be CLEAN_COMPONENT records [nfine / %d][n <= %d] with pixels in [-1, %d) and finite words"
                         % (self.nfavg, self.ncomp_max, self.ndir))

    def set_components(self, records):
        """The component records [nfine / nfavg][n <= ncomp_max] (clean_components(span, ...)[0]) from the next integration on."""
        r = self._checked_components(records)
        with self._next_lock:
            self._next['components'] = r

    def set_mode(self, mode):
        """'subtract' (out = V - M) or 'model' (out = M) from the next integration on."""
        m = self._checked_mode(mode)
        with self._next_lock:
            self._next['mode'] = m

    def ncomponents(self):
        """The filled records of the longest list in force."""
        return 0 if self._components is None else int((self._components['pixel'] >= 0).sum(axis=1).max())

    def _check_header(self, ihdr):
        """UpchanCorr's output, UpchanCalApply's, UpchanPeel's or this block's own; returns (nfine, acc_len)."""
        who = "UPCHAN_PREDICT"
        nfine, acc_len = check_visibility_header(who, ihdr, self.nstand, reject=('npix', 'nsrc'))
        if nfine % self.nfavg:
            raise ValueError("%s: nfavg %d does not divide the header's nfine %d" % (who, self.nfavg, nfine))
        if self._components is not None and self._components.shape[0] != nfine // self.nfavg:
            raise ValueError("%s: components for %d channel groups, the header's nfine / nfavg is %d" % (who, self._components.shape[0], nfine // self.nfavg))
        nsub = ihdr.get('nsubtracted', 0)
        if not isinstance(nsub, int) or isinstance(nsub, bool) or nsub < 0:
            raise ValueError("%s: the header's 'nsubtracted' is %r" % (who, nsub))
        return nfine, acc_len

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        n = self.ncomponents()
        ohdr.update(ncomponents=n, nsubtracted=ihdr.get('nsubtracted', 0) + n, predict_mode=self._mode, nbit=32, complex=True, seq0=start)
        return ohdr

    def _set_components(self, ngroup):
        r = self._components
        if r is None:
            r = np.zeros((ngroup, self.ncomp_max), CLEAN_COMPONENT)
            r['pixel'] = -1
        self._call('predict_set_components', r)

    def _load_pending(self, ngroup):
        """set_components or set_mode: on the device before the next integration is enqueued (SetComponents waits for the
        integrations in flight, so each of those keeps what it was enqueued with).  True if anything changed."""
        with self._next_lock:
            nxt, self._next = self._next, {}
        changed = False
        if 'components' in nxt:
            r = self._checked_components(nxt['components'], quiet=True)
            if r is None:
                self.log.warning("UPCHAN_PREDICT: the components are not records for %d channel groups: they stay as they were" % ngroup)
            else:
                self._components = r
                self._set_components(ngroup)
                changed = True
        if 'mode' in nxt and nxt['mode'] != self._mode:
            self._mode = nxt['mode']
            self._call('predict_set_mode', MODES[self._mode])
            changed = True
        return changed

    def main(self):
        self.bind()
        # Streaming and tickets: InFlight, the loop over the spans: SpanLoop (block_base.py).  The span size follows the header's
        # nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.predict_wait, self._bf.predict_sync, mark=self._bf.predict_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_PREDICT", inflight, oring, streaming)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop)

    def _sequence(self, iseq, loop):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, acc_len = self._check_header(ihdr)
        ngroup = nfine // self.nfavg
        loop.inflight.retire(0)
        if self._ctx != (self.nstand, nfine):
            self._call('predict_initialize', self.gpu, self.nstand, nfine, self.nfavg, self.ndir, self.ncomp_max, self.cross)
            self._ctx = (self.nstand, nfine)
            self._set_components(ngroup)
            self._call('predict_set_mode', MODES[self._mode])
        self._ngroup = ngroup
        self._call('predict_set_geometry', self.tau, fine_frequencies(ihdr, nfine))       # (the frequencies are the sequence's)
        gulp_size = nfine * (2 * self.nstand) ** 2 * 8
        self.oring.resize(gulp_size)

        def pending(t):
            if self._next and self._load_pending(ngroup):
                return RESTART                  # the header names the count and the mode: a sequence of its own from here

        def apply(t, held, out):
            self._call('predict_run', held, out.target())
            return {'npredict': self.stats['npredict'] + 1}

        loop.run(iseq, ihdr['seq0'], gulp_size, acc_len, gulp_size, lambda t: self.output_header(ihdr, t), apply, before=pending)
