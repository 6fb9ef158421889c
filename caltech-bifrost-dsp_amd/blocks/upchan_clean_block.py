"""UpchanClean: Hogbom CLEAN of UpchanImage's dirty images on the GPU, with the imager's exact point-spread function.

Reads the output ring of UpchanImage (or of another UpchanClean: cleaning deeper) in device space: one span per integration,
  f32 [nfine / nfavg][4][npix] = [XX, YY, Re(XY), Im(XY)]          (a cleaned span's records and stats behind it are not read)
and writes one output span per input span (xengClean*, csrc/clean_kernels.h; the definition is in include/xeng.h):
  0             f32 [ngroup][4][npix], the residual: the format of the input, so anything that reads an image reads it
  comp_offset   [ngroup][niter][8] 32-bit words {i32 pixel, f32 I, f32 C_XX, C_YY, C_Re, C_Im, 0, 0}: the components
  stats_offset  [ngroup][4] 32-bit words {i32 ncomp, i32 reason, f32 peak, 0}
(imaging.clean_components takes a span apart; restore and components_to_model use what it returns).  Per channel group the
brightest pixel of the window in |XX + YY| is found, `gain` of its four words recorded and that much of the point-spread function
subtracted from every pixel of the list, until `niter` components, or the peak is at or below max(threshold, fraction * the first
peak), or nothing finite is left in the window.

`positions` and `lmn` must be UpchanImage's; nfavg, autos, nfine and the frequencies come from the header.  The weights are NOT in
the header: `weights` (default: all 1) must be the ones UpchanImage ran with, or the point-spread function is another array's.
`window` (bool or 0/1 per pixel, default every pixel) says where components may sit; every pixel is subtracted from.

set_weights, set_window, set_control and the commands `weights`, `niter` (at most the constructor's), `gain` and `threshold` hold
from the next integration.  A change of niter, gain, threshold or fraction starts a new output sequence, so that a sequence's
header describes every span of it; a span always has the size of the constructor's niter, and what lies past stats_offset + 16
ngroup of a shallower run is not written.  A gap in the input loses nothing but those integrations; the output restarts in a
sequence of its own.  No reference counterpart.
"""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from .block_base import RESTART, Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .imaging import check_fine_axis, checked_weights, clean_layout, fine_frequencies, image_norm, steering_delays

MAX_NITER = 4096        # XENG_CLEAN_MAX_NITER


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and bool(np.isfinite(v))


class UpchanClean(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, positions, lmn, niter, gain=0.1, threshold=0.0, fraction=0.0, window=None, weights=None, guarantee=True,
                 core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanClean, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_CLEAN"
        try:
            self.tau = steering_delays(positions, lmn)      # [npix][nstand]
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        self.npix, self.nstand = self.tau.shape
        if isinstance(niter, bool) or not isinstance(niter, (int, np.integer)) or not 1 <= niter <= MAX_NITER:
            raise ValueError("%s: niter %r is not an integer in [1, %d]" % (who, niter, MAX_NITER))
        self.niter_max, self.gpu = int(niter), gpu
        self._control = self._checked_control(niter, gain, threshold, fraction)
        self._weights = self._checked_weights(np.ones(self.nstand, np.float32) if weights is None else weights)
        self._window = self._checked_window(window)
        self._next = {}                         # set_weights / set_window / set_control: what the next integration takes
        self._next_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.define_command_key('niter', type=int, condition=lambda v: not isinstance(v, bool) and 0 <= v <= self.niter_max)
        self.define_command_key('gain', type=(int, float), condition=lambda v: _is_number(v) and 0 < v <= 1)
        self.define_command_key('threshold', type=(int, float), condition=lambda v: _is_number(v) and v >= 0)
        self.update_stats({'nclean': 0, 'ngap': 0})
        self._ctx = None                        # (nstand, nfine, nfavg) of the live context
        self._autos = False

    # ------------------------------------------------------------------ checked arguments
    def _checked_weights(self, w, quiet=False):
        """f32 [nstand], finite and >= 0, with two stands left (a pair whatever the header's autos); else ValueError, or None if `quiet`."""
        return checked_weights("UPCHAN_CLEAN", w, self.nstand, (False, 1), quiet)

    def _checked_window(self, window):
        if window is None:
            return None
        try:
            a = np.asarray(window)
            ok = a.shape == (self.npix,) and a.dtype.kind in 'biu'
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("UPCHAN_CLEAN: the window must be %d booleans or integers, one per pixel" % self.npix)
        return np.ascontiguousarray(a != 0, np.uint8)

    def _checked_control(self, niter, gain, threshold, fraction):
        ok = (isinstance(niter, (int, np.integer)) and not isinstance(niter, bool) and 0 <= niter <= self.niter_max and _is_number(gain)
              and 0 < gain <= 1 and _is_number(threshold) and threshold >= 0 and _is_number(fraction) and fraction >= 0)
        if not ok:
            raise ValueError("UPCHAN_CLEAN: niter %r in [0, %d], gain %r in (0, 1], threshold %r and fraction %r finite and >= 0 are required"
                             % (niter, self.niter_max, gain, threshold, fraction))
        return int(niter), float(np.float32(gain)), float(np.float32(threshold)), float(np.float32(fraction))

    def set_weights(self, w):
        """Per-stand weights from the next integration on: UpchanImage's."""
        a = self._checked_weights(w)
        with self._next_lock:
            self._next['weights'] = a

    def set_window(self, window):
        """Where components may sit, from the next integration on (None: every pixel)."""
        a = self._checked_window(window)
        with self._next_lock:
            self._next['window'] = (a,)

    def set_control(self, niter=None, gain=None, threshold=None, fraction=None):
        """niter (at most the constructor's), gain, threshold, fraction from the next integration on; None keeps a value."""
        with self._next_lock:
            cur = self._next.get('control', self._control)
            new = tuple(c if v is None else v for c, v in zip(cur, (niter, gain, threshold, fraction)))
            self._next['control'] = self._checked_control(*new)

    # ------------------------------------------------------------------ the header
    def _check_header(self, ihdr):
        """UpchanImage's output (or UpchanClean's) only; returns (nfine, nfavg, autos, acc_len)."""
        who = "UPCHAN_CLEAN"
        if ihdr.get('npix') != self.npix:
            raise ValueError("%s: 'npix' is %r in the header, %d directions here: not UpchanImage's images of this list" % (who, ihdr.get('npix'), self.npix))
        if ihdr.get('nprod') != 4:
            raise ValueError("%s: 'nprod' is %r in the header: four-word images only" % (who, ihdr.get('nprod')))
        if ihdr.get('nstand') != self.nstand:
            raise ValueError("%s: %r stands in the header, positions for %d" % (who, ihdr.get('nstand'), self.nstand))
        if ihdr.get('nbit') != 32 or ihdr.get('complex'):
            raise ValueError("%s: the input is not f32 images (nbit %r, complex %r)" % (who, ihdr.get('nbit'), ihdr.get('complex')))
        nfine, nfavg = ihdr.get('nfine'), ihdr.get('nfavg')
        for k, v in (('nfine', nfine), ('nfavg', nfavg)):
            if not isinstance(v, int) or isinstance(v, bool) or v <= 0:
                raise ValueError("%s: the header's '%s' is %r: not UpchanImage's images" % (who, k, v))
        if nfine % nfavg:
            raise ValueError("%s: the header's nfavg %d does not divide its nfine %d" % (who, nfavg, nfine))
        if not isinstance(ihdr.get('autos'), bool):
            raise ValueError("%s: the header's 'autos' is %r" % (who, ihdr.get('autos')))
        acc_len = check_fine_axis(who, ihdr)
        if ihdr.get('cleaned'):
            so = ihdr.get('stats_offset')
            if not isinstance(so, int) or isinstance(so, bool) or so < 16 * (nfine // nfavg) * self.npix:
                raise ValueError("%s: a cleaned input whose 'stats_offset' is %r" % (who, so))
        return nfine, nfavg, ihdr['autos'], acc_len

    def input_span_bytes(self, ihdr, nfine, nfavg):
        """An image, or a cleaned span: its residual is at the front, and the header says where the span ends."""
        ngroup = nfine // nfavg
        if ihdr.get('cleaned'):
            return max(ihdr['stats_offset'] + 16 * ngroup, ihdr.get('span_bytes', 0))
        return ngroup * 4 * self.npix * 4

    def output_header(self, ihdr, start, ngroup, span_bytes):
        niter, gain, threshold, fraction = self._control
        comp_offset, stats_offset, _ = clean_layout(ngroup, niter, self.npix)
        ohdr = ihdr.copy()
        ohdr.update(cleaned=True, niter=niter, gain=gain, threshold=threshold, fraction=fraction, comp_offset=comp_offset, stats_offset=stats_offset,
                    span_bytes=span_bytes, seq0=start)
        return ohdr

    # ------------------------------------------------------------------ pending changes
    def _load_pending(self):
        """What set_* and the commands left: on the device before the next integration is enqueued (the Set calls wait for the
        integrations in flight, so each of those keeps what it was enqueued with).  True if the control changed."""
        with self._next_lock:
            nxt, self._next = self._next, {}
        w, control = nxt.get('weights'), nxt.get('control', self._control)
        if self.update_pending:
            cmd = self.take_commands(('weights', 'niter', 'gain', 'threshold'))
            if cmd.get('weights') is not None:
                w = self._checked_weights(cmd['weights'])
            new = [cmd.get('niter'), cmd.get('gain'), cmd.get('threshold'), None]
            control = self._checked_control(*(c if v is None else v for c, v in zip(control, new)))
        if w is not None:
            self._weights = w
            self._call('clean_set_weights', self._weights, self._autos)
        if 'window' in nxt:
            self._window = nxt['window'][0]
            self._call('clean_set_window', self._window)
        changed = control != self._control
        if changed:
            self._control = control
            self._call('clean_set_control', *self._control)
        return changed

    def main(self):
        self.bind()
        # Streaming and tickets: InFlight, the loop over the spans: SpanLoop (block_base.py).  The output size follows the header's
        # nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.clean_wait, self._bf.clean_sync, mark=self._bf.clean_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_CLEAN", inflight, oring, streaming)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop)

    def _sequence(self, iseq, loop):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, nfavg, autos, acc_len = self._check_header(ihdr)
        try:
            image_norm(self._weights, autos, nfavg)
        except ValueError as e:
            raise ValueError("UPCHAN_CLEAN: %s" % e)
        loop.inflight.retire(0)
        self._autos = autos
        if self._ctx != (self.nstand, nfine, nfavg):
            self._call('clean_initialize', self.gpu, self.nstand, nfine, nfavg, self.npix, self.niter_max)
            self._ctx = (self.nstand, nfine, nfavg)
            self._call('clean_set_window', self._window)
            self._call('clean_set_control', *self._control)
        self._call('clean_set_weights', self._weights, autos)
        self._call('clean_set_geometry', self.tau, fine_frequencies(ihdr, nfine))
        ngroup = nfine // nfavg
        ogulp_size = clean_layout(ngroup, self.niter_max, self.npix)[2]
        self.oring.resize(ogulp_size)

        def pending(t):
            if (self.update_pending or self._next) and self._load_pending():
                return RESTART                  # another control: a sequence of its own, whose header says so

        def clean(t, held, out):
            self._call('clean_run', held, out.target())
            return {'nclean': self.stats['nclean'] + 1}

        # (nothing is carried from one integration to the next: a gap only breaks the time axis)
        loop.run(iseq, ihdr['seq0'], self.input_span_bytes(ihdr, nfine, nfavg), acc_len, ogulp_size,
                 lambda t: self.output_header(ihdr, t, ngroup, ogulp_size), clean, before=pending)
