"""UpchanImage: dirty images of the fine-channel visibilities, by the direct Fourier sum on the GPU.

Reads the output ring of UpchanCorr in device space: one span per integration,
  cf32 [nfine][nstand][npol = 2][nstand][npol]
and writes one output span per input span,
  f32 [nfine / nfavg][4][npix] = [XX, YY, Re(XY), Im(XY)]
the visibility matrix beamformed onto every direction of a list and averaged over groups of `nfavg` fine channels (xengImage*,
csrc/image_kernels.h; the definition is in include/xeng.h).  The list `lmn` [npix][3] is fixed for the block's life: an all-sky
grid, patches around sources, or both (imaging.py); `positions` [nstand][3] are the stands' east-north-up coordinates in metres.
The geometry (steering_delays, and the fine-channel frequencies from the header's fine_sfreq / fine_bw_hz) is set per sequence.
With weights w (default: all 1) and without autos a unit point source at a pixel reads 1 there; a stand with weight 0 is not
read at all, so a flagged input may hold anything.  No reference counterpart: the reference writes its visibilities to disk
(DESIGN.md 8); there is no file writer here either.

A gap in the input (spans this reader never saw) loses nothing but those integrations; the output restarts in a sequence of its own
so that every span's time follows from its place.  set_weights(w) (or a `weights` command, a list of nstand numbers) takes effect
at the next integration.
"""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .imaging import check_visibility_header, checked_weights, fine_frequencies, steering_delays


class UpchanImage(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, positions, lmn, nfavg=1, weights=None, autos=False, guarantee=True, core=-1, gpu=-1,
                 etcd_client=None, backend=None):
        super(UpchanImage, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_IMAGE"
        try:
            self.tau = steering_delays(positions, lmn)      # [npix][nstand]
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        self.npix, self.nstand = self.tau.shape
        if isinstance(nfavg, bool) or not isinstance(nfavg, (int, np.integer)) or nfavg <= 0:
            raise ValueError("%s: nfavg %r is not a positive integer" % (who, nfavg))
        self.nfavg, self.autos, self.gpu = int(nfavg), bool(autos), gpu
        self._weights = self._checked_weights(np.ones(self.nstand, np.float32) if weights is None else weights)
        self._next_weights = None               # set_weights: what the next integration takes
        self._weights_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.update_stats({'nimage': 0, 'ngap': 0})
        self._ctx = None                        # (nstand, nfine) of the live context

    def _checked_weights(self, w, quiet=False):
        """f32 [nstand], finite and >= 0, leaving a pair of stands; else ValueError, or None if `quiet`."""
        return checked_weights("UPCHAN_IMAGE", w, self.nstand, (self.autos, self.nfavg), quiet)

    def set_weights(self, w):
        """Per-stand weights from the next integration on (0: the stand is not read)."""
        a = self._checked_weights(w)
        with self._weights_lock:
            self._next_weights = a

    def _check_header(self, ihdr):
        """UpchanCorr's output only; returns (nfine, acc_len)."""
        who = "UPCHAN_IMAGE"
        if 'npix' in ihdr:
            raise ValueError("%s: the input carries 'npix': it has been imaged already" % who)
        nfine, acc_len = check_visibility_header(who, ihdr, self.nstand)
        if nfine % self.nfavg:
            raise ValueError("%s: nfavg %d does not divide the header's nfine %d" % (who, self.nfavg, nfine))
        return nfine, acc_len

    def output_header(self, ihdr, start, nfine):
        ohdr = ihdr.copy()
        ohdr.update(npix=self.npix, nfavg=self.nfavg, nprod=4, autos=self.autos, nbit=32, complex=False, seq0=start,
                    image_sfreq=ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * (self.nfavg - 1) / 2.0, image_bw_hz=ihdr['fine_bw_hz'] * self.nfavg)
        return ohdr

    def _set_weights(self):
        self._call('image_set_weights', self._weights, self.autos)

    def _load_pending_weights(self):
        """set_weights or a `weights` command: on the device before the next integration is enqueued (SetWeights waits for the
        integrations in flight, so each of those keeps the weights it was enqueued with)."""
        with self._weights_lock:
            w, self._next_weights = self._next_weights, None
        if self.update_pending:
            self.update_command_vals()
            cmd = self.command_vals.get('weights')
            if cmd is not None:
                w = self._checked_weights(cmd)
        if w is not None:
            self._weights = w
            self._set_weights()

    def main(self):
        self.bind()
        # Streaming and tickets: InFlight, the loop over the spans: SpanLoop (block_base.py).  The output size follows the header's
        # nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.image_wait, self._bf.image_sync, mark=self._bf.image_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_IMAGE", inflight, oring, streaming)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop)

    def _sequence(self, iseq, loop):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, acc_len = self._check_header(ihdr)
        loop.inflight.retire(0)
        if self._ctx != (self.nstand, nfine):
            self._call('image_initialize', self.gpu, self.nstand, nfine, self.nfavg, self.npix)
            self._ctx = (self.nstand, nfine)
            self._set_weights()
        self._call('image_set_geometry', self.tau, fine_frequencies(ihdr, nfine))
        ogulp_size = (nfine // self.nfavg) * 4 * self.npix * 4
        self.oring.resize(ogulp_size)

        def pending(t):
            if self.update_pending or self._next_weights is not None:
                self._load_pending_weights()

        def image(t, held, out):
            self._call('image_run', held, out.target())
            return {'nimage': self.stats['nimage'] + 1}

        # (nothing is carried from one integration to the next: a gap only breaks the time axis)
        loop.run(iseq, ihdr['seq0'], nfine * (2 * self.nstand) ** 2 * 8, acc_len, ogulp_size, lambda t: self.output_header(ihdr, t, nfine), image,
                 before=pending)
