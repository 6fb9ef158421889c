"""UpchanFlag: robust outlier flags from the fine-channel visibilities, on the GPU.

Reads a ring of UpchanCorr's format in device space -- UpchanCorr's own output or UpchanCalApply's -- one span per integration,
  cf32 [nfine][nstand][npol = 2][nstand][npol]
and writes one output span per input span:
  0             u8  [nfine][2][nstand]     the mask: bit 0 cross-power outlier, 1 auto outlier, 2 channel flagged, 3 non-finite
                                           statistic, 4 weight 0; padded to a multiple of 16 bytes
  stats_offset  f32 [nfine][2][nstand][2]  {R, A}: the summed cross-power of a (stand, polarisation) with all others, and its auto
  chan_offset   f32 [nfine][2][4]          {med_R, mad_R, the channel baseline b, the stands judged}
(xengFlag*, csrc/flag_kernels.h; the definition is in include/xeng.h).  Per (channel, polarisation) a stand is an outlier where its R
or A lies more than nsig x 1.4826 MAD from the median over the stands; per polarisation a channel is flagged where the stands' median R
lies that far from the median over the channels within `wchan` of it (0: over all channels).  A stand with weight 0 is not read.
Every integration stands alone: nothing is kept from one to the next and there is no test along time.  No reference counterpart: the
reference leaves flagging to offline packages.

The mask reaches the other blocks through the host: flags() -> (seq, mask, stats, chan) of the newest finished integration, or None
before the first; blocks/flagging.py turns a mask into UpchanCalApply's factors (flag_factors) and into the per-stand weights of
UpchanGainCal, UpchanImage and UpchanPeel (stand_weights).  The output header is the input's plus `flagged`, the controls `nsig_cross`,
`nsig_auto`, `nsig_chan`, `wchan`, and `stats_offset`, `chan_offset`.

A gap in the input (spans this reader never saw) loses those integrations and restarts the output in a sequence of its own so that
every span's time follows from its place.  set_weights(w) and set_control(nsig_cross, nsig_auto, nsig_chan, wchan) (or the commands
`weights` and `control`) take effect at the next integration; new controls begin an output sequence of their own, since the header
names them.  Not built: a test along time, flags on a ring of their own applied by the downstream blocks without the host, cross-hand
statistics, per-baseline flags.
"""
import json
from threading import Lock

import numpy as np

from ..backend import default_backend
from .block_base import RESTART, Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .flagging import DEFAULT_CONTROL, MAX_NFINE, MAX_NSTAND, checked_control
from .imaging import check_visibility_header, checked_weights


class UpchanFlag(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, nstand, weights=None, nsig_cross=DEFAULT_CONTROL[0], nsig_auto=DEFAULT_CONTROL[1], nsig_chan=DEFAULT_CONTROL[2],
                 wchan=DEFAULT_CONTROL[3], guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanFlag, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_FLAG"
        if isinstance(nstand, bool) or not isinstance(nstand, (int, np.integer)) or not 4 <= nstand <= MAX_NSTAND:
            raise ValueError("%s: %r stands: an integer from 4 to %d" % (who, nstand, MAX_NSTAND))
        self.nstand, self.gpu = int(nstand), gpu
        self._weights = self._checked_weights(np.ones(self.nstand, np.float32) if weights is None else weights)
        self._control = checked_control(who, (nsig_cross, nsig_auto, nsig_chan, wchan))
        self._next = {}                         # set_weights / set_control: what the next integration takes
        self._next_lock = Lock()
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.define_command_key('control', type=list, condition=lambda v: checked_control(who, v, quiet=True) is not None)
        self.update_stats({'nflag': 0, 'ngap': 0, 'flagged_fraction': 0.0})
        self._ctx = None                        # (nstand, nfine) of the live context
        self._flags = None                      # (seq, mask, stats, chan) of the newest finished integration
        self._flags_lock = Lock()

    def _checked_weights(self, w, quiet=False):
        """f32 [nstand], finite and >= 0, at least 4 of them > 0; else ValueError, or None if `quiet`."""
        a = checked_weights("UPCHAN_FLAG", w, self.nstand, quiet=quiet)
        if a is not None and int((a > 0).sum()) < 4:
            if quiet:
                return None
            raise ValueError("UPCHAN_FLAG: the weights leave %d stands, the tests need 4 at the least" % int((a > 0).sum()))
        return a

    def set_weights(self, w):
        """Per-stand weights, on / off, from the next integration on (0: the stand is not read)."""
        a = self._checked_weights(w)
        with self._next_lock:
            self._next['weights'] = a

    def set_control(self, nsig_cross, nsig_auto, nsig_chan, wchan):
        """The three tests' thresholds in sigma (0: that test is off) and the channel test's half window (0: all channels), from the
        next integration on."""
        c = checked_control("UPCHAN_FLAG", (nsig_cross, nsig_auto, nsig_chan, wchan))
        with self._next_lock:
            self._next['control'] = c

    def flags(self):
        """(seq, mask uint8 [nfine][2][nstand], stats float32 [nfine][2][nstand][2], chan float32 [nfine][2][4]) of the newest
        finished integration -- seq is its first sample -- or None before the first."""
        with self._flags_lock:
            return self._flags

    def _check_header(self, ihdr):
        """UpchanCorr's output, calibrated or not; returns (nfine, acc_len)."""
        who = "UPCHAN_FLAG"
        nfine, acc_len = check_visibility_header(who, ihdr, self.nstand, reject=('npix', 'nsrc', 'flagged'))
        if nfine > MAX_NFINE:
            raise ValueError("%s: %d fine channels, %d at the most" % (who, nfine, MAX_NFINE))
        return nfine, acc_len

    def layout(self, nfine):
        """(stats_offset, chan_offset, span bytes) of an output span"""
        stats_offset = (nfine * 2 * self.nstand + 15) & ~15
        chan_offset = stats_offset + nfine * 2 * self.nstand * 2 * 4
        return stats_offset, chan_offset, chan_offset + nfine * 2 * 4 * 4

    def output_header(self, ihdr, start, nfine):
        ohdr = ihdr.copy()
        stats_offset, chan_offset, _ = self.layout(nfine)
        c = self._control
        ohdr.update(flagged=True, nsig_cross=c[0], nsig_auto=c[1], nsig_chan=c[2], wchan=c[3], stats_offset=stats_offset, chan_offset=chan_offset, nbit=8,
                    complex=False, seq0=start)
        return ohdr

    def _load_pending(self):
        """set_* or a command: on the device before the next integration is enqueued (the setters wait for the integrations in
        flight, so each of those keeps what it was enqueued with).  Returns whether the controls changed."""
        with self._next_lock:
            nxt, self._next = self._next, {}
        if self.update_pending:
            nxt.update(self.take_commands(('weights', 'control')))
        if 'weights' in nxt:
            w = self._checked_weights(nxt['weights'], quiet=True)
            if w is None:
                self.log.warning("UPCHAN_FLAG: the weights are not %d finite numbers >= 0 that leave 4 stands: they stay as they were" % self.nstand)
            else:
                self._weights = w
                self._call('flag_set_weights', self._weights)
        if 'control' in nxt:
            c = checked_control("UPCHAN_FLAG", nxt['control'], quiet=True)
            if c is None:
                self.log.warning("UPCHAN_FLAG: the control %r is not valid: it stays as it was" % (nxt['control'],))
            elif c != self._control:
                self._control = c
                self._call('flag_set_control', *c)
                return True
        return False

    def _finish(self, ospan, meta):
        """A call's kernels have completed: its mask, stats and chan go to the host, then its span is committed."""
        try:
            if meta is not None:
                t, nfine = meta
                stats_offset, chan_offset, size = self.layout(nfine)
                raw = np.array(ospan.data.numpy(), copy=True).reshape(-1).view(np.uint8)[:size]
                mask = raw[:nfine * 2 * self.nstand].reshape(nfine, 2, self.nstand)
                with self._flags_lock:
                    self._flags = (t, mask, raw[stats_offset:chan_offset].view(np.float32).reshape(nfine, 2, self.nstand, 2),
                                   raw[chan_offset:size].view(np.float32).reshape(nfine, 2, 4))
                self.update_stats({'flagged_fraction': float((mask != 0).mean())})
        finally:
            ospan.close()

    def main(self):
        self.bind()
        # Streaming and tickets: InFlight, the loop over the spans: SpanLoop (block_base.py).  The output size follows the header's
        # nfine: the ring is sized per sequence.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.flag_wait, self._bf.flag_sync, finish=self._finish, mark=self._bf.flag_mark) as inflight, self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "UPCHAN_FLAG", inflight, oring, streaming)
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop)

    def _sequence(self, iseq, loop):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        nfine, acc_len = self._check_header(ihdr)
        loop.inflight.retire(0)
        if self._ctx != (self.nstand, nfine):
            self._call('flag_initialize', self.gpu, self.nstand, nfine)
            self._ctx = (self.nstand, nfine)
            self._call('flag_set_weights', self._weights)
            self._call('flag_set_control', *self._control)
        stats_offset, chan_offset, ogulp_size = self.layout(nfine)
        self.oring.resize(ogulp_size)

        def pending(t):
            if (self.update_pending or self._next) and self._load_pending():
                return RESTART                  # the header names the controls: a sequence of its own from here

        def flag(t, held, out):
            self._call('flag_run', held, out.target((t, nfine)), stats_offset, chan_offset)
            return {'nflag': self.stats['nflag'] + 1}

        loop.run(iseq, ihdr['seq0'], nfine * (2 * self.nstand) ** 2 * 8, acc_len, ogulp_size, lambda t: self.output_header(ihdr, t, nfine), flag, before=pending)
