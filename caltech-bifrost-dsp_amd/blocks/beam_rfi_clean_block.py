"""BeamRfiClean: bandpass normalisation, zero-DM subtraction and outlier excision of the fine-channel power beams.

Reads the output ring of UpchanSumBeams (live) or of UpchanBeamform(dual_pol=True) (from dumps), in device space: spans of
  f32 [nwin][npair][nchan][nupchan][4] = [XX, YY, Re(XY*), Im(XY*)]
and writes a ring of the same format, time-aligned, so that BeamDedisperse and BeamFold read it unchanged (BeamCoherentDedisperse
stands in the voltage ring the same way).  Per block of nstat windows and per (pair, fine channel) the mean and variance of the
four words are measured; channels whose variance over squared mean stands out from the band's median by nsig_chan robust sigma,
dead channels and masked ones are dropped for that block; every window of the block is then normalised to zero mean and unit
variance per channel, samples beyond nsig_clip sigma and windows with a broadband excess beyond nsig_broad sigma (or with fewer
than min_fraction of the channels left) are zeroed, and with zerodm the mean over the channels is taken off every window
(xengRfi*, csrc/rfi_kernels.h; the definition is in include/xeng.h).  Excised data is +0, the mean of a normalised channel: the
dedisperser's sums need no weights.  No reference counterpart.

The engine's output is nstat windows late; the block hides that.  It enqueues every span, does not commit the first nstat/nwin
outputs (they lie before the sequence) and begins the output sequence at the input's own seq0: output span j is cleaned input
span j under the input's time tags, nstat/nwin spans late in wall-clock time.  The last nstat windows of a sequence are not
flushed: a sequence of J spans gives J - nstat/nwin output spans.  A new sequence or a gap in the input resets the context;
after a gap the output restarts in a sequence of its own (BeamDedisperse's rule), again nstat/nwin spans short.

Commands `control` ({nsig_chan, nsig_clip, nsig_broad, min_fraction, zerodm}, any subset) and `mask` (a list of nfine numbers,
non-zero leaves the channel out) hold from the next block to be decided; set_control() and set_mask() are the Python entries.
flags() returns the newest decided block's tables.
"""
import json

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray
from .beam_dedisperse_block import check_power_beam_header
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .rfi_clean import CODE_BEFORE, CODE_OK, rfi_controls

CONTROL_KEYS = ('nsig_chan', 'nsig_clip', 'nsig_broad', 'min_fraction', 'zerodm')


def _count(v):
    return isinstance(v, int) and not isinstance(v, bool)


class BeamRfiClean(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, nchan, nupchan, nwin, nstat, nsig_chan=5.0, nsig_clip=6.0, nsig_broad=5.0, min_fraction=0.5, zerodm=True,
                 mask=None, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamRfiClean, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_RFI_CLEAN"
        if not all(_count(v) for v in (npair, nchan, nupchan, nwin, nstat)) or min(npair, nchan, nupchan, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r nchan=%r nupchan=%r nwin=%r nstat=%r must be positive integers" % (who, npair, nchan, nupchan, nwin, nstat))
        nfine = nchan * nupchan
        if npair > 65535 or not 4 <= nfine <= 8192:
            raise ValueError("%s: %d pairs (1 to 65535) of %d fine channels (4 to 8192)" % (who, npair, nfine))
        if not 2 <= nstat <= 1 << 20 or nwin > nstat or nstat % nwin:
            raise ValueError("%s: blocks of nstat=%r windows, not 2 to 2^20 and a whole number of spans of nwin=%r" % (who, nstat, nwin))
        if (nstat + nwin) * npair * nfine * 16 >= 1 << 32:
            raise ValueError("%s: a history of %d + %d windows of %d x %d channels is 4 GiB or more" % (who, nstat, nwin, npair, nfine))
        self.npair, self.nchan, self.nupchan, self.nwin, self.nstat, self.nfine, self.gpu = npair, nchan, nupchan, nwin, nstat, nfine, gpu
        self.nhead = nstat // nwin              # spans of a sequence whose output lies before it
        self._control = self._checked_control(dict(nsig_chan=nsig_chan, nsig_clip=nsig_clip, nsig_broad=nsig_broad, min_fraction=min_fraction, zerodm=zerodm), {})
        self._mask = self._checked_mask(mask) if mask is not None else None
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('control', type=dict, condition=lambda v: self._checked_control(v, self._control, quiet=True) is not None)
        self.define_command_key('mask', type=list, condition=lambda v: self._checked_mask(v, quiet=True) is not None)
        self._sums = dict(samples=0, lost=0, channels=0, dropped=0, windows=0, flagged=0)
        self.update_stats({'nwindow': 0, 'ngap': 0, 'nblock': 0, 'frac_samples': 0.0, 'frac_channels': 0.0, 'frac_windows': 0.0})
        self._live = False
        self._scratch = None                    # where the outputs that lie before a sequence go
        self._stats_pool = []

    # ------------------------------------------------------------------ controls and mask
    def _checked_control(self, v, base, quiet=False):
        """`base` updated by the keys of v, checked through rfi_controls; ValueError, or None if `quiet`."""
        try:
            if not isinstance(v, dict) or not v or set(v) - set(CONTROL_KEYS):
                raise ValueError("the keys are %s" % (CONTROL_KEYS,))
            c = dict(base)
            c.update(v)
            if not isinstance(c.get('zerodm'), (bool, int)):
                raise ValueError("zerodm %r is not a truth value" % (c.get('zerodm'),))
            c['zerodm'] = bool(c['zerodm'])
            rfi_controls(nfine=self.nfine, **dict((k, c[k]) for k in CONTROL_KEYS[:4]))
            return c
        except (TypeError, KeyError, ValueError) as e:
            if quiet:
                return None
            raise ValueError("BEAM_RFI_CLEAN: control %r: %s" % (v, e))

    def _checked_mask(self, m, quiet=False):
        try:
            a = np.asarray(m)
            ok = a.shape == (self.nfine,) and a.dtype.kind in 'biuf' and bool(np.all(np.isfinite(a)))
        except (TypeError, ValueError):
            ok = False
        if ok:
            return (a != 0).astype(np.uint8)
        if quiet:
            return None
        raise ValueError("BEAM_RFI_CLEAN: the mask must be %d numbers" % self.nfine)

    def set_control(self, **kw):
        """Any of nsig_chan, nsig_clip, nsig_broad, min_fraction, zerodm; holds from the next block to be decided (ValueError)."""
        c = self._checked_control(kw, self._control)
        self.acquire_control_lock()
        try:
            self._control, self._control_dirty = c, True
            self.update_pending = True
        finally:
            self.release_control_lock()

    def set_mask(self, mask):
        """nfine numbers, non-zero leaves the channel out (None: no channel); holds from the next block to be decided."""
        m = self._checked_mask(mask) if mask is not None else np.zeros(self.nfine, np.uint8)
        self.acquire_control_lock()
        try:
            self._mask, self._mask_dirty = m, True
            self.update_pending = True
        finally:
            self.release_control_lock()

    _control_dirty = _mask_dirty = False

    def _send_control(self):
        c = self._control
        k = rfi_controls(nfine=self.nfine, **dict((key, c[key]) for key in CONTROL_KEYS[:4]))
        self._call('rfi_set_control', k[0], k[1], k[2], k[3], int(c['zerodm']))
        self._control_dirty = False

    def _send_mask(self, inflight):
        inflight.retire(0)                      # (the setter waits for the stream: the spans in flight are finished first)
        self._call('rfi_set_mask', self._mask)
        self._mask_dirty = False

    def _load_pending(self, inflight):
        cmds = self.take_commands(('control', 'mask'))
        if 'control' in cmds:
            self._control, self._control_dirty = self._checked_control(cmds['control'], self._control), True
        if 'mask' in cmds:
            self._mask, self._mask_dirty = self._checked_mask(cmds['mask']), True
        if self._control_dirty:
            self._send_control()
        if self._mask_dirty:
            self._send_mask(inflight)

    def flags(self):
        """(flags uint8, mu, var, r float32 [npair][nfine], gains float32 [npair][nfine][4]) of the newest decided block; waits for
        the context's work."""
        return self._bf.rfi_block(self.npair, self.nfine)

    # ------------------------------------------------------------------ the loop
    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(rfi_cleaned=True, rfi_nstat=self.nstat, rfi_zerodm=self._control['zerodm'], seq0=start,
                    **dict(('rfi_' + k, self._control[k]) for k in CONTROL_KEYS[:4]))
        return ohdr

    def _finish(self, osp, meta):
        """A span whose kernels (and copy) have completed: its stats go into the running fractions; then commit the span."""
        try:
            st = meta.numpy().reshape(-1).view(np.int32).reshape(self.nwin, self.npair, 4).astype(np.int64)
            self._stats_pool.append(meta)
            seen = st[..., 2] != CODE_BEFORE
            nf = self.nfine
            s = self._sums
            s['samples'] += int(seen.sum()) * nf
            s['lost'] += int((np.where(st[..., 2] == CODE_OK, nf - st[..., 0], nf) * seen).sum())
            s['channels'] += int(seen.sum()) * nf
            s['dropped'] += int((st[..., 3] * seen).sum())
            s['windows'] += int(seen.sum())
            s['flagged'] += int(((st[..., 2] != CODE_OK) & seen).sum())
            if s['windows']:
                self.update_stats({'frac_samples': s['lost'] / s['samples'], 'frac_channels': s['dropped'] / s['channels'],
                                   'frac_windows': s['flagged'] / s['windows']})
        finally:
            osp.close()

    def main(self):
        self.bind()
        ogulp_size = self.nwin * self.npair * self.nfine * 16
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        streaming = spans_outlive_release(self.iring, self.oring)
        staged = streaming and self.oring.space == 'cuda_host' and hasattr(self._bf, 'copy_async')
        with InFlight(self._bf.rfi_wait, self._bf.rfi_sync, self._bf, finish=self._finish, mark=self._bf.rfi_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_RFI_CLEAN", inflight, oring, streaming, staged, gap_note=": the statistics start again")
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _sequence(self, iseq, loop, ogulp_size):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        acc_len = check_power_beam_header("BEAM_RFI_CLEAN", ihdr, self.npair, self.nchan, self.nupchan)
        if ihdr.get('rfi_cleaned'):
            raise ValueError("BEAM_RFI_CLEAN: the input carries 'rfi_cleaned': it has been cleaned already")
        loop.inflight.retire(0)
        if not self._live:
            self._call('rfi_initialize', self.gpu, self.npair, self.nfine, self.nwin, self.nstat)
            self._live = True
            self._send_control()
            if self._mask is not None:
                self._send_mask(loop.inflight)
        else:
            self._bf.rfi_reset()
        if self._scratch is None:
            self._scratch = XArray(shape=(ogulp_size,), dtype=np.uint8, space=self._bf.space_in)
        state = {'n': 0}                        # spans given to the context since its last reset
        step = self.nwin * acc_len

        def gap():
            self._bf.rfi_reset()
            state['n'] = 0

        def pending(t):
            if self.update_pending or self._control_dirty or self._mask_dirty:
                self._load_pending(loop.inflight)

        def clean(t, held, out):
            head = state['n'] < self.nhead
            stats = self._stats_pool.pop() if self._stats_pool else XArray(shape=(self.nwin * self.npair * 16,), dtype=np.uint8, space=self._bf.space_in)
            try:
                target = self._scratch if head else out.target(stats)
                rv, decided = self._bf.rfi_run(held, self.nwin, target, stats)
            finally:
                if head:
                    self._stats_pool.append(stats)      # (the next call's kernels follow this one's on the stream)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("rfi_run returned %d: %s" % (rv, self._bf.last_error()))
            state['n'] += 1
            return {'nwindow': self.stats['nwindow'] + self.nwin, 'nblock': self.stats['nblock'] + int(bool(decided))}

        # (a span is nwin windows of acc_len samples of the beamformer's clock.  SpanLoop begins the output sequence at the first
        # input span, under that span's time tag; the first output span is reserved nhead spans later and is that span, cleaned)
        loop.run(iseq, ihdr['seq0'], ogulp_size, step, ogulp_size, lambda t: self.output_header(ihdr, t), clean, before=pending, on_gap=gap)
