"""BeamDedisperse: incoherent dedispersion of fine-channel power beams over a grid of DM trials.

Reads the output ring of UpchanSumBeams (live) or of UpchanBeamform(dual_pol=True) (from dumps), in device space: spans of
  f32 [nwin][npair][nchan][nupchan][4] = [XX, YY, Re(XY*), Im(XY*)]
and writes one output span per input span,
  f32 [nwin][npair][ndm][nprod],   nprod = 1 (stokes='I': XX + YY) or 4 (stokes='full': the four words, each by itself)
where output window n of trial d is the sum over the nfine = nchan*nupchan fine channels of window n - (S - s[d][q]) of channel
q, times the channel's weight (xengDedisp*, csrc/dedisp_kernels.h; the definition is in include/xeng.h).  s = dm_delays(...) is
built per sequence from the header's fine-channel frequencies and the window length tsamp = acc_len * nchan / bw_hz; S = max s
is the block's latency in windows (`dedisp_latency` in the output header): all trials share one time axis, output n is the
pulse that reached the top fine channel at window n - S, and the first S windows of a sequence are partial sums.  The history
lives on the device across spans.  No reference counterpart: the reference has no dedisperser.

A new sequence or a gap in the input (spans this reader never saw) resets the context; after a gap the output restarts in a
sequence of its own (UpchanSumBeams' rule).  A `weights` command (a list of nfine finite numbers; 0 leaves a channel out, e.g.
one flagged by UpchanSpectra's spectral kurtosis) takes effect at the next span, on the history already held too.
"""
import json
import math

import numpy as np

from ..backend import default_backend
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .dedisp import dm_delays

STOKES = {'I': 1, 'full': 4}


def check_power_beam_header(who, ihdr, npair, nchan, nupchan):
    """The header of the dual-pol fine-channel power beams of UpchanSumBeams / UpchanBeamform(dual_pol=True), as every reader of
    that ring (BeamDedisperse, BeamFold) checks it; returns acc_len, the samples per window."""
    if ihdr.get('nchan') != nchan or ihdr.get('nbeam') != npair:
        raise ValueError("%s: %r channels x %r pairs in the header, %d x %d configured" % (who, ihdr.get('nchan'), ihdr.get('nbeam'), nchan, npair))
    if ihdr.get('npol') != 2 or ihdr.get('nbit') != 32:
        raise ValueError("%s: the input is not dual-pol f32 power beams (npol %r, nbit %r)" % (who, ihdr.get('npol'), ihdr.get('nbit')))
    if ihdr.get('nupchan') != nupchan:
        raise ValueError("%s: nupchan %r in the header, %d configured" % (who, ihdr.get('nupchan'), nupchan))
    for k in ('nframe_sum', 'fine_sfreq', 'fine_bw_hz', 'bw_hz'):
        if not isinstance(ihdr.get(k), (int, float)) or isinstance(ihdr.get(k), bool) or (k != 'fine_sfreq' and not ihdr[k] > 0):
            raise ValueError("%s: the header's '%s' is %r: not fine-channel power beams summed over windows" % (who, k, ihdr.get(k)))
    acc_len = ihdr['nframe_sum'] * nupchan
    if ihdr.get('acc_len', acc_len) != acc_len:
        raise ValueError("%s: acc_len %r in the header is not nframe_sum x nupchan = %d" % (who, ihdr.get('acc_len'), acc_len))
    return acc_len


def _number(v):
    """A finite int or float (a bool is neither)."""
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def check_dedispersed_header(who, ihdr, npair, ndm):
    """The header of BeamDedisperse's output, as every reader of that ring (BeamPulseSearch, BeamPeriodSearch) checks it; returns
    (nprod, acc_len, dedisp_latency, dms, tsamp)."""
    if 'ndm' not in ihdr:
        raise ValueError("%s: the input carries no 'ndm': it has not been dedispersed" % who)
    if ihdr.get('ndm') != ndm or ihdr.get('nbeam') != npair:
        raise ValueError("%s: %r trials x %r pairs in the header, %d x %d configured" % (who, ihdr.get('ndm'), ihdr.get('nbeam'), ndm, npair))
    if ihdr.get('nprod') not in (1, 4):
        raise ValueError("%s: nprod %r in the header, not 1 or 4" % (who, ihdr.get('nprod')))
    if not _number(ihdr.get('tsamp')) or not ihdr['tsamp'] > 0:
        raise ValueError("%s: the header's 'tsamp' is %r" % (who, ihdr.get('tsamp')))
    dms = ihdr.get('dms')
    if not isinstance(dms, list) or len(dms) != ndm:
        raise ValueError("%s: the header's 'dms' are not %d trials" % (who, ndm))
    S = ihdr.get('dedisp_latency')
    if not isinstance(S, int) or isinstance(S, bool) or S < 0:
        raise ValueError("%s: the header's 'dedisp_latency' is %r" % (who, S))
    acc_len = ihdr.get('acc_len')
    if acc_len is None and isinstance(ihdr.get('nframe_sum'), int) and isinstance(ihdr.get('nupchan'), int):
        acc_len = ihdr['nframe_sum'] * ihdr['nupchan']
    if not isinstance(acc_len, int) or isinstance(acc_len, bool) or acc_len <= 0:
        raise ValueError("%s: the header's 'acc_len' is %r: no window length in samples" % (who, acc_len))
    return ihdr['nprod'], acc_len, S, dms, float(ihdr['tsamp'])


def checked_fine_weights(who, w, nfine, quiet=False):
    """The per-fine-channel weights as the library takes them, f32 [nfine]; not `nfine` finite numbers: ValueError, or None if `quiet`."""
    try:
        a = np.ascontiguousarray(w, np.float32).reshape(-1)
        ok = a.size == nfine and bool(np.all(np.isfinite(a)))
    except (TypeError, ValueError):
        a, ok = None, False
    if ok:
        return a
    if quiet:
        return None
    raise ValueError("%s: the weights must be %d finite numbers" % (who, nfine))


class BeamDedisperse(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, nchan, nupchan, nwin, dms, max_delay=None, weights=None, stokes='I', guarantee=True,
                 core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamDedisperse, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_DEDISPERSE"
        if stokes not in STOKES:
            raise ValueError("%s: stokes %r not one of %s" % (who, stokes, sorted(STOKES)))
        if min(npair, nchan, nupchan, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r nchan=%r nupchan=%r nwin=%r must be positive" % (who, npair, nchan, nupchan, nwin))
        self.dms = np.asarray(dms, np.float64).reshape(-1)
        if self.dms.size == 0 or not np.all(np.isfinite(self.dms)) or self.dms.min() < 0:
            raise ValueError("%s: the DM trials must be a non-empty list of finite, non-negative numbers" % who)
        if max_delay is not None and max_delay < 0:
            raise ValueError("%s: max_delay %r is negative" % (who, max_delay))
        self.npair, self.nchan, self.nupchan, self.nwin, self.gpu = npair, nchan, nupchan, nwin, gpu
        self.nfine, self.ndm, self.nprod, self.stokes = nchan * nupchan, int(self.dms.size), STOKES[stokes], stokes
        self.max_delay = max_delay
        self._weights = self._checked_weights(weights) if weights is not None else None
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.update_stats({'nwindow': 0, 'ngap': 0, 'dedisp_latency': -1})
        self._ctx_delay = None                  # max_delay of the live context
        if max_delay is not None:
            self._initialize(max_delay)

    def _checked_weights(self, w, quiet=False):
        return checked_fine_weights("BEAM_DEDISPERSE", w, self.nfine, quiet)

    def _initialize(self, max_delay):
        self._call('dedisp_initialize', self.gpu, self.npair, self.nfine, self.nwin, self.ndm, max_delay, self.nprod)
        self._ctx_delay = max_delay
        if self._weights is not None:
            self._set_weights()

    def _set_weights(self):
        self._call('dedisp_set_weights', self._weights)

    def _check_header(self, ihdr):
        """The dual-pol fine-channel power beams of UpchanSumBeams / UpchanBeamform(dual_pol=True) only."""
        acc_len = check_power_beam_header("BEAM_DEDISPERSE", ihdr, self.npair, self.nchan, self.nupchan)
        if 'ndm' in ihdr:
            raise ValueError("BEAM_DEDISPERSE: the input carries 'ndm': it has been dedispersed already")
        return acc_len

    def delays(self, ihdr, acc_len):
        """(int32 [ndm][nfine], tsamp): the table of a sequence from its header."""
        tsamp = acc_len * self.nchan / ihdr['bw_hz']
        freqs = ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * np.arange(self.nfine)
        return np.ascontiguousarray(dm_delays(freqs, self.dms, tsamp)), tsamp

    def output_header(self, ihdr, start, S, tsamp):
        ohdr = ihdr.copy()
        ohdr.update(ndm=self.ndm, dms=self.dms.tolist(), dedisp_latency=int(S), nprod=self.nprod, tsamp=tsamp, seq0=start)
        return ohdr

    def main(self):
        self.bind()
        ogulp_size = self.nwin * self.npair * self.ndm * self.nprod * 4
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        streaming = spans_outlive_release(self.iring, self.oring)
        staged = streaming and self.oring.space == 'cuda_host' and hasattr(self._bf, 'copy_async')
        with InFlight(self._bf.dedisp_wait, self._bf.dedisp_sync, self._bf, mark=self._bf.dedisp_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_DEDISPERSE", inflight, oring, streaming, staged, gap_note=": the history starts again")
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _load_pending_weights(self):
        """A `weights` command: on the device before the next span is enqueued (SetWeights waits for the spans in flight)."""
        self.update_command_vals()
        w = self.command_vals.get('weights')
        if w is not None:
            self._weights = self._checked_weights(w)
            self._set_weights()

    def _sequence(self, iseq, loop, ogulp_size):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        acc_len = self._check_header(ihdr)
        table, tsamp = self.delays(ihdr, acc_len)
        S = int(table.max())
        if self.max_delay is not None and S > self.max_delay:
            raise ValueError("BEAM_DEDISPERSE: DM %g needs a delay of %d windows of %g s, max_delay is %d" % (self.dms.max(), S, tsamp, self.max_delay))
        loop.inflight.retire(0)
        if self.max_delay is None and self._ctx_delay != S:
            self._initialize(S)                 # (a history as long as this sequence's table needs)
        self._call('dedisp_set_delays', table)  # (clears the history and the window count: a new sequence starts from nothing)
        self.update_stats({'dedisp_latency': S})

        def pending(t):
            if self.update_pending:
                self._load_pending_weights()

        def dedisperse(t, held, out):
            self._call('dedisp_run', held, self.nwin, out.target())
            return {'nwindow': self.stats['nwindow'] + self.nwin}

        # (a span is nwin windows of acc_len samples of the beamformer's clock; after a gap what the history holds does not line up
        # with what comes now)
        loop.run(iseq, ihdr['seq0'], self.nwin * self.npair * self.nfine * 16, self.nwin * acc_len, ogulp_size,
                 lambda t: self.output_header(ihdr, t, S, tsamp), dedisperse, before=pending, on_gap=self._bf.dedisp_reset)
