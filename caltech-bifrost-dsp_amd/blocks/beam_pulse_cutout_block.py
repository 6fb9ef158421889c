"""BeamPulseCutout: dedispersed cut-outs and DM refinement of single-pulse candidates, the follow-up stage of BeamPulseSearch as
BeamCandFold is that of the periodicity searches.

A further reader of the ring BeamDedisperse reads (UpchanSumBeams, UpchanBeamform(dual_pol=True) or BeamRfiClean), in device space:
  f32 [nwin][npair][nchan][nupchan][4] = [XX, YY, Re(XY*), Im(XY*)]
The engine keeps nhist windows of I = XX + YY per (pair, fine channel) on the device.  A request {id, pair, dm, seq} -- from
pulse_candidates through cutout_requests, by request() or a `requests` command -- asks for the nt x tscr windows around
beamformer-clock sample seq at the top of the band; once the last window it needs (the lowest channel's, at the highest DM of the
plane) has come, the call that brought it writes one span to a host-space output ring:
  nreq_max x CUTOUT_RECORD {id, status, S, S0, i, iw, j, pad, M, A}      the best boxcar over the plane, and the centre row's
  f32 [nreq_max][nband][nt]                                              the dedispersed dynamic spectrum at the centre trial
  f32 [nreq_max][ndmc][nt]                                               the DM-time plane over ndmc fine trials, dstep apart
(xengCutout*, csrc/cutout_kernels.h; the definition is in include/xeng.h).  Only a call that serves reserves and commits an output
span; the header carries the byte offsets.  Once the span's kernels have completed the block calls on_cutout(list) with, per
served request, dict(id, pair, dm, seq, record, refined, waterfall, plane): `refined` is cutout_refined's dict(dm, width, seq, snr,
snr0) or None without a score.  No reference counterpart: the reference has no detection stage.

Per sequence the fine delay table comes from the header as BeamDedisperse's does; seq becomes a window with the sequence's seq0 and
acc_len, dm the nearest fine trial.  A request whose window lies before the sequence (or before the last gap), or whose first
window has left the history, is counted in `nexpired`.  A `weights` command is BeamDedisperse's.  A gap or a new sequence resets
the context and drops what was pending (counted in `ndropped`).

Not built: the four Stokes words, sharing BeamDedisperse's ring instead of a second history, sub-window delays, a scattering fit,
a file or trigger writer."""
import json

import numpy as np

from ..backend import default_backend
from .beam_dedisperse_block import _number, check_power_beam_header, checked_fine_weights
from .block_base import Block, InFlight, SpanLoop, declare_streams, spans_outlive_release
from .dedisp import dm_delays
from .pulse_cutout import (CUTOUT_REQUEST, MAX_PENDING, CutoutQueue, as_cutouts, cutout_k_mad, cutout_offsets, cutout_refined)


def _count(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class BeamPulseCutout(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, nchan, nupchan, nwin, fine_dms, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, weights=None, on_cutout=None,
                 dstep=1, k_mad=1.0, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamPulseCutout, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "BEAM_PULSE_CUTOUT"
        if not all(_count(v) for v in (npair, nchan, nupchan, nwin, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, dstep)):
            raise ValueError("%s: the sizes must be integers" % who)
        if min(npair, nchan, nupchan, nwin) <= 0:
            raise ValueError("%s: sizes npair=%r nchan=%r nupchan=%r nwin=%r must be positive" % (who, npair, nchan, nupchan, nwin))
        self.fine_dms = np.asarray(fine_dms, np.float64).reshape(-1)
        if self.fine_dms.size == 0 or not np.all(np.isfinite(self.fine_dms)) or self.fine_dms.min() < 0:
            raise ValueError("%s: the fine DM grid must be a non-empty list of finite, non-negative numbers" % who)
        nfine = nchan * nupchan
        if not 1 <= nband <= 256 or nfine % nband:
            raise ValueError("%s: nband %r does not divide the %d fine channels, or is not 1 to 256" % (who, nband, nfine))
        if not 1 <= tscr <= 64 or tscr & (tscr - 1):
            raise ValueError("%s: tscr %r is not a power of two from 1 to 64" % (who, tscr))
        if not 16 <= nt <= 1024 or nt % 2:
            raise ValueError("%s: nt %r is not an even number from 16 to 1024" % (who, nt))
        if not 1 <= ndmc <= 256 or not 1 <= nreq_max <= 64 or not 1 <= dstep <= 1 << 20:
            raise ValueError("%s: ndmc %r not 1 to 256, nreq_max %r not 1 to 64 or dstep %r not 1 to 2^20" % (who, ndmc, nreq_max, dstep))
        if nwidth < 1 or 1 << (nwidth - 1) > nt // 2:
            raise ValueError("%s: nwidth %r not 1 or more with 2^(nwidth-1) <= nt/2" % (who, nwidth))
        if nhist < nt * tscr or (nhist + nwin) * npair * nfine * 4 >= 1 << 32:
            raise ValueError("%s: a history of %r windows is shorter than a cut-out of %d, or is 4 GiB or more" % (who, nhist, nt * tscr))
        if not _number(k_mad) or not k_mad > 0:
            raise ValueError("%s: k_mad %r is not a positive number" % (who, k_mad))
        if on_cutout is not None and not callable(on_cutout):
            raise ValueError("%s: on_cutout is not callable" % who)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the cut-outs go to a host-space ring" % (who, oring.space))
        self.npair, self.nchan, self.nupchan, self.nwin, self.nfine, self.gpu = npair, nchan, nupchan, nwin, nfine, gpu
        self.ndmf, self.nhist, self.nband, self.nt, self.tscr, self.ndmc = int(self.fine_dms.size), nhist, nband, nt, tscr, ndmc
        self.nwidth, self.nreq_max, self.dstep, self.ntu = nwidth, nreq_max, dstep, nt * tscr
        self.k_mad = cutout_k_mad(k_mad)
        self.on_cutout = on_cutout
        self._weights = checked_fine_weights(who, weights, nfine) if weights is not None else None
        self._asked = []                        # requests given by request(), not yet with the library
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernels write the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: checked_fine_weights(who, v, nfine, quiet=True) is not None)
        self.define_command_key('requests', type=list, condition=self._requests_ok)
        self.update_stats({'nwindow': 0, 'npending': 0, 'nserved': 0, 'nexpired': 0, 'ndropped': 0, 'ngap': 0})
        self._call('cutout_initialize', self.gpu, npair, nfine, nwin, self.ndmf, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, self.k_mad)
        if self._weights is not None:
            self._call('cutout_set_weights', self._weights)

    def _checked(self, reqs):
        who = "BEAM_PULSE_CUTOUT"
        if not isinstance(reqs, (list, tuple)):
            raise ValueError("%s: requests are not a list" % who)
        out = []
        for r in reqs:
            if not isinstance(r, dict) or not _count(r.get('id')) or not _count(r.get('pair')) or not 0 <= r['pair'] < self.npair or \
                    not _count(r.get('seq')) or not _number(r.get('dm')) or not -1 << 31 <= r['id'] < 1 << 31:
                raise ValueError("%s: a request needs an integer id and seq, a pair below %d and a finite dm: %r" % (who, self.npair, r))
            out.append(dict(id=int(r['id']), pair=int(r['pair']), dm=float(r['dm']), seq=int(r['seq'])))
        return out

    def _requests_ok(self, v):
        try:
            self._checked(v)
            return True
        except ValueError:
            return False

    def request(self, requests):
        """dicts {id, pair, dm, seq} (cutout_requests), in clock samples; taken up before the next span (checked here; ValueError)."""
        reqs = self._checked(requests)
        self.acquire_control_lock()
        try:
            self._asked += reqs
            self.update_pending = True
        finally:
            self.release_control_lock()

    def delays(self, ihdr, acc_len):
        """(int32 [ndmf][nfine], tsamp): the fine table of a sequence from its header, as BeamDedisperse.delays."""
        tsamp = acc_len * self.nchan / ihdr['bw_hz']
        freqs = ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * np.arange(self.nfine)
        return np.ascontiguousarray(dm_delays(freqs, self.fine_dms, tsamp)), tsamp

    def output_header(self, ihdr, start, tsamp):
        ohdr = ihdr.copy()
        a, b, n = cutout_offsets(self.nreq_max, self.nband, self.nt, self.ndmc)
        ohdr.update(cutout=True, nband=self.nband, nt=self.nt, tscr=self.tscr, ndmc=self.ndmc, nwidth=self.nwidth, nreq_max=self.nreq_max, dstep=self.dstep,
                    fine_dms=self.fine_dms.tolist(), tsamp=tsamp, record_offset=0, waterfall_offset=a, plane_offset=b, span_bytes=n, seq0=start)
        return ohdr

    def _finish(self, osp, meta):
        """A span whose kernels (and copy) have completed: the records in physical units, the callback; then commit the span."""
        try:
            acc_len, served = meta
            rec, W, P = as_cutouts(osp.data.numpy().copy(), self.nreq_max, self.nband, self.nt, self.ndmc)
            cuts = []
            for z, (r, ic, seq_c) in enumerate(served):
                refined = cutout_refined(rec[z], self.fine_dms, ic, self.dstep, self.ndmc, self.nt, self.tscr, seq_c, acc_len)
                cuts.append(dict(r, record=rec[z].copy(), refined=refined, waterfall=W[z].copy(), plane=P[z].copy()))
            if self.on_cutout is not None:
                self.on_cutout(cuts)
        finally:
            osp.close()

    def main(self):
        self.bind()
        ogulp_size = cutout_offsets(self.nreq_max, self.nband, self.nt, self.ndmc)[2]
        self.oring.resize(ogulp_size)
        # Streaming, tickets and the staged copy into a pinned-host output ring: InFlight; the loop over the spans: SpanLoop
        # (block_base.py)
        ospace = getattr(self.oring, 'space', 'system')
        direct = ospace in (self._bf.space_in, 'cuda_host')     # (the kernels can write the span themselves)
        staged = spans_outlive_release(self.iring, self.oring) and ospace == 'cuda_host' and hasattr(self._bf, 'copy_async')
        streaming = spans_outlive_release(self.iring, self.oring) and (direct or staged)
        with InFlight(self._bf.cutout_wait, self._bf.cutout_sync, self._bf, finish=self._finish, mark=self._bf.cutout_mark) as inflight, \
                self.oring.begin_writing() as oring:
            loop = SpanLoop(self, "BEAM_PULSE_CUTOUT", inflight, oring, streaming, staged, gap_note=": the history starts again")
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, loop, ogulp_size)

    def _sequence(self, iseq, loop, ogulp_size):
        who = "BEAM_PULSE_CUTOUT"
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        acc_len = check_power_beam_header(who, ihdr, self.npair, self.nchan, self.nupchan)
        if 'ndm' in ihdr:
            raise ValueError("%s: the input carries 'ndm': it has been dedispersed; the cut-outs need the channelised beams" % who)
        table, tsamp = self.delays(ihdr, acc_len)
        if int(table.max()) + self.ntu > self.nhist:
            raise ValueError("%s: DM %g needs a delay of %d windows of %g s beside a cut-out of %d, nhist is %d" % (
                who, self.fine_dms.max(), int(table.max()), tsamp, self.ntu, self.nhist))
        loop.inflight.retire(0)
        self._call('cutout_set_delays', table)  # (clears the window count and what was pending: a new sequence starts from nothing)
        queue = CutoutQueue(table, self.nhist, self.ntu, self.ndmc, self.nreq_max)
        state = {'base': ihdr['seq0'], 'rebase': False, 'info': {}}      # base: the sample of window 0; info: id -> (request, ic, seq_c)
        self.update_stats({'ndropped': self.stats['ndropped'] + self.stats['npending'], 'npending': 0})

        def gap():
            # windows this reader never saw: what the history holds does not line up with what comes now
            self._bf.cutout_reset()
            state['rebase'] = True
            state['info'] = {}
            self.update_stats({'ndropped': self.stats['ndropped'] + queue.reset(), 'npending': 0})

        def take_up(reqs):
            rows, nexp = [], 0
            for r in reqs:
                n_c = (r['seq'] - state['base']) // acc_len
                if n_c < 0 or len(queue.pending) + len(rows) >= MAX_PENDING:
                    nexp += 1                   # (before the sequence or the last gap; or more waiting than the library takes)
                    continue
                ic = int(np.argmin(np.abs(self.fine_dms - r['dm'])))
                rows.append((r['id'], r['pair'], n_c, ic, self.dstep))
                state['info'][r['id']] = (r, ic, state['base'] + n_c * acc_len)
            if rows:
                self._call('cutout_request', np.array(rows, CUTOUT_REQUEST))
                for row in rows:
                    queue.add(*row)
            self.update_stats({'nexpired': self.stats['nexpired'] + nexp, 'npending': len(queue.pending)})

        def pending(t):
            if state['rebase']:
                state['base'], state['rebase'] = t, False
            if self.update_pending:
                cmds = self.take_commands(('weights', 'requests'))
                if 'weights' in cmds:
                    self._weights = checked_fine_weights(who, cmds['weights'], self.nfine)
                    self._call('cutout_set_weights', self._weights)
                asked = self._checked(cmds['requests']) if 'requests' in cmds else []
                self.acquire_control_lock()
                try:
                    asked, self._asked = self._asked + asked, []
                finally:
                    self.release_control_lock()
                if asked:
                    take_up(asked)

        def cut(t, held, out):
            # only a call that serves reserves and writes an output span: the queue tells from the counts, as the library does
            served, expired = queue.take(self.nwin)
            target = None
            if served:
                target = out.target((acc_len, [state['info'].pop(i) for i in served]))
            for i in expired:
                state['info'].pop(i, None)
            rv, got, gone = self._bf.cutout_run(held, self.nwin, target, self.nreq_max)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("cutout_run returned %d: %s" % (rv, self._bf.last_error()))
            if (list(got), list(gone)) != (served, expired):
                raise RuntimeError("%s: the context and the block disagree on what the call serves" % who)
            return {'nwindow': self.stats['nwindow'] + self.nwin, 'nserved': self.stats['nserved'] + len(served),
                    'nexpired': self.stats['nexpired'] + len(expired), 'npending': len(queue.pending)}

        # (a span is nwin windows of acc_len samples of the beamformer's clock)
        loop.run(iseq, ihdr['seq0'], self.nwin * self.npair * self.nfine * 16, self.nwin * acc_len, ogulp_size,
                 lambda t: self.output_header(ihdr, t, tsamp), cut, before=pending, on_gap=gap)
