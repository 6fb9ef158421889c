"""UpchanSumBeams: fine-channel dual-pol power beams from the live voltage beams.

A third reader of Beamform's output ring, beside BeamformSumBeams and BeamformVlbiOutput.  Each coarse channel of each beam is
split into `nupchan` fine channels by an FFT over `nupchan` consecutive samples (one frame), optionally behind the polyphase
filter bank of pfb.py, and beams 2p / 2p+1 of the pairs [pair0, pair0 + npair) are taken as X / Y: every `nframe_sum` frames
it emits [XX, YY, Re(XY*), Im(XY*)] per fine channel (xengUpchanSumBeams*, csrc/upchan_beams_kernels.h).  In exact arithmetic
this is UpchanBeamform's dual-pol output with the coarse weights copied to every fine channel (beamforming, the PFB and the FFT
are linear), at one FFT per beam instead of one per input.  No reference counterpart: the reference's fine-channel beams are
offline only.

Windows: nframe_sum frames, W.  With F = ntime_gulp / nupchan frames per gulp, either W divides F (F / W windows in each
output span) or F divides W (one output span per W / F gulps).  Windows are aligned to the sequence's seq0.  A sequence start
or a gap (gulps this reader never saw) drops the window in progress and resets the context; after a gap the output restarts
in a sequence of its own at the next window boundary, and with a PFB the history is primed with the gulp right before that
boundary (UpchanCorr's state machine).

Input: Beamform's voltage spans, cf32 [nchan][nbeam][ntime_gulp], whole gulps.  Output: one span per output unit,
  f32 [nwin][npair][nchan][nupchan][4],  nwin = F / W (W | F) or 1 (F | W)
the layout of UpchanBeamform's dual-pol output.  Fine channel j of coarse channel c is centred at
sfreq + c*d + (j - nupchan/2)*d/nupchan, d = bw_hz / nchan.
"""
import json
import time

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray
from .block_base import Block, InFlight, declare_streams, gulp_time, spans_outlive_release
from .pfb import pfb_config

NUPCHAN = (8, 16, 32, 64)


class UpchanSumBeams(Block):
    STREAM_DEPTH = 4        # gulps whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, nchan, nbeam, ntime_gulp, nupchan=32, nframe_sum=None, pair0=0, npair=None, pfb_ntap=1,
                 pfb_coeffs=None, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanSumBeams, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_SUM_BEAMS"
        if nupchan not in NUPCHAN:
            raise ValueError("%s: nupchan %r not one of %s" % (who, nupchan, NUPCHAN))
        if ntime_gulp <= 0 or ntime_gulp % nupchan:
            raise ValueError("%s: gulps of %d samples are not whole frames of %d" % (who, ntime_gulp, nupchan))
        self.nframe = ntime_gulp // nupchan
        if nframe_sum is None:
            nframe_sum = self.nframe
        if nframe_sum <= 0 or (self.nframe % nframe_sum and nframe_sum % self.nframe):
            raise ValueError("%s: a window of %d frames neither divides nor is a whole number of %d-frame gulps" % (who, nframe_sum, self.nframe))
        if npair is None:
            npair = nbeam // 2 - pair0
        if nchan <= 0 or pair0 < 0 or npair <= 0 or pair0 + npair > nbeam // 2:
            raise ValueError("%s: pairs [%d, %d) not a non-empty range of the %d pairs of %d beams" % (who, pair0, pair0 + npair, nbeam // 2, nbeam))
        self.pfb_ntap, pfb_h = pfb_config(who, pfb_ntap, pfb_coeffs, nupchan, ntime_gulp)
        self.pfb = pfb_h is not None            # (ntap 1 without coefficients: the plain FFT, no PFB call at all)
        self._bf = backend if backend is not None else default_backend()
        self.nchan, self.nbeam, self.ntime_gulp, self.nupchan, self.gpu = nchan, nbeam, ntime_gulp, nupchan, gpu
        self.nframe_sum, self.pair0, self.npair = nframe_sum, pair0, npair
        self.gulps_per_window = max(1, nframe_sum // self.nframe)
        self.windows_per_gulp = max(1, self.nframe // nframe_sum)
        self.acc_len = nframe_sum * nupchan
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.update_stats({'nwindow': 0, 'ndropped': 0})
        rv = self._bf.upchan_sum_beams_initialize(self.gpu, nchan, nbeam, ntime_gulp, nupchan, pair0, npair, nframe_sum)
        if rv != self._bf.BF_STATUS_SUCCESS:
            raise RuntimeError("xengUpchanSumBeamsInitialize returned %d: %s" % (rv, self._bf.last_error()))
        if self.pfb:
            rv = self._bf.upchan_sum_beams_set_pfb(self.pfb_ntap, pfb_h)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("xengUpchanSumBeamsSetPfb returned %d: %s" % (rv, self._bf.last_error()))

    def output_header(self, ihdr, start):
        chan_bw = ihdr['bw_hz'] / self.nchan
        ohdr = ihdr.copy()
        ohdr.update(nstand=self.npair, nbeam=self.npair, npol=2, complex=True, nbit=32, nupchan=self.nupchan, nframe_sum=self.nframe_sum,
                    fine_bw_hz=chan_bw / self.nupchan, fine_sfreq=ihdr['sfreq'] - chan_bw / 2, pair0=self.pair0, acc_len=self.acc_len, seq0=start)
        if self.pfb:
            ohdr['pfb_ntap'] = self.pfb_ntap
        return ohdr

    def _check_header(self, ihdr):
        """Beamform's voltage output only: not the products of another reader.  (Beamform's experimental ntime_sum output has its
        voltage output's header keys: nothing in a header tells the two apart, so a pipeline must not wire that one here.)"""
        if ihdr.get('nchan') != self.nchan or ihdr.get('nbeam') != self.nbeam:
            raise ValueError("UPCHAN_SUM_BEAMS: %r channels x %r beams in the header, %d x %d configured" % (ihdr.get('nchan'), ihdr.get('nbeam'),
                                                                                                           self.nchan, self.nbeam))
        if ihdr.get('nbit') != 32 or not ihdr.get('complex') or ihdr.get('npol') != 1:
            raise ValueError("UPCHAN_SUM_BEAMS: the input is not single-pol cf32 voltage beams (nbit %r, complex %r, npol %r)"
                             % (ihdr.get('nbit'), ihdr.get('complex'), ihdr.get('npol')))
        for k in ('acc_len', 'ntime_sum', 'nupchan'):
            if k in ihdr:
                raise ValueError("UPCHAN_SUM_BEAMS: the input carries '%s': integrated or channelised products, not voltage beams" % k)

    def main(self):
        self.bind()
        self._oshape = (self.windows_per_gulp, self.npair, self.nchan, self.nupchan, 4)
        ogulp_size = int(np.prod(self._oshape)) * 4
        self.oring.resize(ogulp_size)
        # Streaming (in-repo rings): up to STREAM_DEPTH gulps in flight, each input held until ITS kernel has completed, each
        # output committed when its kernel (and copy) has.  On a bifrost ring: wait for the kernel after every gulp.
        # A pinned-host output ring (as the live power beams' is): the kernel writes a device buffer and the copy stream moves it
        # once the kernel's ticket is done -- a kernel that stores across PCIe holds the beamformer's stream for the length of
        # the transfer.  The calls and copies in flight are InFlight's (block_base.py).
        streaming = spans_outlive_release(self.iring, self.oring)
        self._staged = streaming and self.oring.space == 'cuda_host' and hasattr(self._bf, 'copy_async')
        self._dev = None if streaming else XArray(shape=self._oshape, dtype=np.float32, space=self._bf.space_in)
        with InFlight(self._bf.upchan_sum_beams_wait, self._bf.upchan_sum_beams_sync, self._bf) as inflight, self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, oring, ogulp_size, streaming, inflight)

    def _drop(self, nlost, why):
        """Windows lost to gulps that were not read; the one in progress and the PFB history go with them."""
        self._bf.upchan_sum_beams_reset()
        self.update_stats({'ndropped': self.stats['ndropped'] + nlost})
        self.log.warning("UPCHAN_SUM_BEAMS >> %d window(s) dropped: %s" % (nlost, why))

    def _enqueued(self, streaming, inflight, ospan, held, stage):
        """After a launch: keep the gulp in flight, or wait for it and hand the output over."""
        if streaming:
            inflight.push(self._bf.upchan_sum_beams_mark(), ospan, held, stage)
            inflight.retire(self.STREAM_DEPTH)
            return
        self._bf.upchan_sum_beams_sync()
        if ospan is not None:
            try:
                ospan.data_view(np.float32).reshape(self._oshape)[...] = self._dev      # (synchronous copy)
            finally:
                ospan.close()

    def _sequence(self, iseq, oring, ogulp_size, streaming, inflight):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        self._check_header(ihdr)
        seq0 = ihdr['seq0']
        igulp_size = self.nchan * self.nbeam * self.ntime_gulp * 8
        gpw = self.gulps_per_window
        this_gulp_time = seq0
        expected = seq0                         # the gulp that continues the window in progress
        pos = None                              # gulps of the window in progress; None: waiting for the next boundary
        oseq = None
        self._bf.upchan_sum_beams_reset()       # (a new sequence: what came before it counts as zero)
        try:
            prev_time = time.time()
            for ispan in iseq.read(igulp_size):
                if ispan.size < igulp_size:
                    continue                    # a short final gulp is skipped (as the reference's gulp_nframe reader does)
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, self.ntime_gulp, this_gulp_time)
                if this_gulp_time != expected:
                    # lost: every window that overlaps the samples not read, but one already given up while waiting
                    k_lo = (expected - seq0) // self.acc_len + (1 if pos is None and (expected - seq0) % self.acc_len else 0)
                    k_hi = (this_gulp_time - 1 - seq0) // self.acc_len
                    self._drop(max(0, k_hi - k_lo + 1), "samples [%d, %d) were not read" % (expected, this_gulp_time))
                    pos = None
                    if oseq is not None:
                        inflight.retire(0)
                        oseq.end()
                        oseq = None
                expected = this_gulp_time + self.ntime_gulp
                self.update_stats({'curr_sample': this_gulp_time})
                held = ispan.data
                if pos is None:
                    k = (this_gulp_time - seq0) // self.ntime_gulp
                    if k % gpw:
                        if self.pfb_ntap > 1 and (k + 1) % gpw == 0:
                            # the next window's first frames see this gulp's tail
                            rv = self._bf.upchan_sum_beams_prime(held)
                            if rv != self._bf.BF_STATUS_SUCCESS:
                                raise RuntimeError("xengUpchanSumBeamsPrime returned %d: %s" % (rv, self._bf.last_error()))
                            self._enqueued(streaming, inflight, None, held, None)
                        continue                # (waiting for a window boundary)
                    pos = 0
                if oseq is None:
                    oseq = oring.begin_sequence(time_tag=this_gulp_time, header=json.dumps(self.output_header(ihdr, this_gulp_time)))
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                ospan = stage = None
                try:
                    target = None
                    if pos == gpw - 1:          # this gulp completes a window (or F / W of them)
                        ospan = oseq.reserve(ogulp_size)
                        if self._staged:
                            stage = inflight.take_stage(ogulp_size)
                        target = stage if stage is not None else (ospan.data if streaming else self._dev)
                    rv = self._bf.upchan_sum_beams_run(held, target)
                    if rv != self._bf.BF_STATUS_SUCCESS:
                        raise RuntimeError("xengUpchanSumBeamsRun returned %d: %s" % (rv, self._bf.last_error()))
                    pos = (pos + 1) % gpw
                    if ospan is not None:
                        self.update_stats({'nwindow': self.stats['nwindow'] + self.windows_per_gulp,
                                           'last_end_sample': this_gulp_time + self.ntime_gulp})
                    osp, ospan = ospan, None
                    self._enqueued(streaming, inflight, osp, held, stage)
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
