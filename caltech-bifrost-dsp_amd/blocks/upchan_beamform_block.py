"""UpchanBeamform: fine-channel beams from 4+4-bit F-engine data, FFT and beamforming fused in one HIP kernel.

Counterpart of the reference's upchannelising beamformer, pipeline/scripts/lwa352-upchan-bf.py:94-113 with
pipeline/lwa352_pipeline/blocks/beamform_offline_block.py (weights :110-138, per-gulp work :211-245): each coarse channel is
split into `nupchan` fine channels by an FFT over `nupchan` consecutive samples (one "frame"), weighted per fine channel and
summed over inputs (xengUpchanRun, csrc/upchan_kernels.h; the channelised data never reaches device memory).

Where it differs from the reference: the block takes Beamform's `coeffs` commands (delays in ns, amplitudes,
timed `load_sample`) instead of pointing from RA/Dec, with calibration at fine resolution; the amplitude multiplies the
weight (the reference scales the delay by it, :137); every beam is formed (the reference's TODO at :214-215); the power mode
writes |v|^2 summed over frames (the reference's output writes np.abs(v)).

dual_pol=True (nframe_sum > 0, nbeam even; xengUpchanInitializeDualPol): beams 2p / 2p+1 are the X / Y pols of pair p, and
the block emits their 2x2 products per fine channel, [XX, YY, Re(XY*), Im(XY*)] summed over each window, as BeamformSumBeams
does for the coarse-channel beams (beamform_sum_beams_block.py; the reference's beamformer_sum_test.py:64-77).  The commands
are unchanged: `beamcoeffs` / `calgains` of beam_id 2p steer X and of 2p+1 steer Y, so Jones-mixed weights (both pols of every
stand feeding each output pol) stay possible.  XX / YY are bit-identical to the power mode's outputs of beams 2p / 2p+1.

pfb_ntap > 1 (or pfb_coeffs given; xengUpchanSetPfb): a polyphase filter bank front end, y[f, n] = sum_k h[k*N + n]
x[(f - P + 1 + k)*N + n] before each frame's FFT, so that a tone between fine channels no longer leaks into the whole coarse
channel.  The default coefficients are pfb.pfb_coeffs (sinc * Hamming, sum N).  The history of the last (P - 1)*N samples is
kept on the device across gulps: it is reset at every sequence start and whenever a gulp does not follow the previous one
(gulp_time), so that the samples not seen count as zero.  The header then carries `pfb_ntap`.  No reference counterpart.

Input: u8 [ntime_gulp][nchan][ninput] spans (the Beamform input).  Output per gulp:
  nframe_sum = 0: cf32 [nframe][nbeam][nchan][nupchan]          (nframe = ntime_gulp / nupchan)
  nframe_sum > 0: f32  [nframe / nframe_sum][nbeam][nchan][nupchan]
  dual_pol:       f32  [nframe / nframe_sum][nbeam / 2][nchan][nupchan][4]   (header nbeam = nstand = nbeam / 2, npol = 2)
Fine channel j of coarse channel c is centred at sfreq + c*d + (j - nupchan/2)*d/nupchan, d = bw_hz / nchan.
"""
import json
import time

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray
from ..proclog import cpu_affinity
from .block_base import Block, COMMAND_INVALID, COMMAND_OK, InFlight, declare_streams, gulp_time, split_frames, spans_outlive_release
from .pfb import pfb_config


class UpchanBeamform(Block):
    STREAM_DEPTH = 4        # gulps whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, nchan=256, nbeam=1, ninput=352 * 2, ntime_gulp=2500, nupchan=32, nframe_sum=0,
                 guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None, dual_pol=False, pfb_ntap=1, pfb_coeffs=None):
        super(UpchanBeamform, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        if dual_pol and (nbeam % 2 or not nframe_sum):
            raise ValueError("UPCHAN: dual_pol needs an even nbeam (X / Y pairs; %d given) and nframe_sum > 0 (%d given)" % (nbeam, nframe_sum))
        self.dual_pol = bool(dual_pol)
        self._bf = backend if backend is not None else default_backend()
        self.nchan, self.nbeam, self.ninput, self.ntime_gulp = nchan, nbeam, ninput, ntime_gulp
        self.nupchan, self.nframe_sum, self.gpu = nupchan, nframe_sum, gpu
        if ntime_gulp % nupchan or (nframe_sum and (ntime_gulp // nupchan) % nframe_sum):
            raise ValueError("UPCHAN: gulps of %d samples are not whole frames of %d (or windows of %d frames)" % (ntime_gulp, nupchan, nframe_sum))
        self.nframe = ntime_gulp // nupchan
        self.pfb_ntap, pfb_h = pfb_config("UPCHAN", pfb_ntap, pfb_coeffs, nupchan, ntime_gulp)
        self.pfb = pfb_h is not None            # (ntap 1 without coefficients: the plain FFT, no PFB call at all)
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.freqs = np.zeros((nchan, nupchan))  # fine-channel centres, set from each sequence header
        shape = (nchan, nupchan, nbeam, ninput)
        # weights: latest commanded (new) -> active on the host (cpu) -> on the device (gpu), per beam at its load sample
        self.cal_gains = np.ones(shape, dtype=np.complex64)
        self.weights_new = np.zeros(shape, dtype=np.complex64)
        self.weights_cpu = np.zeros(shape, dtype=np.complex64)
        self.weights_gpu = XArray(shape=shape, dtype=np.complex64, space=self._bf.space_in)
        self.weights_load_sample = np.zeros(nbeam)
        self._weights_version = 0
        self.define_command_key('coeffs', type=dict, initial_val={})
        for b in range(nbeam):
            self.update_stats({'cal_gains%d' % b: [False, ] * ninput})
        if self.dual_pol:
            rv = self._bf.upchan_initialize_dual_pol(self.gpu, ninput, nchan, ntime_gulp, nupchan, nbeam, nframe_sum)
        else:
            rv = self._bf.upchan_initialize(self.gpu, ninput, nchan, ntime_gulp, nupchan, nbeam, nframe_sum)
        if rv != self._bf.BF_STATUS_SUCCESS:
            raise RuntimeError("xengUpchanInitialize%s returned %d: %s" % ("DualPol" if self.dual_pol else "", rv, self._bf.last_error()))
        if self.pfb:
            rv = self._bf.upchan_set_pfb(self.pfb_ntap, pfb_h)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("xengUpchanSetPfb returned %d: %s" % (rv, self._bf.last_error()))

    def _etcd_callback(self, watchresponse):
        """Every command is enacted as it arrives (all share the `coeffs` key, as Beamform's do)."""
        cpu_affinity.set_core(self.core)
        self.acquire_control_lock()
        try:
            for event in watchresponse.events:
                try:
                    seq_id, kwargs = self._parse_event(event)
                except ValueError:
                    self.log.exception("UPCHAN >> Failed to JSON-decode event %s" % str(event.value))
                    self._send_command_response("0", False, "JSON-decode failed!")
                    continue
                if kwargs is None:
                    continue
                try:
                    proc_ok = self._process_commands(kwargs, set_pending_flag=False)
                except Exception:
                    proc_ok = COMMAND_INVALID
                self.update_stats({'last_cmd_response': proc_ok})
                self.update_command_vals()
                self._send_command_response(seq_id, proc_ok == COMMAND_OK, str(proc_ok))
        finally:
            self.release_control_lock()

    def update_command_vals(self):
        """`calgains`: 2 * nchan * nupchan floats (re, im interleaved, channel-major) per (beam, input).  `beamcoeffs`: the weight
        amps * exp(2 pi i f tau 1e-9) * cal at every fine frequency f (Beamform's formula, beamform_block.py:340-342), active from
        its `load_sample` on (-1 or absent: the next gulp)."""
        cpu_affinity.set_core(self.core)
        self.command_vals.update(self._pending_command_vals)
        update_beam_cal_state = False
        for k, v in self._pending_command_vals.items():
            try:
                if not v:
                    continue
                if v['type'] == 'calgains':
                    i, b = v['input_id'], v['beam_id']
                    data = np.asarray(v['data'], dtype=np.float64)
                    if data.size != 2 * self.nchan * self.nupchan:
                        self.log.error("UPCHAN >> calgains need %d values, got %d" % (2 * self.nchan * self.nupchan, data.size))
                        continue
                    self.cal_gains[:, :, b, i] = (data[0::2] + 1j * data[1::2]).reshape(self.nchan, self.nupchan)
                    self.stats['cal_gains%d' % b][i] = True
                    update_beam_cal_state = True
                if v['type'] == 'beamcoeffs':
                    b = v['beam_id']
                    delays_ns = np.asarray(v['data']['delays'], dtype=np.float64)
                    amps = np.asarray(v['data']['amps'], dtype=np.float64)
                    phases = np.exp(2j * np.pi * self.freqs[:, :, None] * delays_ns[None, None, :] * 1e-9)     # chan x fine x input
                    self.weights_new[:, :, b, :] = amps * phases * self.cal_gains[:, :, b, :]
                    self.weights_load_sample[b] = v.get('load_sample', -1)
                    self.update_pending = True
            except KeyError:
                self.log.error("UPCHAN >> Failed to parse command")
        self.update_stats(self.command_vals)
        if update_beam_cal_state:
            self.update_stats({'cal_gains%d' % b: self.stats['cal_gains%d' % b] for b in range(self.nbeam)})

    def _load_pending_weights(self, this_gulp_time):
        """Weights whose load sample has come move from `new` to `cpu`; True when the device copy has to be rewritten."""
        copy_pending = False
        self.acquire_control_lock()
        for b in range(self.nbeam):
            if self.weights_load_sample[b] == 0:    # 0 = nothing pending for this beam
                continue
            if this_gulp_time >= self.weights_load_sample[b]:
                self.weights_cpu[:, :, b, :] = self.weights_new[:, :, b, :]
                self.weights_load_sample[b] = 0
                copy_pending = True
        if self.weights_load_sample.sum() == 0:
            self.update_pending = False
        self.stats['update_pending'] = self.update_pending
        self.stats['last_cmd_proc_time'] = time.time()
        self.release_control_lock()
        return copy_pending

    def output_header(self, ihdr):
        chan_bw = ihdr['bw_hz'] / self.nchan
        ohdr = ihdr.copy()
        ohdr.update(nstand=self.nbeam, nbeam=self.nbeam, nupchan=self.nupchan, nframe_sum=self.nframe_sum, nbit=32, npol=1,
                    fine_bw_hz=chan_bw / self.nupchan, fine_sfreq=ihdr['sfreq'] - chan_bw / 2)
        if self.dual_pol:                       # (the keys BeamformSumBeams sets on the live power beams)
            ohdr.update(nstand=self.nbeam // 2, nbeam=self.nbeam // 2, npol=2, complex=True)
        elif self.nframe_sum:
            ohdr.pop('complex', None)
        else:
            ohdr['complex'] = True
        if self.pfb:
            ohdr['pfb_ntap'] = self.pfb_ntap
        return ohdr

    def main(self):
        self.bind()
        nout = self.nframe // self.nframe_sum if self.nframe_sum else self.nframe
        if self.dual_pol:
            ogulp_size = nout * (self.nbeam // 2) * self.nchan * self.nupchan * 16
        else:
            ogulp_size = nout * self.nbeam * self.nchan * self.nupchan * (4 if self.nframe_sum else 8)
        self.oring.resize(ogulp_size)
        # In-repo rings keep a span's memory alive while it is referenced: several gulps in flight, each output span committed
        # when ITS kernel has completed (tickets).  A bifrost ring: wait for the kernel after every gulp.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.upchan_wait, self._bf.upchan_sync) as inflight, self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, oring, ogulp_size, streaming, inflight)

    def _sequence(self, iseq, oring, ogulp_size, streaming, inflight):
        self.update_pending = True
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        if ihdr['nchan'] != self.nchan or ihdr['nstand'] * ihdr['npol'] != self.ninput:
            raise ValueError("UPCHAN: %d channels x %d inputs in the header, %d x %d configured" % (ihdr['nchan'], ihdr['nstand'] * ihdr['npol'],
                                                                                                  self.nchan, self.ninput))
        chan_bw = ihdr['bw_hz'] / self.nchan
        self.freqs = (ihdr['sfreq'] + chan_bw * np.arange(self.nchan)[:, None]
                      + (np.arange(self.nupchan)[None, :] - self.nupchan // 2) * chan_bw / self.nupchan)
        seq0 = ihdr['seq0']
        row = self.nchan * self.ninput
        igulp_size = self.ntime_gulp * row
        read_parts = getattr(iseq, 'read_parts', None)
        copy_pending = True
        this_gulp_time = seq0
        expected = None                         # (PFB) the gulp that continues the history: none at the sequence's start
        with oring.begin_sequence(time_tag=iseq.time_tag, header=json.dumps(self.output_header(ihdr))) as oseq:
            prev_time = time.time()
            for ispan in (read_parts(igulp_size) if read_parts is not None else iseq.read(igulp_size)):
                if ispan.size < igulp_size:
                    continue                    # a short final gulp is skipped (as the reference's gulp_nframe reader does)
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, self.ntime_gulp, this_gulp_time)
                self.update_stats({'curr_sample': this_gulp_time})
                if self.pfb_ntap > 1:
                    if this_gulp_time != expected:
                        self._bf.upchan_reset()     # (a new sequence, or gulps not read: what came before counts as zero)
                    expected = this_gulp_time + self.ntime_gulp
                if self.update_pending:
                    copy_pending = self._load_pending_weights(this_gulp_time) or copy_pending
                if copy_pending:
                    inflight.retire(0)          # (kernels in flight may still read the device copy of the weights)
                    self.weights_gpu[...] = self.weights_cpu
                    self._weights_version += 1
                    copy_pending = False
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                ospan = oseq.reserve(ogulp_size)
                try:
                    parts = getattr(ispan, 'parts', None)
                    if parts is not None and len(parts) == 2:
                        ntime0 = split_frames(parts, row, self.nupchan, "UPCHAN")
                        held = parts
                        rv = self._bf.upchan_run_parts(parts[0], ntime0, parts[1], ospan.data, self.weights_gpu, self._weights_version)
                    else:
                        held = ispan.data
                        rv = self._bf.upchan_run(held, ospan.data, self.weights_gpu, self._weights_version)
                    if rv != self._bf.BF_STATUS_SUCCESS:
                        raise RuntimeError("xengUpchanRun returned %d: %s" % (rv, self._bf.last_error()))
                    if streaming:
                        inflight.push(self._bf.upchan_mark(), ospan, held)
                        ospan = None
                        inflight.retire(self.STREAM_DEPTH)
                    else:
                        self._bf.upchan_sync()
                finally:
                    if ospan is not None:
                        ospan.close()
                self.update_stats({'last_end_sample': this_gulp_time})
                this_gulp_time += self.ntime_gulp
                curr_time = time.time()
                process_time = curr_time - prev_time
                prev_time = curr_time
                self.perf_proclog.update({'acquire_time': acquire_time, 'reserve_time': 0.0, 'process_time': process_time})
            inflight.retire(0)                  # the sequence ends: every gulp in flight is committed first
