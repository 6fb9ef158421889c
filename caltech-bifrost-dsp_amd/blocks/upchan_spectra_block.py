"""UpchanSpectra: per-input fine-channel power and squared power, the input of the spectral-kurtosis estimator.

A further reader of the F-engine voltage ring, next to Beamform / Corr (live) or behind TbfSource -> Copy (a dump).  Each
coarse channel of each input is split into `nupchan` fine channels by an FFT over `nupchan` consecutive samples (one frame),
optionally behind the polyphase filter bank of pfb.py, and per input and fine channel the block emits, every `nframe_sum`
frames, S1 = sum |X|^2 and S2 = sum |X|^4 over the window (xengUpchanSpectra*, csrc/upchan_spectra_kernels.h): the
fine-resolution bandpass of every input and, through spectral_kurtosis.py, the per-input, per-channel interference flag.  The
block computes the product; acting on the flags is the consumer's business.  No reference counterpart: the reference has no
per-input fine-channel product and no interference statistic.

Windows: nframe_sum frames, W.  With F = ntime_gulp / nupchan frames per gulp, either W divides F (F / W windows in each output
span) or F divides W (one output span per W / F gulps).  Windows are aligned to the sequence's seq0.  A sequence start or a gap
(gulps this reader never saw) drops the window in progress and resets the context; after a gap the output restarts in a
sequence of its own at the next window boundary, and with a PFB the history is primed with the gulp right before that boundary
(UpchanSumBeams's state machine).

Input: u8 [ntime_gulp][nchan][ninput] spans (the Beamform input), whole or in two parts of whole frames.  Output: one span per
output unit,
  f32 [nwin][2][nchan][nupchan][ninput],  nwin = F / W (W | F) or 1 (F | W);  plane 0 = S1, plane 1 = S2
input = stand * npol + pol, as the header's input_to_ant says.  Fine channel j of coarse channel c is centred at
sfreq + c*d + (j - nupchan/2)*d/nupchan, d = bw_hz / nchan.
"""
import json
import time

from ..backend import default_backend
from .block_base import Block, InFlight, declare_streams, gulp_time, split_frames, spans_outlive_release
from .pfb import pfb_config

NUPCHAN = (1, 2, 4, 8, 16, 32, 64)


class UpchanSpectra(Block):
    STREAM_DEPTH = 4        # gulps whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, nchan, ninput, ntime_gulp, nupchan=32, nframe_sum=None, pfb_ntap=1, pfb_coeffs=None,
                 guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(UpchanSpectra, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        who = "UPCHAN_SPECTRA"
        if nupchan not in NUPCHAN:
            raise ValueError("%s: nupchan %r not one of %s" % (who, nupchan, NUPCHAN))
        if nchan <= 0 or ninput <= 0:
            raise ValueError("%s: %d channels x %d inputs" % (who, nchan, ninput))
        if ntime_gulp <= 0 or ntime_gulp % nupchan:
            raise ValueError("%s: gulps of %d samples are not whole frames of %d" % (who, ntime_gulp, nupchan))
        self.nframe = ntime_gulp // nupchan
        if nframe_sum is None:
            nframe_sum = self.nframe
        if nframe_sum <= 0 or (self.nframe % nframe_sum and nframe_sum % self.nframe):
            raise ValueError("%s: a window of %d frames neither divides nor is a whole number of %d-frame gulps" % (who, nframe_sum, self.nframe))
        self.pfb_ntap, pfb_h = pfb_config(who, pfb_ntap, pfb_coeffs, nupchan, ntime_gulp)
        self.pfb = pfb_h is not None            # (ntap 1 without coefficients: the plain FFT, no PFB call at all)
        self._bf = backend if backend is not None else default_backend()
        self.nchan, self.ninput, self.ntime_gulp, self.nupchan, self.gpu = nchan, ninput, ntime_gulp, nupchan, gpu
        self.nframe_sum = nframe_sum
        self.gulps_per_window = max(1, nframe_sum // self.nframe)
        self.windows_per_gulp = max(1, self.nframe // nframe_sum)
        self.acc_len = nframe_sum * nupchan
        declare_streams(iring, 'beam')          # (the kernel runs on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.update_stats({'nwindow': 0, 'ndropped': 0})
        rv = self._bf.upchan_spectra_initialize(self.gpu, ninput, nchan, ntime_gulp, nupchan, nframe_sum)
        if rv != self._bf.BF_STATUS_SUCCESS:
            raise RuntimeError("xengUpchanSpectraInitialize returned %d: %s" % (rv, self._bf.last_error()))
        if self.pfb:
            rv = self._bf.upchan_spectra_set_pfb(self.pfb_ntap, pfb_h)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("xengUpchanSpectraSetPfb returned %d: %s" % (rv, self._bf.last_error()))

    def output_header(self, ihdr, start):
        chan_bw = ihdr['bw_hz'] / self.nchan
        ohdr = ihdr.copy()
        ohdr.update(nupchan=self.nupchan, nframe_sum=self.nframe_sum, fine_bw_hz=chan_bw / self.nupchan, fine_sfreq=ihdr['sfreq'] - chan_bw / 2,
                    nbit=32, nmoment=2, acc_len=self.acc_len, seq0=start)
        ohdr.pop('complex', None)
        if self.pfb:
            ohdr['pfb_ntap'] = self.pfb_ntap
        return ohdr

    def main(self):
        self.bind()
        ogulp_size = self.windows_per_gulp * 2 * self.nchan * self.nupchan * self.ninput * 4
        self.oring.resize(ogulp_size)
        # In-repo rings keep a span's memory alive while it is referenced: several gulps in flight, each input span held until
        # ITS kernel has completed, each output span committed when its kernel has (tickets).  A bifrost ring: wait for the
        # kernel after every gulp.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.upchan_spectra_wait, self._bf.upchan_spectra_sync) as inflight, self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, oring, ogulp_size, streaming, inflight)

    def _drop(self, nlost, why):
        """Windows lost to gulps that were not read; the one in progress and the PFB history go with them."""
        self._bf.upchan_spectra_reset()
        self.update_stats({'ndropped': self.stats['ndropped'] + nlost})
        self.log.warning("UPCHAN_SPECTRA >> %d window(s) dropped: %s" % (nlost, why))

    def _enqueued(self, streaming, inflight, ospan, held):
        """After a launch: keep the gulp in flight, or wait for it."""
        if streaming:
            inflight.push(self._bf.upchan_spectra_mark(), ospan, held)
            inflight.retire(self.STREAM_DEPTH)
            return
        self._bf.upchan_spectra_sync()
        if ospan is not None:
            ospan.close()

    def _sequence(self, iseq, oring, ogulp_size, streaming, inflight):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        if ihdr['nchan'] != self.nchan or ihdr['nstand'] * ihdr['npol'] != self.ninput:
            raise ValueError("UPCHAN_SPECTRA: %d channels x %d inputs in the header, %d x %d configured" % (ihdr['nchan'], ihdr['nstand'] * ihdr['npol'],
                                                                                                          self.nchan, self.ninput))
        seq0 = ihdr['seq0']
        row = self.nchan * self.ninput
        igulp_size = self.ntime_gulp * row
        gpw = self.gulps_per_window
        read_parts = getattr(iseq, 'read_parts', None)
        this_gulp_time = seq0
        expected = seq0                         # the gulp that continues the window in progress
        pos = None                              # gulps of the window in progress; None: waiting for the next boundary
        oseq = None
        self._bf.upchan_spectra_reset()         # (a new sequence: what came before it counts as zero)
        try:
            prev_time = time.time()
            for ispan in (read_parts(igulp_size) if read_parts is not None else iseq.read(igulp_size)):
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
                parts = getattr(ispan, 'parts', None)
                two = parts is not None and len(parts) == 2
                held = parts if two else ispan.data
                ntime0 = split_frames(parts, row, self.nupchan, "UPCHAN_SPECTRA") if two else 0
                if pos is None:
                    k = (this_gulp_time - seq0) // self.ntime_gulp
                    if k % gpw:
                        if self.pfb_ntap > 1 and (k + 1) % gpw == 0:
                            # the next window's first frames see this gulp's tail
                            rv = self._bf.upchan_spectra_prime_parts(parts[0], ntime0, parts[1]) if two else self._bf.upchan_spectra_prime(held)
                            if rv != self._bf.BF_STATUS_SUCCESS:
                                raise RuntimeError("xengUpchanSpectraPrime returned %d: %s" % (rv, self._bf.last_error()))
                            self._enqueued(streaming, inflight, None, held)
                        continue                # (waiting for a window boundary)
                    pos = 0
                if oseq is None:
                    oseq = oring.begin_sequence(time_tag=this_gulp_time, header=json.dumps(self.output_header(ihdr, this_gulp_time)))
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                ospan = None
                try:
                    if pos == gpw - 1:          # this gulp completes a window (or F / W of them)
                        ospan = oseq.reserve(ogulp_size)
                    target = ospan.data if ospan is not None else None
                    if two:
                        rv = self._bf.upchan_spectra_run_parts(parts[0], ntime0, parts[1], target)
                    else:
                        rv = self._bf.upchan_spectra_run(held, target)
                    if rv != self._bf.BF_STATUS_SUCCESS:
                        raise RuntimeError("xengUpchanSpectraRun returned %d: %s" % (rv, self._bf.last_error()))
                    pos = (pos + 1) % gpw
                    if ospan is not None:
                        self.update_stats({'nwindow': self.stats['nwindow'] + self.windows_per_gulp,
                                           'last_end_sample': this_gulp_time + self.ntime_gulp})
                    osp, ospan = ospan, None
                    self._enqueued(streaming, inflight, osp, held)
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
