"""UpchanCorr: fine-channel visibilities from 4+4-bit F-engine data, FFT, frequency selection and correlation on the GPU.

Counterpart of the reference's upchannelised imager, pipeline/scripts/lwa352-upchan-imag.py:95-106: each coarse channel is
split into `nupchan` fine channels by an FFT over `nupchan` consecutive samples (one "frame"), the fine channels
[fine_lo, fine_hi) of the merged (coarse, fine) axis are kept (FrequencySelectBlock) and correlated, V = sum_f X_i conj(X_j),
over `nframe_per_integration` frames (blocks.correlate).  The selection is fused: unselected fine channels are never
correlated.  xengUpchanCorr* (csrc/upchan_corr_kernels.h) stage each gulp's fine channels and contract them on fp32 MFMAs.

Where it differs from the reference: fine channels ascend in frequency (fftshifted, as UpchanBeamform's); an
integration is a whole number of gulps, aligned to the sequence's seq0; the full Hermitian matrix is written; there is no HDF5
writer (VisibilitySaveBlock; h5py is not available).

pfb_ntap > 1 (or pfb_coeffs given; xengUpchanCorrSetPfb): the polyphase filter bank front end of UpchanBeamform (pfb.py),
y[f, n] = sum_k h[k*N + n] x[(f - P + 1 + k)*N + n] before each frame's FFT.  The history of the last (P - 1)*N samples
carries across gulps and across dumps (contiguous integrations continue the filter); it is reset at every sequence start and
at every gap.  While the block waits for an integration boundary after a gap it primes the history with the gulp right before
the boundary, so every frame of a written integration is a full PFB frame, except within P - 1 frames of seq0 or of a gap that
also took that gulp.  The header then carries `pfb_ntap`.

Input: u8 [ntime_gulp][nchan][ninput] spans (the Beamform input).  Output: one span per integration,
  cf32 [nfine][nstand][npol][nstand][npol],  V[c', s0, p0, s1, p1] = sum_f X[f, c', s0 p0] conj(X[f, c', s1 p1])
one output sequence per run of consecutive integrations, its header's seq0 the first one's start sample (as Corr's).  Merged
fine channel m = c*N + j is centred at sfreq + c*d + (j - N/2)*d/N, d = bw_hz / nchan.
"""
import json
import time

from ..backend import default_backend
from .block_base import Block, InFlight, declare_streams, gulp_time, split_frames, spans_outlive_release
from .pfb import pfb_config

NUPCHAN = (1, 2, 4, 8, 16, 32, 64)


class UpchanCorr(Block):
    STREAM_DEPTH = 4        # calls whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, nchan, ninput, ntime_gulp, nupchan, nframe_per_integration, fine_lo=0, fine_hi=None,
                 guarantee=True, core=-1, gpu=-1, backend=None, pfb_ntap=1, pfb_coeffs=None):
        super(UpchanCorr, self).__init__(log, iring, oring, guarantee, core, etcd_client=None)
        if fine_hi is None:
            fine_hi = nchan * nupchan
        if nupchan not in NUPCHAN:
            raise ValueError("UPCHAN_CORR: nupchan %d not one of %s" % (nupchan, NUPCHAN))
        if ntime_gulp <= 0 or ntime_gulp % nupchan:
            raise ValueError("UPCHAN_CORR: gulps of %d samples are not whole frames of %d" % (ntime_gulp, nupchan))
        self.nframe = ntime_gulp // nupchan
        if nframe_per_integration <= 0 or nframe_per_integration % self.nframe:
            raise ValueError("UPCHAN_CORR: an integration of %d frames is not a whole number of %d-frame gulps" % (nframe_per_integration, self.nframe))
        if not 0 <= fine_lo < fine_hi <= nchan * nupchan:
            raise ValueError("UPCHAN_CORR: fine channels [%d, %d) not a non-empty range within [0, %d)" % (fine_lo, fine_hi, nchan * nupchan))
        self.pfb_ntap, pfb_h = pfb_config("UPCHAN_CORR", pfb_ntap, pfb_coeffs, nupchan, ntime_gulp)
        self.pfb = pfb_h is not None            # (ntap 1 without coefficients: the plain FFT, no PFB call at all)
        self._bf = backend if backend is not None else default_backend()
        self.nchan, self.ninput, self.ntime_gulp, self.nupchan, self.gpu = nchan, ninput, ntime_gulp, nupchan, gpu
        self.nframe_per_integration = nframe_per_integration
        self.gulps_per_integration = nframe_per_integration // self.nframe
        self.acc_len = nframe_per_integration * nupchan
        self.fine_lo, self.fine_hi, self.nfine = fine_lo, fine_hi, fine_hi - fine_lo
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.update_stats({'nintegration': 0, 'ndropped': 0})
        rv = self._bf.upchan_corr_initialize(self.gpu, ninput, nchan, ntime_gulp, nupchan, fine_lo, fine_hi, 0)
        if rv != self._bf.BF_STATUS_SUCCESS:
            raise RuntimeError("xengUpchanCorrInitialize returned %d: %s" % (rv, self._bf.last_error()))
        if self.pfb:
            rv = self._bf.upchan_corr_set_pfb(self.pfb_ntap, pfb_h)
            if rv != self._bf.BF_STATUS_SUCCESS:
                raise RuntimeError("xengUpchanCorrSetPfb returned %d: %s" % (rv, self._bf.last_error()))

    def output_header(self, ihdr, start):
        chan_bw = ihdr['bw_hz'] / self.nchan
        m = self.fine_lo
        ohdr = ihdr.copy()
        ohdr.update(nupchan=self.nupchan, fine_lo=self.fine_lo, nfine=self.nfine, fine_bw_hz=chan_bw / self.nupchan,
                    fine_sfreq=ihdr['sfreq'] + (m // self.nupchan) * chan_bw + (m % self.nupchan - self.nupchan // 2) * chan_bw / self.nupchan,
                    nframe_per_integration=self.nframe_per_integration, acc_len=self.acc_len, complex=True, nbit=32, seq0=start)
        if self.pfb:
            ohdr['pfb_ntap'] = self.pfb_ntap
        return ohdr

    def main(self):
        self.bind()
        ogulp_size = self.nfine * self.ninput * self.ninput * 8
        self.oring.resize(ogulp_size)
        # In-repo rings keep a span's memory alive while it is referenced: several calls in flight, each input span held until
        # ITS stage kernel has completed, each output span committed when ITS dump kernel has (tickets).  A bifrost ring: wait
        # for the kernels after every gulp.
        streaming = spans_outlive_release(self.iring, self.oring)
        with InFlight(self._bf.upchan_corr_wait, self._bf.upchan_corr_sync) as inflight, self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, oring, ogulp_size, streaming, inflight)

    def _drop(self, nlost, reset, why):
        """Integrations lost to gulps that were not read; the one in progress (reset) leaves nothing in the next one.  With a
        PFB history the reset is made in any case: the samples before the gap are not the ones before the next gulp."""
        if reset:
            self._bf.upchan_corr_reset()
        self.update_stats({'ndropped': self.stats['ndropped'] + nlost})
        self.log.warning("UPCHAN_CORR >> %d integration(s) dropped: %s" % (nlost, why))

    def _prime(self, ispan, row, streaming, inflight):
        """The PFB history from this gulp's tail, nothing accumulated; the input is held until the copies have run."""
        parts = getattr(ispan, 'parts', None)
        if parts is not None and len(parts) == 2:
            held = parts
            rv = self._bf.upchan_corr_prime_parts(parts[0], split_frames(parts, row, self.nupchan, "UPCHAN_CORR"), parts[1])
        else:
            held = ispan.data
            rv = self._bf.upchan_corr_prime(held)
        if rv != self._bf.BF_STATUS_SUCCESS:
            raise RuntimeError("xengUpchanCorrPrime returned %d: %s" % (rv, self._bf.last_error()))
        if streaming:
            inflight.push(self._bf.upchan_corr_mark(), None, held)
            inflight.retire(self.STREAM_DEPTH)
        else:
            self._bf.upchan_corr_sync()

    def _sequence(self, iseq, oring, ogulp_size, streaming, inflight):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        if ihdr['nchan'] != self.nchan or ihdr['nstand'] * ihdr['npol'] != self.ninput:
            raise ValueError("UPCHAN_CORR: %d channels x %d inputs in the header, %d x %d configured" % (ihdr['nchan'], ihdr['nstand'] * ihdr['npol'],
                                                                                                       self.nchan, self.ninput))
        seq0 = ihdr['seq0']
        row = self.nchan * self.ninput
        igulp_size = self.ntime_gulp * row
        gpi = self.gulps_per_integration
        read_parts = getattr(iseq, 'read_parts', None)
        this_gulp_time = seq0
        expected = seq0                         # the gulp that continues the integration in progress
        pos = None                              # gulps of the integration in progress; None: waiting for the next boundary
        oseq = None
        if self.pfb_ntap > 1:
            self._bf.upchan_corr_reset()        # (a new sequence: what came before it counts as zero)
        try:
            prev_time = time.time()
            for ispan in (read_parts(igulp_size) if read_parts is not None else iseq.read(igulp_size)):
                if ispan.size < igulp_size:
                    continue                    # a short final gulp is skipped (as the reference's gulp_nframe reader does)
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, self.ntime_gulp, this_gulp_time)
                if this_gulp_time != expected:
                    # gulps this reader never saw: an integration they belonged to is lost, and the output realigns to the
                    # next boundary in a sequence of its own (as Corr does)
                    # (lost: every integration that overlaps the samples not read, but one already given up while waiting)
                    k_lo = (expected - seq0) // self.acc_len + (1 if pos is None and (expected - seq0) % self.acc_len else 0)
                    k_hi = (this_gulp_time - 1 - seq0) // self.acc_len
                    self._drop(max(0, k_hi - k_lo + 1), bool(pos) or self.pfb_ntap > 1, "samples [%d, %d) were not read" % (expected, this_gulp_time))
                    pos = None
                    if oseq is not None:
                        inflight.retire(0)
                        oseq.end()
                        oseq = None
                expected = this_gulp_time + self.ntime_gulp
                self.update_stats({'curr_sample': this_gulp_time})
                if pos is None:
                    k = (this_gulp_time - seq0) // self.ntime_gulp
                    if k % gpi:
                        if self.pfb_ntap > 1 and (k + 1) % gpi == 0:
                            self._prime(ispan, row, streaming, inflight)    # (the next integration's first frames see its tail)
                        continue                # (waiting for an integration boundary)
                    pos = 0
                if oseq is None:
                    oseq = oring.begin_sequence(time_tag=this_gulp_time, header=json.dumps(self.output_header(ihdr, this_gulp_time)))
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                parts = getattr(ispan, 'parts', None)
                if parts is not None and len(parts) == 2:
                    ntime0 = split_frames(parts, row, self.nupchan, "UPCHAN_CORR")
                    held = parts
                    rv = self._bf.upchan_corr_accumulate_parts(parts[0], ntime0, parts[1])
                else:
                    held = ispan.data
                    rv = self._bf.upchan_corr_accumulate(held)
                if rv != self._bf.BF_STATUS_SUCCESS:
                    raise RuntimeError("xengUpchanCorrAccumulate returned %d: %s" % (rv, self._bf.last_error()))
                pos += 1
                ospan = None
                try:
                    if pos == gpi:
                        ospan = oseq.reserve(ogulp_size)
                        rv = self._bf.upchan_corr_dump(ospan.data)
                        if rv != self._bf.BF_STATUS_SUCCESS:
                            raise RuntimeError("xengUpchanCorrDump returned %d: %s" % (rv, self._bf.last_error()))
                        pos = 0
                        self.update_stats({'nintegration': self.stats['nintegration'] + 1, 'last_end_sample': this_gulp_time + self.ntime_gulp})
                    if streaming:
                        inflight.push(self._bf.upchan_corr_mark(), ospan, held)
                        ospan = None
                        inflight.retire(self.STREAM_DEPTH)
                    else:
                        self._bf.upchan_corr_sync()
                finally:
                    if ospan is not None:
                        ospan.close()
                curr_time = time.time()
                process_time = curr_time - prev_time
                prev_time = curr_time
                self.perf_proclog.update({'acquire_time': acquire_time, 'reserve_time': 0.0, 'process_time': process_time})
            if pos:                             # (the sequence ends inside an integration: it is not written)
                self._bf.upchan_corr_reset()
        finally:
            inflight.retire(0)                  # every call in flight is complete (and every output span committed) first
            if oseq is not None:
                oseq.end()
