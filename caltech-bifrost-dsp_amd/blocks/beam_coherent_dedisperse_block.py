"""BeamCoherentDedisperse: coherent dedispersion of the live voltage beams.

A further reader of Beamform's output ring, beside UpchanSumBeams and BeamformVlbiOutput, that writes a ring of the same format:
every coarse channel of the beams 2p / 2p+1 of the pairs [pair0, pair0 + npair) is filtered by overlap-save with the chirp of the
pair's DM (coherent_dedisp.chirp_table; xengCdedisp*, csrc/cdedisp_kernels.h; the definition is in include/xeng.h), which aligns
every frequency inside a coarse channel to the channel's centre.  The delays BETWEEN the coarse channels stay in the data, for
BeamDedisperse or BeamFold behind an UpchanSumBeams.  No reference counterpart.

Input: Beamform's voltage spans, cf32 [nchan][nbeam][ntime_gulp], whole gulps.  Output: one span per filter block,
  cf32 [nchan][2 npair][L],   L = nfft - overlap
Block j of a stream covers the input samples [j L, j L + nfft) counted from the stream's first sample, and its span holds the
samples j L + overlap/2 ... of it: output sample i is input sample i + overlap/2, and the spans tile the time axis.  ntime_gulp
and L need not divide one another: a gulp completes between 0 and ceil(ntime_gulp / L) blocks, and the block counts samples itself
to know how many spans to reserve.  The output header is the input's with nbeam = nstand = 2 npair, pair0, seq0 (the first sample
the sequence holds), cdedisp_dm (one per pair), cdedisp_nfft and cdedisp_overlap; it carries none of acc_len, ntime_sum, nupchan, so
UpchanSumBeams(nbeam=2 npair, ntime_gulp=L) and BeamformVlbiOutput read it as they read Beamform's.

nfft and overlap: both given, or both None: then cdedisp_plan chooses them at the first sequence from the header's band and the
largest |DM| of `dms`, with a step that is a multiple of `multiple_of` (the nupchan of an UpchanSumBeams behind this block).

Sequence, gap and short-gulp rules are UpchanSumBeams': a short final gulp is skipped; a new input sequence or a gap (gulps this
reader never saw) resets the context, and after a gap the output restarts in a sequence of its own whose seq0 is the first sample
it holds.  A `dms` command (npair finite numbers) uploads a new table, which takes effect at the next block; the output restarts in
a sequence of its own there too, so that every sequence's cdedisp_dm is the DM its samples were filtered with.

Transforms above 2^13 points (the sweep below about 28 MHz at DM 10 needs them) are BeamCoherentDedisperseLong's
(beam_coherent_dedisperse_long_block.py), a subclass of this block on an engine of its own.  Not built: a bandpass taper, barycentring.
BeamDedisperse's single delay table cannot express a coherent DM per pair: behind this block it is right for one DM only."""
import json
import math
import time

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray, copy_array
from .block_base import Block, InFlight, declare_streams, gulp_time, spans_outlive_release
from .coherent_dedisp import NFFT_MAX, NFFT_MIN, cdedisp_plan, chirp_table, smear_samples

WHO = "BEAM_COHERENT_DEDISPERSE"


def _dms_ok(v, npair):
    return isinstance(v, (list, tuple)) and len(v) == npair and all(isinstance(d, (int, float)) and not isinstance(d, bool) and math.isfinite(d)
                                                                    for d in v)


class BeamCoherentDedisperse(Block):
    STREAM_DEPTH = 4        # gulps whose kernels may be in flight behind the one being enqueued (in-repo rings)
    # what BeamCoherentDedisperseLong changes: the name in messages, the backend's methods (ENGINE + '_run' ...), the entry point
    # named when a run fails, the transform lengths and the planner
    WHO = WHO
    ENGINE = 'cdedisp'
    RUN_NAME = "xengCdedispRun"
    NFFT_RANGE = (NFFT_MIN, NFFT_MAX, "2^8 to 2^13")
    plan = staticmethod(cdedisp_plan)

    def __init__(self, log, iring, oring, nchan, nbeam, ntime_gulp, dms, pair0=0, npair=None, nfft=None, overlap=None, multiple_of=1,
                 guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamCoherentDedisperse, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        if npair is None:
            npair = nbeam // 2 - pair0
        if min(nchan, nbeam, ntime_gulp) <= 0:
            raise ValueError("%s: sizes nchan=%r nbeam=%r ntime_gulp=%r must be positive" % (self.WHO, nchan, nbeam, ntime_gulp))
        if pair0 < 0 or npair <= 0 or pair0 + npair > nbeam // 2:
            raise ValueError("%s: pairs [%d, %d) not a non-empty range of the %d pairs of %d beams" % (self.WHO, pair0, pair0 + npair, nbeam // 2, nbeam))
        if not _dms_ok(dms, npair):
            raise ValueError("%s: `dms` must be %d finite numbers, one per pair: %r" % (self.WHO, npair, dms))
        if (nfft is None) != (overlap is None):
            raise ValueError("%s: give both nfft and overlap, or neither" % self.WHO)
        if not isinstance(multiple_of, int) or multiple_of < 1:
            raise ValueError("%s: multiple_of %r is not a positive integer" % (self.WHO, multiple_of))
        if nfft is not None:
            self._check_plan(nfft, overlap, multiple_of)
        self.nchan, self.nbeam, self.ntime_gulp, self.pair0, self.npair, self.gpu = nchan, nbeam, ntime_gulp, pair0, npair, gpu
        self.dms = [float(d) for d in dms]
        self.nfft, self.overlap, self.multiple_of = nfft, overlap, multiple_of
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')  # (the kernel writes the span itself, or a copy does from a device buffer)
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('dms', type=list, condition=lambda v: _dms_ok(v, self.npair))
        self.update_stats({'nblock': 0, 'ndropped': 0, 'dms': self.dms})
        self._live = False                      # the context exists
        self._nsamples = self._nblocks = 0      # since the context's last reset
        self._first = 0                         # the input sample that was sample 0 of that reset
        if nfft is not None:
            self._initialize()

    def _engine(self, name):
        return getattr(self._bf, '%s_%s' % (self.ENGINE, name))

    @classmethod
    def _check_plan(self, nfft, overlap, multiple_of):
        lo, hi, text = self.NFFT_RANGE
        if not isinstance(nfft, int) or not lo <= nfft <= hi or nfft & (nfft - 1):
            raise ValueError("%s: nfft %r is not a power of two from %s" % (self.WHO, nfft, text))
        if not isinstance(overlap, int) or overlap < 0 or overlap & 1 or overlap > nfft // 2:
            raise ValueError("%s: overlap %r is not an even number from 0 to nfft/2 = %d" % (self.WHO, overlap, nfft // 2))
        if (nfft - overlap) % multiple_of:
            raise ValueError("%s: the step %d is not a multiple of %d" % (self.WHO, nfft - overlap, multiple_of))

    def _initialize(self):
        self._call(self.ENGINE + '_initialize', self.gpu, self.nchan, self.nbeam, self.ntime_gulp, self.pair0, self.npair, self.nfft, self.overlap)
        self.step = self.nfft - self.overlap
        self.max_blocks = -(-self.ntime_gulp // self.step)
        self._live = True
        self._nsamples = self._nblocks = 0

    def _reset(self, first):
        self._engine('reset')()
        self._nsamples = self._nblocks = 0
        self._first = first

    def _freqs(self, ihdr):
        chan_bw = ihdr['bw_hz'] / self.nchan
        return ihdr['sfreq'] + chan_bw * np.arange(self.nchan), chan_bw

    def _set_chirp(self, ihdr):
        freqs, chan_bw = self._freqs(ihdr)
        sweep = max(float(np.max(smear_samples(freqs, chan_bw, d))) for d in self.dms)
        if sweep > self.overlap:
            self.log.warning("%s >> a sweep of %.0f samples is longer than the overlap of %d: the pulses wrap" % (self.WHO, sweep, self.overlap))
        self._upload_chirp(freqs, chan_bw)

    def _upload_chirp(self, freqs, chan_bw):
        self._call('cdedisp_set_chirp', np.ascontiguousarray(chirp_table(freqs, chan_bw, self.dms, self.nfft)))

    def output_header(self, ihdr, start):
        ohdr = ihdr.copy()
        ohdr.update(nstand=2 * self.npair, nbeam=2 * self.npair, pair0=self.pair0, seq0=start, cdedisp_dm=list(self.dms), cdedisp_nfft=self.nfft,
                    cdedisp_overlap=self.overlap)
        return ohdr

    def _check_header(self, ihdr):
        """Beamform's voltage output only (UpchanSumBeams' check): not the products of another reader."""
        if ihdr.get('nchan') != self.nchan or ihdr.get('nbeam') != self.nbeam:
            raise ValueError("%s: %r channels x %r beams in the header, %d x %d configured" % (self.WHO, ihdr.get('nchan'), ihdr.get('nbeam'), self.nchan, self.nbeam))
        if ihdr.get('nbit') != 32 or not ihdr.get('complex') or ihdr.get('npol') != 1:
            raise ValueError("%s: the input is not single-pol cf32 voltage beams (nbit %r, complex %r, npol %r)"
                             % (self.WHO, ihdr.get('nbit'), ihdr.get('complex'), ihdr.get('npol')))
        for k in ('acc_len', 'ntime_sum', 'nupchan'):
            if k in ihdr:
                raise ValueError("%s: the input carries '%s': integrated or channelised products, not voltage beams" % (self.WHO, k))
        for k in ('bw_hz', 'sfreq'):
            v = ihdr.get(k)
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v) or v <= 0:
                raise ValueError("%s: the header's '%s' is %r: the chirp needs the band" % (self.WHO, k, v))

    def main(self):
        self.bind()
        # Streaming, tickets and the staged copy: InFlight (block_base.py).  A call that completes ONE block writes its span
        # itself; one that completes several writes them side by side into a device buffer, and the copy stream moves each into
        # a span of its own (so does every call when the output ring is pinned host memory).
        streaming = spans_outlive_release(self.iring, self.oring)
        can_copy = hasattr(self._bf, 'copy_async')
        self._staged = streaming and self.oring.space == 'cuda_host' and can_copy
        self._dev = None
        with InFlight(self._engine('wait'), self._engine('sync'), self._bf, outstanding=lambda: 2 * self.max_blocks) as inflight, \
                self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                self._sequence(iseq, oring, streaming, can_copy, inflight)

    def _sequence(self, iseq, oring, streaming, can_copy, inflight):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        self._check_header(ihdr)
        inflight.retire(0)
        if self.nfft is None:
            freqs, chan_bw = self._freqs(ihdr)
            self.nfft, self.overlap = self.plan(freqs, chan_bw, max(abs(d) for d in self.dms), self.multiple_of)
            self.log.info("%s >> planned nfft %d, overlap %d" % (self.WHO, self.nfft, self.overlap))
        if not self._live:
            self._initialize()
        unit = self.nchan * 2 * self.npair * self.step * 8
        self.oring.resize(unit)
        seq0 = ihdr['seq0']
        igulp_size = self.nchan * self.nbeam * self.ntime_gulp * 8
        this_gulp_time = seq0
        expected = seq0
        oseq = None
        self._reset(seq0)                       # (a new sequence: what came before it counts as nothing)
        self._set_chirp(ihdr)
        try:
            prev_time = time.time()
            for ispan in iseq.read(igulp_size):
                if ispan.size < igulp_size:
                    continue                    # a short final gulp is skipped (as the reference's gulp_nframe reader does)
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, self.ntime_gulp, this_gulp_time)
                restart = False
                if this_gulp_time != expected:
                    # samples this reader never saw: the block in progress does not line up with what comes now
                    if self._nsamples > self._nblocks * self.step:
                        self.update_stats({'ndropped': self.stats['ndropped'] + 1})
                    self.log.warning("%s >> samples [%d, %d) were not read: the stream starts again" % (self.WHO, expected, this_gulp_time))
                    self._reset(this_gulp_time)
                    restart = True
                if self.update_pending:
                    self.update_command_vals()
                    new = self.command_vals.get('dms')
                    if new is not None and [float(d) for d in new] != self.dms:
                        self.dms = [float(d) for d in new]
                        self._set_chirp(ihdr)   # (waits for the work in flight; holds from the next block)
                        self.update_stats({'dms': self.dms})
                        restart = True
                if restart and oseq is not None:
                    inflight.retire(0)
                    oseq.end()
                    oseq = None
                expected = this_gulp_time + self.ntime_gulp
                self.update_stats({'curr_sample': this_gulp_time})
                held = ispan.data
                if oseq is None:
                    start = self._first + self._nblocks * self.step + self.overlap // 2
                    oseq = oring.begin_sequence(time_tag=start, header=json.dumps(self.output_header(ihdr, start)))
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                after = self._nsamples + self.ntime_gulp
                nb = (0 if after < self.nfft else (after - self.nfft) // self.step + 1) - self._nblocks
                ospans, stage = [], None
                try:
                    for _ in range(nb):
                        ospans.append(oseq.reserve(unit))
                    # where the kernel writes: the span itself, a device buffer the copy stream empties, or one this thread does
                    direct = streaming and nb == 1 and not self._staged
                    staged = streaming and can_copy and nb >= 1 and not direct
                    target = None
                    if direct:
                        target = ospans[0].data
                    elif staged:
                        stage = inflight.take_stage(self.max_blocks * unit)
                        target = stage
                    elif nb:
                        if self._dev is None or self._dev.nbytes != self.max_blocks * unit:
                            self._dev = XArray(shape=(self.max_blocks * unit,), dtype=np.uint8, space=self._bf.space_in)
                        target = self._dev
                    rv, done = self._engine('run')(held, target)
                    if rv != self._bf.BF_STATUS_SUCCESS:
                        raise RuntimeError("%s returned %d: %s" % (self.RUN_NAME, rv, self._bf.last_error()))
                    if done != nb:
                        raise RuntimeError("%s: the context completed %d block(s) where the block counted %d" % (self.WHO, done, nb))
                    self._nsamples, self._nblocks = after, self._nblocks + nb
                    if nb:
                        self.update_stats({'nblock': self.stats['nblock'] + nb, 'last_end_sample': self._first + self._nblocks * self.step + self.overlap // 2})
                    if direct or staged or (streaming and nb == 0):
                        osps, ospans = ospans, []
                        inflight.push(self._engine('mark')(), osps, held, stage)
                        inflight.retire(self.STREAM_DEPTH)
                    else:
                        inflight.retire(0)      # (spans are committed in order)
                        self._engine('sync')()
                        while ospans:
                            k = nb - len(ospans)
                            copy_array(ospans[0].data, self._dev.byte_slice(k * unit, unit))   # (synchronous copy)
                            ospans.pop(0).close()
                finally:
                    for osp in ospans:
                        osp.close()
                curr_time = time.time()
                process_time = curr_time - prev_time
                prev_time = curr_time
                self.perf_proclog.update({'acquire_time': acquire_time, 'reserve_time': 0.0, 'process_time': process_time})
        finally:
            inflight.retire(0)                  # every call in flight is complete (and every output span committed) first
            if oseq is not None:
                oseq.end()
