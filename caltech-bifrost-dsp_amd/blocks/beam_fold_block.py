"""BeamFold: phase-folded pulse profiles of known pulsars from the fine-channel power beams, one pulsar per beam pair.

Reads the ring BeamDedisperse reads -- the output of UpchanSumBeams (live) or of UpchanBeamform(dual_pol=True) (from dumps), in
device space: spans of
  f32 [nwin][npair][nchan][nupchan][4] = [XX, YY, Re(XY*), Im(XY*)]
and folds every window into the profile kept on the device (xengFold*, csrc/fold_kernels.h; the definition is in
include/xeng.h): the bin of a window comes from a 64-bit integer oscillator per pair, set from the pair's spin model
(fold_phase) and re-tuned at every sub-integration boundary, at a sequence start and after a gap.  Every `nsub` spans the
profile is dumped and cleared into ONE output span
  f32 [npair][nprod][nfine/nfscr][nbin],   nprod = 1 (stokes='I': XX + YY) or 4 (stokes='full'), the bin the fastest axis
with the channels of a pair rotated by the pair's DM (fold_rotations at the header's fine-channel frequencies), weighted and
summed in groups of nfscr (nfscr = nfine: the dedispersed profile; 1: the full cube), and divided by the hits when
`normalise`.  Each sub-integration is an output sequence of its own, of one span: its header carries what belongs to it -- the
hits per pair and bin, its start -- beside nbin, nfscr, nprod, tsamp, nsub and the pulsar list.  No reference counterpart: the
reference ships its power beams to external pulsar backends.

Clock: `pepoch` and the phase are on the SEQUENCE'S SAMPLE CLOCK IN SECONDS: sample s of the input (the unit of the header's
seq0 and of the span time tags) is at t = s * nchan / bw_hz.  Window m of a span that starts at sample s0 is folded at the phase
of its midpoint, t = s0 * nchan / bw_hz + (m + 1/2) * tsamp with tsamp = acc_len * nchan / bw_hz.  No barycentring: f0, f1 are
the apparent (topocentric) values for the time of the observation.

`pulsars` is a list of npair entries, each None (the pair is left out: its plane is +0) or dict(f0, f1, pepoch, dm) (f1 and
pepoch default to 0).  Sequence, gap and short-span rules are UpchanSumBeams': a short final span is skipped; a new input
sequence starts from nothing (the sub-integration in progress is dropped); a gap inside a sequence resets nothing -- the fold
goes on with the phase re-tuned from the next span's own time, and the gap shows in the hits.  Commands `weights` (nfine finite
numbers; 0 leaves a channel out) and `pulsars` both take effect at the next sub-integration boundary.
"""
import json
import time
from fractions import Fraction

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray, copy_array
from .beam_dedisperse_block import STOKES, check_power_beam_header, checked_fine_weights
from .block_base import Block, InFlight, declare_streams, gulp_time, spans_outlive_release
from .fold import fold_phase, fold_rotations, fold_rotations_coherent

WHO = "BEAM_FOLD"


def checked_pulsars(pulsars, npair):
    """The list as the block keeps it: None or dict(f0, f1, pepoch, dm) of floats per pair; ValueError otherwise."""
    if not isinstance(pulsars, (list, tuple)) or len(pulsars) != npair:
        raise ValueError("%s: `pulsars` must be a list of %d entries (None or dict(f0, f1, pepoch, dm))" % (WHO, npair))
    out = []
    for p, e in enumerate(pulsars):
        if e is None:
            out.append(None)
            continue
        if not isinstance(e, dict) or set(e) - {'f0', 'f1', 'pepoch', 'dm', 'name'} or 'f0' not in e or 'dm' not in e:
            raise ValueError("%s: pulsar %d is %r, not None or dict(f0, f1, pepoch, dm)" % (WHO, p, e))
        try:
            v = dict(f0=float(e['f0']), f1=float(e.get('f1', 0.0)), pepoch=float(e.get('pepoch', 0.0)), dm=float(e['dm']))
        except (TypeError, ValueError):
            raise ValueError("%s: pulsar %d has a value that is not a number: %r" % (WHO, p, e))
        if not all(np.isfinite(x) for x in v.values()) or v['f0'] <= 0 or v['dm'] < 0:
            raise ValueError("%s: pulsar %d needs finite values, f0 > 0 and dm >= 0: %r" % (WHO, p, e))
        if 'name' in e:
            v['name'] = str(e['name'])
        out.append(v)
    return out


class BeamFold(Block):
    STREAM_DEPTH = 4        # spans whose kernels may be in flight behind the one being enqueued (in-repo rings)

    def __init__(self, log, iring, oring, npair, nchan, nupchan, nwin, nbin, pulsars, nsub, nfscr=None, stokes='I', normalise=True,
                 weights=None, guarantee=True, core=-1, gpu=-1, etcd_client=None, backend=None):
        super(BeamFold, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        if stokes not in STOKES:
            raise ValueError("%s: stokes %r not one of %s" % (WHO, stokes, sorted(STOKES)))
        for k, v in (('npair', npair), ('nchan', nchan), ('nupchan', nupchan), ('nwin', nwin), ('nbin', nbin), ('nsub', nsub)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
                raise ValueError("%s: %s = %r must be a positive integer" % (WHO, k, v))
        if nbin > 65536:
            raise ValueError("%s: nbin %d is above 65536" % (WHO, nbin))
        self.npair, self.nchan, self.nupchan, self.nwin, self.nbin, self.nsub, self.gpu = npair, nchan, nupchan, nwin, nbin, nsub, gpu
        self.nfine, self.nprod, self.stokes, self.normalise = nchan * nupchan, STOKES[stokes], stokes, bool(normalise)
        self.nfscr = self.nfine if nfscr is None else nfscr
        if not isinstance(self.nfscr, (int, np.integer)) or self.nfscr <= 0 or self.nfine % self.nfscr:
            raise ValueError("%s: nfscr %r does not divide the %d fine channels" % (WHO, nfscr, self.nfine))
        self.pulsars = checked_pulsars(pulsars, npair)
        self._weights = self._checked_weights(weights) if weights is not None else None
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.define_command_key('pulsars', type=list, condition=self._pulsars_ok)
        self.update_stats({'nwindow': 0, 'ngap': 0, 'nsubint': 0})
        rv = self._bf.fold_initialize(self.gpu, npair, self.nfine, nwin, nbin, self.nprod)
        if rv != self._bf.BF_STATUS_SUCCESS:
            raise RuntimeError("xengFoldInitialize returned %d: %s" % (rv, self._bf.last_error()))
        self._call('fold_set_weights', self._weights)

    def _pulsars_ok(self, v):
        try:
            checked_pulsars(v, self.npair)
            return True
        except ValueError:
            return False

    def _checked_weights(self, w, quiet=False):
        return checked_fine_weights(WHO, w, self.nfine, quiet)

    # ---- what the library is told, from the header and the pulsar list
    def rotations(self, ihdr):
        """int32 [npair][nfine]: fold_rotations of each pair's DM and f0 at the header's fine-channel centres (0 for a pair left out).
        Where the header carries `cdedisp_dm` -- the beams have passed BeamCoherentDedisperse, which has aligned the fine channels of
        a coarse channel to its centre already -- fold_rotations_coherent with that pair's coherent DM instead: pair p of this
        block is entry pair0 + p of the list, pair0 being what the upchanneliser behind that block selected."""
        freqs = ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * np.arange(self.nfine)
        dm_coh = ihdr.get('cdedisp_dm')
        if dm_coh is not None:
            first = int(ihdr.get('pair0', 0))
            if not isinstance(dm_coh, list) or first < 0 or first + self.npair > len(dm_coh):
                raise ValueError("%s: the header's 'cdedisp_dm' %r does not cover the pairs [%d, %d)" % (WHO, dm_coh, first, first + self.npair))
            coarse = ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * self.nupchan * (np.arange(self.nfine) // self.nupchan + 0.5)
        rot = np.zeros((self.npair, self.nfine), np.int32)
        for p, e in enumerate(self.pulsars):
            if e is None:
                continue
            if dm_coh is None:
                rot[p] = fold_rotations(freqs, e['dm'], e['f0'], self.nbin)
            else:
                rot[p] = fold_rotations_coherent(freqs, coarse, e['dm'], float(dm_coh[first + p]), e['f0'], self.nbin)
        return rot

    def phase(self, ihdr, acc_len, sample):
        """(phi0, dphi uint64 [npair], ddphi int64 [npair], active uint8 [npair]) of a span that starts at `sample`: fold_phase at
        the midpoint of its first window, in exact rational arithmetic."""
        per = Fraction(self.nchan) / Fraction(ihdr['bw_hz'])        # seconds per sample
        tsamp = acc_len * per
        t0 = sample * per + tsamp / 2
        phi0, dphi, ddphi, active = np.zeros(self.npair, np.uint64), np.zeros(self.npair, np.uint64), np.zeros(self.npair, np.int64), np.zeros(self.npair, np.uint8)
        for p, e in enumerate(self.pulsars):
            if e is not None:
                a, b, c = fold_phase(e['f0'], e['f1'], e['pepoch'], t0, tsamp)
                phi0[p], dphi[p], ddphi[p], active[p] = a, b, c, 1
        return phi0, dphi, ddphi, active

    def output_header(self, ihdr, start, tsamp, hits, nwindow):
        ohdr = ihdr.copy()
        ohdr.update(nbin=self.nbin, nfscr=self.nfscr, nprod=self.nprod, tsamp=tsamp, nsub=self.nsub, pulsars=self.pulsars, normalise=self.normalise,
                    hits=hits.tolist(), subint_start=start, subint_nwindow=nwindow, seq0=start)
        return ohdr

    def main(self):
        self.bind()
        self._oshape = (self.npair, self.nprod, self.nfine // self.nfscr, self.nbin)
        ogulp_size = int(np.prod(self._oshape)) * 4
        self.oring.resize(ogulp_size)
        streaming = spans_outlive_release(self.iring, self.oring)
        self._dev = XArray(shape=self._oshape, dtype=np.float32, space=self._bf.space_in)      # a dump lands here first: its hits go into the header
        with InFlight(self._bf.fold_wait, self._bf.fold_sync) as inflight:
            with self.oring.begin_writing() as oring:
                for iseq in self.iring.read(guarantee=self.guarantee):
                    self._sequence(iseq, oring, ogulp_size, streaming, inflight)

    def _load_pending(self, ihdr):
        """`weights` and `pulsars` commands, at a sub-integration boundary (the setters wait for the spans in flight)."""
        self.update_command_vals()
        w, psr = self.command_vals.get('weights'), self.command_vals.get('pulsars')
        if w is not None:
            self._weights = self._checked_weights(w)
            self._call('fold_set_weights', self._weights)
        if psr is not None:
            self.pulsars = checked_pulsars(psr, self.npair)
            self._call('fold_set_rotations', self.rotations(ihdr))

    def _sequence(self, iseq, oring, ogulp_size, streaming, inflight):
        ihdr = json.loads(iseq.header.tostring())
        self.sequence_proclog.update(ihdr)
        acc_len = check_power_beam_header(WHO, ihdr, self.npair, self.nchan, self.nupchan)
        for k in ('nbin', 'ndm'):
            if k in ihdr:
                raise ValueError("%s: the input carries '%s': it has been folded or dedispersed already" % (WHO, k))
        tsamp = acc_len * self.nchan / ihdr['bw_hz']
        inflight.retire(0)
        self._bf.fold_reset()                   # (a new sequence starts from nothing)
        self._call('fold_set_rotations', self.rotations(ihdr))
        seq0 = ihdr['seq0']
        ntime_span = self.nwin * acc_len        # samples of the beamformer's clock per span
        igulp_size = self.nwin * self.npair * self.nfine * 16
        this_gulp_time = seq0
        expected = seq0
        count = 0                               # windows taken since the reset
        in_sub, sub_start = 0, None             # spans folded into the sub-integration in progress, its first sample
        tune = True
        hits = np.zeros((self.npair, self.nbin), np.uint32)
        try:
            prev_time = time.time()
            for ispan in iseq.read(igulp_size):
                if ispan.size < igulp_size:
                    continue                    # a short final span is skipped (as the reference's gulp_nframe reader does)
                this_gulp_time = gulp_time(ispan, seq0, igulp_size, ntime_span, this_gulp_time)
                if this_gulp_time != expected:
                    # windows this reader never saw: the fold goes on, its phase taken from this span's own time
                    self.update_stats({'ngap': self.stats['ngap'] + 1})
                    self.log.warning("%s >> samples [%d, %d) were not read: the phase is set again" % (WHO, expected, this_gulp_time))
                    tune = True
                expected = this_gulp_time + ntime_span
                self.update_stats({'curr_sample': this_gulp_time})
                if in_sub == 0:
                    sub_start = this_gulp_time
                    if self.update_pending:
                        self._load_pending(ihdr)
                if tune:
                    self._call('fold_set_phase', *(self.phase(ihdr, acc_len, this_gulp_time) + (count,)))
                    tune = False
                held = ispan.data
                curr_time = time.time()
                acquire_time = curr_time - prev_time
                prev_time = curr_time
                self._call('fold_run', held, self.nwin)
                count += self.nwin
                in_sub += 1
                self.update_stats({'nwindow': self.stats['nwindow'] + self.nwin, 'last_end_sample': this_gulp_time + ntime_span})
                if streaming:
                    inflight.push(self._bf.fold_mark(), None, held)
                    inflight.retire(self.STREAM_DEPTH)
                else:
                    self._bf.fold_sync()
                if in_sub == self.nsub:
                    self._call('fold_dump', self._dev, hits, self.nfscr, self.normalise, True)
                    self._bf.fold_sync()
                    inflight.retire(0)
                    with oring.begin_sequence(time_tag=sub_start, header=json.dumps(self.output_header(ihdr, sub_start, tsamp, hits, in_sub * self.nwin))) as oseq:
                        with oseq.reserve(ogulp_size) as ospan:
                            copy_array(ospan.data, self._dev)       # (synchronous: once per sub-integration)
                    self.update_stats({'nsubint': self.stats['nsubint'] + 1})
                    in_sub, tune = 0, True      # (the oscillator is set again from the next span's time)
                curr_time = time.time()
                process_time = curr_time - prev_time
                prev_time = curr_time
                self.perf_proclog.update({'acquire_time': acquire_time, 'reserve_time': 0.0, 'process_time': process_time})
        finally:
            inflight.retire(0)                  # every call in flight is complete first
