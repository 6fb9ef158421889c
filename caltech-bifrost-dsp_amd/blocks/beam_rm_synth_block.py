"""BeamRmSynth: Faraday rotation-measure synthesis of the folded dual-pol profiles, the follow-up stage of BeamFold(stokes='full').

Reads the ring BeamFold writes: every input sequence is one sub-integration, one span of
  f32 [npair][4][nfine/nfscr][nbin] = [XX, YY, Re(XY*), Im(XY*)], the bin the fastest axis
and yields one output sequence of one span on a host-space ring:
  npair x RM_RECORD {k, peak, n_on, n_off}      the depth of the Faraday spectrum's peak (k = -1: none)
  f32 [npair][nphi]                             the Faraday spectrum: |F(phi_k)|^2 summed over the on-pulse bins
  f32 [npair][4][nbin]                          I, Q, U, V summed over the band, Q and U de-rotated at depth k
(xengRmsynth*, csrc/rmsynth_kernels.h; the definition is in include/xeng.h).  The header gains `rm_phis`, `lambda0_sq`, `rm_feeds`,
the byte offsets `record_offset`, `spec_offset`, `profile_offset`, and the masks' counts `rm_n_on`, `rm_n_off` per pair.  No
reference counterpart: the reference ships its beams to external pulsar backends.

The channel groups' centres come from the header's `fine_sfreq`, `fine_bw_hz` and `nfscr`; the rotation table (rm_table) is made
again only when they or the weights change.  A pair whose entry in the header's `pulsars` is None is inactive: nothing of it is
read and its output is +0.  By default every bin is both off-pulse (the baseline) and on-pulse (the spectrum).  Commands `weights`
(nchg finite numbers; 0 leaves a group out) and `masks` (dict(off=[npair][nbin], on=[npair][nbin]) of 0 / 1, either may be
missing) hold from the next span.  If the input ring is not in device space the span is copied to the device once.

Not built: leakage and X-Y phase calibration, an ionospheric model, spectra summed over sub-integrations (additive: on the host),
RM-CLEAN, a depth grid per pair, single-pulse RM from the cut-outs, a contraction on MFMAs."""
import json

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray, copy_array
from .block_base import Block, declare_streams
from .rm_synth import FEEDS, MAX_NPHI, rm_offsets, rm_table

WHO = "BEAM_RM_SYNTH"


def _count(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class BeamRmSynth(Block):
    def __init__(self, log, iring, oring, npair, nchg, nbin, phis, feeds='linear', weights=None, off=None, on=None, guarantee=True, core=-1, gpu=-1,
                 etcd_client=None, backend=None):
        super(BeamRmSynth, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        if not all(_count(v) for v in (npair, nchg, nbin)) or min(npair, nchg, nbin) <= 0 or npair > 65535 or nchg > 65536 or nbin > 65536:
            raise ValueError("%s: npair=%r (1 to 65535), nchg=%r and nbin=%r (1 to 65536) must be integers" % (WHO, npair, nchg, nbin))
        if feeds not in FEEDS:
            raise ValueError("%s: feeds %r not one of %s" % (WHO, feeds, sorted(FEEDS)))
        try:
            self.phis = np.asarray(phis, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("%s: the depths are not a list of numbers" % WHO)
        if not 1 <= self.phis.size <= MAX_NPHI or not np.all(np.isfinite(self.phis)) or nchg * self.phis.size * 8 > 1 << 30:
            raise ValueError("%s: 1 to %d finite depths, and a table of at most 1 GiB" % (WHO, MAX_NPHI))
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the spectra go to a host-space ring" % (WHO, oring.space))
        self.npair, self.nchg, self.nbin, self.nphi, self.feeds, self.gpu = npair, nchg, nbin, int(self.phis.size), feeds, gpu
        self._weights = self._checked_weights(weights) if weights is not None else None
        self._masks = self._checked_masks(dict(off=off, on=on))
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.define_command_key('masks', type=dict, condition=lambda v: self._checked_masks(v, quiet=True) is not None)
        self.update_stats({'nsubint': 0, 'npeak': 0})
        self._call('rmsynth_initialize', self.gpu, npair, nchg, nbin, self.nphi, FEEDS[feeds])
        self._call('rmsynth_set_masks', self._masks['off'], self._masks['on'])
        self._table_key, self._active, self.lambda0_sq = None, None, None

    def _checked_weights(self, w, quiet=False):
        try:
            a = np.ascontiguousarray(w, np.float32).reshape(-1)
            ok = a.size == self.nchg and bool(np.all(np.isfinite(a))) and bool(np.any(a != 0))
        except (TypeError, ValueError):
            a, ok = None, False
        if ok:
            return a
        if quiet:
            return None
        raise ValueError("%s: the weights must be %d finite numbers, not all 0" % (WHO, self.nchg))

    def _checked_masks(self, m, quiet=False):
        """dict(off, on) of uint8 [npair][nbin] or None (every bin) each."""
        out, ok = {}, isinstance(m, dict) and not set(m) - {'off', 'on'}
        for k in ('off', 'on'):
            v = m.get(k) if ok else None
            if v is None:
                out[k] = None
                continue
            try:
                a = np.asarray(v)
                ok = ok and a.shape == (self.npair, self.nbin) and a.dtype.kind in 'biu' and bool(np.all((a == 0) | (a == 1)))
                out[k] = np.ascontiguousarray(a, np.uint8) if ok else None
            except (TypeError, ValueError):
                ok = False
        if ok:
            return out
        if quiet:
            return None
        raise ValueError("%s: masks are dict(off, on) of %d x %d values of 0 or 1 (or None)" % (WHO, self.npair, self.nbin))

    def group_frequencies(self, ihdr):
        """The centres of the channel groups in Hz: group g is the fine channels [g nfscr, (g + 1) nfscr) of the header."""
        nfscr = ihdr['nfscr']
        return ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * (nfscr * np.arange(self.nchg) + (nfscr - 1) / 2.0)

    def _check_header(self, ihdr):
        if 'nbin' not in ihdr:
            raise ValueError("%s: the input carries no 'nbin': it has not been folded" % WHO)
        if 'rm_phis' in ihdr:
            raise ValueError("%s: the input carries 'rm_phis': it is a Faraday spectrum already" % WHO)
        if ihdr.get('nprod') != 4:
            raise ValueError("%s: nprod %r in the header: the four dual-pol words are needed (BeamFold(stokes='full'))" % (WHO, ihdr.get('nprod')))
        if ihdr['nbin'] != self.nbin or ihdr.get('nbeam') != self.npair:
            raise ValueError("%s: %r bins x %r pairs in the header, %d x %d configured" % (WHO, ihdr['nbin'], ihdr.get('nbeam'), self.nbin, self.npair))
        for k in ('fine_sfreq', 'fine_bw_hz'):
            if not isinstance(ihdr.get(k), (int, float)) or isinstance(ihdr.get(k), bool) or (k == 'fine_bw_hz' and not ihdr[k] > 0):
                raise ValueError("%s: the header's '%s' is %r" % (WHO, k, ihdr.get(k)))
        nfscr = ihdr.get('nfscr')
        nfine = ihdr.get('nchan', 0) * ihdr.get('nupchan', 0) if _count(ihdr.get('nchan')) and _count(ihdr.get('nupchan')) else None
        if not _count(nfscr) or nfscr <= 0 or nfine is None or nfine != nfscr * self.nchg:
            raise ValueError("%s: %r fine channels in groups of %r in the header, %d groups configured" % (WHO, nfine, nfscr, self.nchg))

    def output_header(self, ihdr, counts):
        ohdr = ihdr.copy()
        a, b, n = rm_offsets(self.npair, self.nphi, self.nbin)
        ohdr.update(rm_phis=self.phis.tolist(), lambda0_sq=self.lambda0_sq, rm_feeds=self.feeds, record_offset=0, spec_offset=a, profile_offset=b,
                    span_bytes=n, rm_n_on=counts[0], rm_n_off=counts[1])
        return ohdr

    def _counts(self):
        full = [self.nbin] * self.npair
        on, off = self._masks['on'], self._masks['off']
        return (full if on is None else on.sum(1).astype(int).tolist()), (full if off is None else off.sum(1).astype(int).tolist())

    def _load_pending(self):
        cmds = self.take_commands(('weights', 'masks'))
        if 'weights' in cmds:
            self._weights = self._checked_weights(cmds['weights'])
            self._table_key = None
        if 'masks' in cmds:
            self._masks = self._checked_masks(cmds['masks'])
            self._call('rmsynth_set_masks', self._masks['off'], self._masks['on'])

    def main(self):
        self.bind()
        igulp_size = self.npair * 4 * self.nchg * self.nbin * 4
        ogulp_size = rm_offsets(self.npair, self.nphi, self.nbin)[2]
        self.oring.resize(ogulp_size)
        self._dev = XArray(shape=(ogulp_size,), dtype=np.uint8, space=self._bf.space_in)       # a call's output lands here first
        self._stage = None
        with self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                ihdr = json.loads(iseq.header.tostring())
                self.sequence_proclog.update(ihdr)
                self._check_header(ihdr)
                if self.update_pending:
                    self._load_pending()
                key = (ihdr['fine_sfreq'], ihdr['fine_bw_hz'], ihdr['nfscr'])
                if key != self._table_key:
                    T, w, use, self.lambda0_sq = rm_table(self.group_frequencies(ihdr), self.phis, self._weights)
                    self._call('rmsynth_set_table', T, w, use)
                    self._table_key = key
                psr = ihdr.get('pulsars')
                active = np.ones(self.npair, np.uint8) if not isinstance(psr, list) or len(psr) != self.npair else np.array([e is not None for e in psr], np.uint8)
                if self._active is None or not np.array_equal(active, self._active):
                    self._call('rmsynth_set_active', active)
                    self._active = active
                for ispan in iseq.read(igulp_size):
                    if ispan.size < igulp_size:
                        continue                # a short span is no cube
                    held = ispan.data
                    if getattr(held, 'space', self._bf.space_in) != self._bf.space_in:
                        if self._stage is None:
                            self._stage = XArray(shape=(igulp_size,), dtype=np.uint8, space=self._bf.space_in)
                        copy_array(self._stage, held)       # (one staged copy per span: the kernels read the cube many times)
                        held = self._stage
                    self._call('rmsynth_run', held, self._dev)
                    self._bf.rmsynth_sync()
                    with oring.begin_sequence(time_tag=iseq.time_tag, header=json.dumps(self.output_header(ihdr, self._counts()))) as oseq:
                        with oseq.reserve(ogulp_size) as ospan:
                            copy_array(ospan.data, self._dev)       # (synchronous: once per sub-integration)
                            k = ospan.data.numpy()[:16 * self.npair].view(np.int32)[::4]
                            npeak = int(np.count_nonzero(k >= 0))
                    self.update_stats({'nsubint': self.stats['nsubint'] + 1, 'npeak': self.stats['npeak'] + npeak})
