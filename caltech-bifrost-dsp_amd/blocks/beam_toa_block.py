"""BeamToa: template-matched arrival phases, DM corrections and arrival times of the folded profiles, the timing stage behind BeamFold.

Reads the ring BeamFold writes: every input sequence is one sub-integration, one span of
  f32 [npair][nprod][nfine/nfscr][nbin],   nprod = 1 (stokes='I') or 4 (stokes='full': XX + YY is formed), the bin the fastest axis
and yields one output sequence of one span on a host-space ring, with rows r = 0 .. nsub-1 the sub-bands and r = nsub the band:
  npair x (nsub+1) x TOA_RECORD {l, peak, base, var}   the lag of the correlation's peak (l = -1: none), the off-pulse mean and variance
  f32 [npair][nsub+1][nbin]                            the weighted sub-band profiles and their sum
  f32 [npair][nsub+1][nharm][2]                        their harmonics 1 .. nharm with the baseline taken out
  f32 [npair][nsub+1][nlag]                            their correlation with the template at the lags l / nlag turns
(xengToa*, csrc/toa_kernels.h; the definition is in include/xeng.h).  After the call has completed the block refines every row's
lag between the grid's points (toa_refine), fits a DM correction to the sub-bands' offsets (toa_dm_fit) and turns the offset into
a time (toa_epoch), in float64 on the host.  The header gains `toas`, per pair None or dict(tau, tau_err, toa_s, dm_offset, dm_err,
snr, chi2), `toa_nsub`, `toa_nharm`, `toa_nlag`, `toa_edges`, `toa_freqs` and the byte offsets `record_offset`, `profile_offset`,
`harmonic_offset`, `ccf_offset`.  tau is the delay of the pulse behind the template in turns at the frequency BeamFold aligns to
(the centre of the highest fine channel): the DM fit's line read there where two or more sub-bands gave an offset, else the band
row's own; toa_s is toa_epoch of it, a decimal string of seconds on the sequence's sample clock with 15 digits behind the point.
No reference counterpart: the reference ships its beams to external pulsar backends.

The sub-bands are toa_subbands(nchg, nsub); their frequencies come from the header's `fine_sfreq`, `fine_bw_hz` and `nfscr`.  A
pair whose entry in the header's `pulsars` is None is inactive: nothing of it is read and its output is +0.  By default every bin
is off-pulse.  Commands `templates` (as the constructor's), `weights` (nchg finite numbers; 0 leaves a group out) and `masks`
(dict(off=[npair][nbin]) of 0 / 1) hold from the next span.  If the input ring is not in device space the span is copied to the
device once.

Not built: barycentring, a par-file or polyco reader, a .tim or archive writer, template generation from data, profile-evolution
(2-D template) fits, scattering fits."""
import json

import numpy as np

from ..backend import default_backend
from ..ndarray import XArray, copy_array
from .block_base import Block, declare_streams
from .dedisp import KDM
from .toa import (MAX_NBIN, MAX_NHARM, MAX_NLAG, MAX_NSUB, MAX_TABLE_BYTES, as_toa, subband_frequencies, toa_dm_fit, toa_epoch, toa_offsets, toa_refine,
                  toa_subbands, toa_tables, toa_template)

WHO = "BEAM_TOA"


def _count(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class BeamToa(Block):
    def __init__(self, log, iring, oring, npair, nchg, nbin, nsub, templates, nharm=None, nlag=None, weights=None, off=None, guarantee=True, core=-1,
                 gpu=-1, etcd_client=None, backend=None):
        super(BeamToa, self).__init__(log, iring, oring, guarantee, core, etcd_client=etcd_client)
        if not all(_count(v) for v in (npair, nchg, nbin, nsub)) or not 1 <= npair <= 65535 or not 1 <= nchg <= 65536 or not 3 <= nbin <= MAX_NBIN or \
                not 1 <= nsub <= min(nchg, MAX_NSUB):
            raise ValueError("%s: npair=%r (1 to 65535), nchg=%r (1 to 65536), nbin=%r (3 to %d) and nsub=%r (1 to min(nchg, %d)) must be integers"
                             % (WHO, npair, nchg, nbin, MAX_NBIN, nsub, MAX_NSUB))
        nharm = min(MAX_NHARM, (nbin - 1) // 2) if nharm is None else nharm
        nlag = min(MAX_NLAG, 4 * nbin) if nlag is None else nlag
        if not _count(nharm) or not 1 <= nharm <= min(MAX_NHARM, (nbin - 1) // 2) or not _count(nlag) or not 1 <= nlag <= MAX_NLAG:
            raise ValueError("%s: nharm=%r (1 to min(%d, (nbin - 1) / 2)) and nlag=%r (1 to %d) must be integers" % (WHO, nharm, MAX_NHARM, nlag, MAX_NLAG))
        if max(nbin * nharm, nharm * nlag, npair * (nsub + 1) * nharm) * 8 > MAX_TABLE_BYTES:
            raise ValueError("%s: a table above 1 GiB" % WHO)
        if getattr(oring, 'space', 'system') not in ('system', 'cuda_host'):
            raise ValueError("%s: the output ring is in space %r: the arrival phases go to a host-space ring" % (WHO, oring.space))
        self.npair, self.nchg, self.nbin, self.nsub, self.nharm, self.nlag, self.gpu = npair, nchg, nbin, nsub, nharm, nlag, gpu
        self.edges = toa_subbands(nchg, nsub)
        self._S = self._checked_templates(templates)
        self._weights = self._checked_weights(weights) if weights is not None else None
        self._off = self._checked_masks(dict(off=off))
        self._bf = backend if backend is not None else default_backend()
        declare_streams(iring, 'beam')          # (the kernels run on the beamformer's stream)
        declare_streams(oring, 'beam', 'copy')
        if self.gpu != -1:
            self._bf.set_device(self.gpu)
        self.define_command_key('templates', type=list, condition=lambda v: self._checked_templates(v, quiet=True) is not None)
        self.define_command_key('weights', type=list, condition=lambda v: self._checked_weights(v, quiet=True) is not None)
        self.define_command_key('masks', type=dict, condition=lambda v: self._checked_masks(v, quiet=True) is not False)
        self.update_stats({'nsubint': 0, 'ntoa': 0})
        self._nprod, self._active = None, None

    def _checked_templates(self, t, quiet=False):
        try:
            a = np.asarray(t, np.float64)
            if a.shape not in ((self.npair, self.nbin), (self.npair, self.nsub, self.nbin)):
                raise ValueError("%d x %d or %d x %d x %d numbers are needed, not %r" % (self.npair, self.nbin, self.npair, self.nsub, self.nbin, a.shape))
            return toa_template(a, self.nharm, self.nsub)
        except (TypeError, ValueError) as e:
            if quiet:
                return None
            raise ValueError("%s: the templates: %s" % (WHO, e))

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
        """uint8 [npair][nbin] or None (every bin) of dict(off); False (quiet) or ValueError otherwise."""
        ok = isinstance(m, dict) and not set(m) - {'off'}
        v = m.get('off') if ok else None
        out = None
        if ok and v is not None:
            try:
                a = np.asarray(v)
                ok = a.shape == (self.npair, self.nbin) and a.dtype.kind in 'biu' and bool(np.all((a == 0) | (a == 1)))
                out = np.ascontiguousarray(a, np.uint8) if ok else None
            except (TypeError, ValueError):
                ok = False
        if ok:
            return out
        if quiet:
            return False
        raise ValueError("%s: masks are dict(off) of %d x %d values of 0 or 1 (or None)" % (WHO, self.npair, self.nbin))

    def group_frequencies(self, ihdr):
        """The centres of the channel groups in Hz: group g is the fine channels [g nfscr, (g + 1) nfscr) of the header."""
        nfscr = ihdr['nfscr']
        return ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * (nfscr * np.arange(self.nchg) + (nfscr - 1) / 2.0)

    def reference_frequency(self, ihdr):
        """The frequency in Hz BeamFold aligns its channels to: the centre of the highest fine channel."""
        return ihdr['fine_sfreq'] + ihdr['fine_bw_hz'] * (ihdr['nfscr'] * self.nchg - 1)

    def _check_header(self, ihdr):
        if 'nbin' not in ihdr:
            raise ValueError("%s: the input carries no 'nbin': it has not been folded" % WHO)
        for k in ('rm_phis', 'toa_nlag'):
            if k in ihdr:
                raise ValueError("%s: the input carries '%s': it is no folded cube any more" % (WHO, k))
        if ihdr.get('nprod') not in (1, 4):
            raise ValueError("%s: nprod %r in the header: 1 or 4 is needed" % (WHO, ihdr.get('nprod')))
        if ihdr['nbin'] != self.nbin or ihdr.get('nbeam') != self.npair:
            raise ValueError("%s: %r bins x %r pairs in the header, %d x %d configured" % (WHO, ihdr['nbin'], ihdr.get('nbeam'), self.nbin, self.npair))
        for k in ('fine_sfreq', 'fine_bw_hz'):
            if not isinstance(ihdr.get(k), (int, float)) or isinstance(ihdr.get(k), bool) or (k == 'fine_bw_hz' and not ihdr[k] > 0):
                raise ValueError("%s: the header's '%s' is %r" % (WHO, k, ihdr.get(k)))
        nfscr = ihdr.get('nfscr')
        nfine = ihdr.get('nchan', 0) * ihdr.get('nupchan', 0) if _count(ihdr.get('nchan')) and _count(ihdr.get('nupchan')) else None
        if not _count(nfscr) or nfscr <= 0 or nfine is None or nfine != nfscr * self.nchg:
            raise ValueError("%s: %r fine channels in groups of %r in the header, %d groups configured" % (WHO, nfine, nfscr, self.nchg))

    def _load_pending(self):
        cmds = self.take_commands(('templates', 'weights', 'masks'))
        if 'templates' in cmds:
            self._S = self._checked_templates(cmds['templates'])
            if self._nprod is not None:
                self._call('toa_set_template', self._S)
        if 'weights' in cmds:
            self._weights = self._checked_weights(cmds['weights'])
            if self._nprod is not None:
                self._call('toa_set_bands', self.edges, self._weights)
        if 'masks' in cmds:
            self._off = self._checked_masks(cmds['masks'])
            if self._nprod is not None:
                self._call('toa_set_mask', self._off)

    def _open(self, nprod):
        """The context for cubes of nprod planes (made again if a later sequence has the other nprod)."""
        self._call('toa_initialize', self.gpu, self.npair, nprod, self.nchg, self.nbin, self.nsub, self.nharm, self.nlag)
        self._call('toa_set_bands', self.edges, self._weights)
        self._call('toa_set_tables', *toa_tables(self.nbin, self.nharm, self.nlag))
        self._call('toa_set_template', self._S)
        self._call('toa_set_mask', self._off)
        self._nprod, self._active = nprod, None

    def measure(self, ihdr, span, active):
        """The header's `toas`: per pair None or dict(tau, tau_err, toa_s, dm_offset, dm_err, snr, chi2) from one output span."""
        rec, _, PH, _ = as_toa(span, self.npair, self.nsub, self.nbin, self.nharm, self.nlag)
        freqs = subband_frequencies(self.group_frequencies(ihdr), self.edges, self._weights)
        f_ref = self.reference_frequency(ihdr) * 1e-6
        psr = ihdr.get('pulsars')
        toas = []
        for p in range(self.npair):
            if not active[p]:
                toas.append(None)
                continue
            fits = [toa_refine(PH[p, r], self._S[p, r], int(rec[p, r]['l']), self.nlag, float(rec[p, r]['var']), self.nbin) for r in range(self.nsub + 1)]
            band = fits[self.nsub]
            e = psr[p] if isinstance(psr, list) and len(psr) == self.npair and isinstance(psr[p], dict) else None
            dm = None
            if e is not None and self.nsub >= 2:
                ok = [f is not None and np.isfinite(freqs[r]) for r, f in enumerate(fits[:self.nsub])]
                use = [r for r in range(self.nsub) if ok[r]]
                if len(use) >= 2:
                    dm = toa_dm_fit([fits[r]['tau'] for r in use], [fits[r]['tau_err'] for r in use], freqs[use], e['f0'],
                                    None if band is None else band['tau'])
            if band is None and (dm is None or dm['dm'] is None):
                toas.append(None)
                continue
            out = dict(tau=None if band is None else band['tau'], tau_err=None if band is None else band['tau_err'], toa_s=None, dm_offset=None, dm_err=None,
                       snr=None if band is None else band['snr'], chi2=None if band is None else band['chi2'])
            if dm is not None and dm['dm'] is not None:
                x_ref = KDM * e['f0'] * f_ref ** -2
                out.update(dm_offset=dm['dm'], dm_err=dm['dm_err'], tau=dm['tau_inf'] + dm['dm'] * x_ref)
                if band is None:
                    out['tau_err'] = dm['tau_inf_err']
            if e is not None and out['tau'] is not None:
                t = toa_epoch(ihdr, p, out['tau'])
                n = round(t * 10 ** 15)
                out['toa_s'] = "%s%d.%015d" % ('-' if n < 0 else '', abs(n) // 10 ** 15, abs(n) % 10 ** 15)
            for k, v in out.items():
                if isinstance(v, float) and not np.isfinite(v):
                    out[k] = None                       # (the header is JSON)
            toas.append(out)
        return toas, freqs

    def output_header(self, ihdr, toas, freqs):
        ohdr = ihdr.copy()
        a, b, c, n = toa_offsets(self.npair, self.nsub, self.nbin, self.nharm, self.nlag)
        ohdr.update(toas=toas, toa_nsub=self.nsub, toa_nharm=self.nharm, toa_nlag=self.nlag, toa_edges=self.edges.tolist(),
                    toa_freqs=[None if not np.isfinite(f) else float(f) for f in freqs], record_offset=0, profile_offset=a, harmonic_offset=b, ccf_offset=c,
                    span_bytes=n)
        return ohdr

    def main(self):
        self.bind()
        ogulp_size = toa_offsets(self.npair, self.nsub, self.nbin, self.nharm, self.nlag)[3]
        self.oring.resize(ogulp_size)
        self._dev = XArray(shape=(ogulp_size,), dtype=np.uint8, space=self._bf.space_in)       # a call's output lands here first
        self._host = XArray(shape=(ogulp_size,), dtype=np.uint8, space='system')               # ... and is measured here
        self._stage = None
        with self.oring.begin_writing() as oring:
            for iseq in self.iring.read(guarantee=self.guarantee):
                ihdr = json.loads(iseq.header.tostring())
                self.sequence_proclog.update(ihdr)
                self._check_header(ihdr)
                if ihdr['nprod'] != self._nprod:
                    self._open(ihdr['nprod'])
                if self.update_pending:
                    self._load_pending()
                igulp_size = self.npair * self._nprod * self.nchg * self.nbin * 4
                psr = ihdr.get('pulsars')
                active = np.ones(self.npair, np.uint8) if not isinstance(psr, list) or len(psr) != self.npair else np.array([e is not None for e in psr], np.uint8)
                if self._active is None or not np.array_equal(active, self._active):
                    self._call('toa_set_active', active)
                    self._active = active
                for ispan in iseq.read(igulp_size):
                    if ispan.size < igulp_size:
                        continue                # a short span is no cube
                    held = ispan.data
                    if getattr(held, 'space', self._bf.space_in) != self._bf.space_in:
                        if self._stage is None or self._stage_bytes != igulp_size:
                            self._stage, self._stage_bytes = XArray(shape=(igulp_size,), dtype=np.uint8, space=self._bf.space_in), igulp_size
                        copy_array(self._stage, held)       # (one staged copy per span: the kernels address the device)
                        held = self._stage
                    self._call('toa_run', held, self._dev)
                    self._bf.toa_sync()
                    copy_array(self._host, self._dev)       # (synchronous: once per sub-integration)
                    toas, freqs = self.measure(ihdr, self._host.numpy(), active)
                    with oring.begin_sequence(time_tag=iseq.time_tag, header=json.dumps(self.output_header(ihdr, toas, freqs))) as oseq:
                        with oseq.reserve(ogulp_size) as ospan:
                            copy_array(ospan.data, self._host)
                    self.update_stats({'nsubint': self.stats['nsubint'] + 1, 'ntoa': self.stats['ntoa'] + sum(t is not None for t in toas)})
