"""BeamFold without a GPU, both ring implementations: the oscillator of the restatement (tests/fold_ref.py) against exact
rational arithmetic; fold_phase against the spin model in exact arithmetic over 10^5 windows; fold_rotations against the formula
written out; profile_snr; the restatement against a term-by-term loop; the block on CPU rings with a backend that serves fold_*
from the restatement -- spans within and across sequences, the sub-integration cadence, the output header and hits, a gap (the
phase is set again, the fold goes on), a `weights` and a `pulsars` command landing at the next boundary, an inactive pair,
refusals -- and the C entry points' argument checks."""
import ctypes
import json
from fractions import Fraction
from math import lcm

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import BeamFold, fold_phase, fold_rotations, profile_snr
from caltech_bifrost_dsp_amd.blocks.dedisp import KDM
from caltech_bifrost_dsp_amd.ring import Ring
from tests.fake_backend import OracleBackend
from tests.fold_ref import MASK, FoldRef, fmaf32, fold_naive, osc_bin, osc_phase
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_dedisp_cpu import CHAN_BW, SFREQ, power_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


# ---------------------------------------------------------------- the oscillator
@pytest.mark.parametrize("ddphi", [0, 3 << 20, -(5 << 21)])
def test_oscillator_is_the_contracts_polynomial_mod_one_turn(ddphi):
    """Phi(m) = phi0 + dphi*m + ddphi*m(m-1)/2 turns*2^64 against Fractions: the fraction of a turn and the bin, at the first and
    last 500 of 10^6 windows, every 997th between, and around the window at which Phi wraps; nbin a power of two and not."""
    phi0, dphi = (1 << 64) - (1 << 40), int(0.0123456789 * 2 ** 64)
    ms = sorted(set(list(range(500)) + list(range(0, 10 ** 6, 997)) + list(range(10 ** 6 - 500, 10 ** 6))))
    wraps = 0
    for nbin in (1024, 7):
        prev = None
        for m in ms:
            turns = Fraction(phi0, 1 << 64) + Fraction(dphi, 1 << 64) * m + Fraction(ddphi, 1 << 64) * Fraction(m * (m - 1), 2)
            frac = turns - (turns.numerator // turns.denominator)
            phi = osc_phase(phi0, dphi, ddphi, m)
            assert 0 <= phi <= MASK and Fraction(phi, 1 << 64) == frac
            top = (frac * (1 << 32)).numerator // (frac * (1 << 32)).denominator        # floor(frac * 2^32)
            assert osc_bin(phi0, dphi, ddphi, m, nbin) == (top * nbin) >> 32 < nbin
            if prev is not None and m == prev[0] + 1 and phi < prev[1] and dphi < (1 << 63):
                wraps += 1
            prev = (m, phi)
    assert osc_phase(phi0, dphi, ddphi, 0) == phi0 and osc_phase(phi0, dphi, ddphi, 1) == (phi0 + dphi) & MASK      # (m(m-1)/2 = 0 at 0 and 1)
    assert wraps > 0


# ---------------------------------------------------------------- fold_phase
@pytest.mark.parametrize("f0,f1", [(0.7, 1e-12), (33.0, -3.7e-10)])
def test_fold_phase_reproduces_the_spin_model_on_every_window(f0, f1):
    """phi(t) = f0 (t - pepoch) + f1 (t - pepoch)^2 / 2 at t0 + m tsamp in exact integer arithmetic (the floats are dyadic
    rationals: one common denominator D) against the oscillator of fold_phase, 10^5 windows, 1024 bins.  The oscillator is
    within (1 + m + m(m-1)/2) 2^-65 turns of the model (three roundings to 2^-64 turns); this (t0, f0) keeps the model itself
    farther than that from every bin edge, so the bins must agree on every window."""
    pepoch, t0, tsamp, nbin, nwindows = 100.25, 12345.678, 0.04, 1024, 10 ** 5
    F = Fraction
    dt = F(t0) - F(pepoch)
    c0 = F(f0) * dt + F(f1) * dt * dt / 2
    c1 = (F(f0) + F(f1) * dt) * F(tsamp)
    c2 = F(f1) * F(tsamp) ** 2 / 2
    D = lcm(c0.denominator, c1.denominator, c2.denominator)
    n0, n1, n2 = (int(c * D) for c in (c0, c1, c2))
    assert F(n0, D) == c0 and F(n1, D) == c1 and F(n2, D) == c2
    phi0, dphi, ddphi = fold_phase(f0, f1, pepoch, t0, tsamp)
    assert all(isinstance(v, int) for v in (phi0, dphi, ddphi)) and 0 <= phi0 <= MASK and 0 <= dphi <= MASK
    assert (ddphi < 0) == (f1 < 0) and abs(F(ddphi, 1 << 64) - 2 * c2) <= F(1, 1 << 65)
    worst_edge, mism = None, 0
    for m in range(nwindows):
        num = (n0 + n1 * m + n2 * m * m) % D                    # frac(phi) = num / D
        scaled = num * nbin
        ref_bin, rem = divmod(scaled, D)                        # the model's bin and how far into it, in bins * D
        edge = min(rem, D - rem)                                # distance to the nearer bin edge, in bins * D
        slack = edge * (1 << 65) - (1 + m + m * (m - 1) // 2) * nbin * D      # > 0: farther than the oscillator's error
        worst_edge = slack if worst_edge is None else min(worst_edge, slack)
        mism += osc_bin(phi0, dphi, ddphi, m, nbin) != ref_bin
    assert worst_edge > 0, "the reference comes within the oscillator's error of a bin edge: choose another t0"
    assert mism == 0
    # exact inputs are taken as they are; a Fraction t0 and the float it rounds to differ
    assert fold_phase(F(f0), F(f1), F(pepoch), F(t0), F(tsamp)) == (phi0, dphi, ddphi)
    assert fold_phase(1, 0, 0, F(1, 3), F(1, 8)) == (round(F(1 << 64, 3)), 1 << 61, 0)
    with pytest.raises(ValueError, match="fold_phase"):
        fold_phase(1.0, 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="fold_phase"):
        fold_phase(1.0, 1e3, 0.0, 0.0, 1.0)


# ---------------------------------------------------------------- fold_rotations, profile_snr
def test_fold_rotations_is_the_formula_at_the_headers_frequencies():
    """rint(KDM dm (f^-2 - f_ref^-2) f_spin nbin) mod nbin, f in MHz, f_ref the top channel: 0 there, several turns over the
    band at this DM (so the mod matters), growing towards low frequencies before the mod."""
    hdr = power_header(3, 2, 8, 4)
    nfine, nbin, dm, f_spin = 24, 64, 30.0, 1.4
    freqs = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(nfine)
    f_mhz = freqs * 1e-6
    raw = [round(KDM * dm * (f ** -2 - f_mhz[-1] ** -2) * f_spin * nbin) for f in f_mhz]
    got = fold_rotations(freqs, dm, f_spin, nbin)
    assert got.dtype == np.int32 and got.shape == (nfine,) and got.tolist() == [r % nbin for r in raw]
    assert got[-1] == 0 and raw[0] > nbin and all(a >= b for a, b in zip(raw, raw[1:])) and got.min() >= 0 and got.max() < nbin
    assert (fold_rotations(freqs, 0.0, f_spin, nbin) == 0).all()
    lo = fold_rotations(freqs, dm, f_spin, nbin, f_ref_hz=freqs[0])        # (a reference below the band: negative delays wrap)
    assert lo[0] == 0 and lo.min() >= 0 and lo.tolist() == [round(KDM * dm * (f ** -2 - f_mhz[0] ** -2) * f_spin * nbin) % nbin for f in f_mhz]
    for bad in (dict(dm=float('nan')), dict(f_spin=0.0), dict(nbin=0), dict(freqs_hz=[0.0, 1e6]), dict(f_ref_hz=-1.0)):
        kw = dict(freqs_hz=freqs, dm=dm, f_spin=f_spin, nbin=nbin)
        kw.update(bad)
        with pytest.raises(ValueError, match="fold_rotations"):
            fold_rotations(**kw)


def test_profile_snr_takes_the_quietest_half_and_the_peak():
    rng = np.random.default_rng(2)
    prof = 10 + rng.standard_normal(64)
    prof[60:64] += 6                                            # a broad hump that wraps...
    prof[0:3] += 6
    prof[62] += 40                                              # ...and the peak
    s = profile_snr(prof)
    off = prof[10:42]                                           # any half away from the hump has these statistics to a few %
    assert s['bin'] == 62 and s['peak'] == prof[62] and abs(s['mean'] - off.mean()) < 0.5 and 0.6 < s['sigma'] < 1.4
    assert s['snr'] == (s['peak'] - s['mean']) / s['sigma'] > 25
    flat = np.full(16, 3.0)
    assert profile_snr(flat)['snr'] == 0.0
    flat[5] = 4.0
    assert profile_snr(flat) == dict(mean=3.0, sigma=0.0, peak=4.0, bin=5, snr=float('inf'))
    with pytest.raises(ValueError, match="profile_snr"):
        profile_snr([1.0])


# ---------------------------------------------------------------- the restatement
def _osc_arrays(osc):
    """[(phi0, dphi, ddphi, active)] -> the four host arrays of xengFoldSetPhase."""
    return (np.array([o[0] for o in osc], np.uint64), np.array([o[1] for o in osc], np.uint64), np.array([o[2] for o in osc], np.int64),
            np.array([o[3] for o in osc], np.uint8))


def _period_osc(period, phase=0.0, ddphi=0, active=1):
    """An oscillator of `period` windows per turn."""
    return (int(phase * 2 ** 64) & MASK, int(round(2 ** 64 / period)) & MASK, ddphi, active)


def test_fmaf32_is_one_rounding():
    """Against Fractions where rounding first to fp64 and then to fp32 goes wrong: w*x = 2^-24 (1 - 2^-46) is 2^-70 short of
    the fp32 tie above s = 1 + 2^-23 (fp64 rounds the sum onto the tie, and the tie then goes to the even neighbour)."""
    w, x = np.float32(1 + 2.0 ** -23), np.float32((1 - 2.0 ** -23) * 2.0 ** -24)
    wrong = 0
    for s in (np.float32(1 + 2.0 ** -23), np.float32(-(1 + 2.0 ** -23)), np.float32(1.0), np.float32(3.0)):
        exact = Fraction(float(w)) * Fraction(float(x)) + Fraction(float(s))
        lo = np.float32(float(exact))                                       # (two roundings: may be the wrong neighbour)
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda c: abs(Fraction(float(c)) - exact))
        wrong += lo != best
        assert fmaf32(w, np.array([x]), np.array([s]))[0] == best
    assert wrong >= 2                                                       # (the cases do exercise the double rounding)
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    assert np.array_equal(fmaf32(np.float32(1), b, c), b + c) and np.array_equal(fmaf32(a, b, np.float32(0)), a * b)


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("normalise", [0, 1])
def test_restatement_is_the_definition(nprod, normalise):
    """Against one term at a time: a period of 5.3 windows on 7 bins and one of 37 windows on 7 bins, a pair left out, a
    SetPhase mid-run, rotations that wrap, weights with zeros, a NaN in a channel left out; exact on integer data with integer
    weights when not normalising."""
    rng = np.random.default_rng(3 + nprod)
    nwindows, npair, nfine, nbin, nfscr = 40, 3, 6, 7, 3
    x = rng.integers(0, 50, (nwindows, npair, nfine, 4)).astype(np.float32)
    osc = [_period_osc(5.3, 0.4, 1 << 50), _period_osc(37, 0.9, -(1 << 52)), _period_osc(3, 0, 0, active=0)]
    osc2 = [_period_osc(5.3, 0.1), _period_osc(11, 0.5), _period_osc(3, 0, 0, active=0)]
    rot = rng.integers(0, nbin, (npair, nfine))
    w = np.array([1, 2, 0, 1, 3, 1], np.float32)
    ref = FoldRef(npair, nfine, nbin, nprod)
    ref.set_rotations(rot)
    ref.set_weights(w)
    ref.set_phase(*_osc_arrays(osc), 0)
    bins = [ref.bins(25)]
    ref.run(x[:10])
    ref.run(x[10:25])
    ref.set_phase(*_osc_arrays(osc2), 25)
    bins.append(ref.bins(15))
    dirty = x[25:].copy()
    dirty[3, 0, 2] = np.nan
    ref.run(dirty)
    bins = np.concatenate(bins, axis=1)
    assert (bins[2] == -1).all() and len(set(bins[0].tolist())) == nbin and (bins[:2] >= 0).all()
    got, hits = ref.dump(nfscr, normalise, 1)
    exp, ehits = fold_naive(x, bins, rot, w, nbin, nfscr, nprod, normalise)
    assert np.array_equal(hits, ehits) and hits.sum() == 2 * nwindows and hits.dtype == np.uint32
    assert got.shape == (npair, nprod, nfine // nfscr, nbin) and got.dtype == np.float32 and np.isfinite(got).all()
    if normalise:
        assert np.allclose(got, exp, rtol=1e-5, atol=0)
    else:
        assert np.array_equal(got.astype(np.float64), exp)
    assert (got[2] == 0).all() and not (ref.prof != 0).any() and ref.hits.sum() == 0
    again, _ = ref.dump(nfscr, normalise, 0)
    assert (again == 0).all() and not np.signbit(again).any()


# ---------------------------------------------------------------- the block on CPU rings
class FoldBackend(OracleBackend):
    """The oracle backend plus xengFold* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.fo, self.calls, self.phases = None, [], []

    def fold_initialize(self, gpu, npair, nfine, nwin, nbin, nprod):
        self.fo = FoldRef(npair, nfine, nbin, nprod)
        self.nwin = nwin
        self.calls.append('init')
        return 0

    def fold_set_phase(self, phi0, dphi, ddphi, active, n_ref):
        assert phi0.dtype == np.uint64 and dphi.dtype == np.uint64 and ddphi.dtype == np.int64 and active.dtype == np.uint8
        if not 0 <= n_ref <= self.fo.n:
            return INVALID_ARGUMENT
        self.fo.set_phase(phi0, dphi, ddphi, active, n_ref)
        self.phases.append((phi0.tolist(), dphi.tolist(), ddphi.tolist(), active.tolist(), n_ref))
        self.calls.append('set_phase')
        return 0

    def fold_set_rotations(self, rot):
        assert rot is None or (rot.dtype == np.int32 and rot.shape == (self.fo.npair, self.fo.nfine) and rot.flags.c_contiguous)
        self.fo.set_rotations(rot)
        self.calls.append('set_rotations')
        return 0

    def fold_set_weights(self, weights):
        assert weights is None or (weights.dtype == np.float32 and weights.shape == (self.fo.nfine,))
        self.fo.set_weights(weights)
        self.calls.append('set_weights')
        return 0

    def fold_run(self, in_arr, nwin_call):
        u = self.fo
        assert u.osc is not None and 1 <= nwin_call <= self.nwin
        u.run(in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, u.npair, u.nfine, 4))
        self.calls.append('run')
        return 0

    def fold_dump(self, out_arr, hits, nfscr, normalise, clear):
        out, h = self.fo.dump(nfscr, normalise, clear)
        out_arr.numpy().reshape(-1).view(np.uint8).view(np.float32)[...] = out.reshape(-1)
        if hits is not None:
            assert hits.dtype == np.uint32 and hits.shape == h.shape
            hits[...] = h
        self.calls.append(('dump', nfscr, bool(normalise), bool(clear)))
        return 0

    def fold_reset(self):
        self.fo.reset()
        self.calls.append('reset')

    def fold_mark(self):
        return self.beam_mark()

    def fold_wait(self, ticket):
        self.beam_wait(ticket)

    def fold_sync(self):
        pass


def _powers(rng, nwindows, npair, nfine):
    return rng.integers(0, 50, (nwindows, npair, nfine, 4)).astype(np.float32)


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


PSR_A = dict(f0=9.3, f1=-2e-7, pepoch=0.5, dm=0.02)
PSR_B = dict(f0=2.1, f1=0.0, pepoch=0.0, dm=0.3)
PSR_C = dict(f0=5.7, f1=1e-8, pepoch=-3.0, dm=0.1)


def _expected_phase(hdr, nchan, acc_len, sample, pulsars):
    """What the block must hand to SetPhase for a span that starts at `sample`: fold_phase at the midpoint of its first window
    on the sequence's sample clock, t = sample * nchan / bw_hz + tsamp / 2."""
    per = Fraction(nchan) / Fraction(hdr['bw_hz'])
    tsamp = acc_len * per
    out = []
    for e in pulsars:
        out.append((0, 0, 0, 0) if e is None else fold_phase(e['f0'], e.get('f1', 0.0), e.get('pepoch', 0.0), sample * per + tsamp / 2, tsamp) + (1,))
    return _osc_arrays(out)


def _expected_rot(hdr, nfine, nbin, pulsars):
    freqs = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(nfine)
    return np.array([np.zeros(nfine, np.int32) if e is None else fold_rotations(freqs, e['dm'], e['f0'], nbin) for e in pulsars], np.int32)


def _subints(hdr, x, spans, nchan, N, W, nwin, nbin, nprod, nsub, nfscr, normalise, pulsars, weights=None, changes=None):
    """The sub-integrations the block must write for the spans `spans` (indices into x, in units of spans) of one sequence,
    driving the restatement directly: [(start sample, out, hits)].  changes: {span index: (pulsars, weights)} taking effect
    at the first boundary at or after that span."""
    npair, nfine, acc_len = x.shape[1], x.shape[2], W * N
    ref = FoldRef(npair, nfine, nbin, nprod)
    ref.set_rotations(_expected_rot(hdr, nfine, nbin, pulsars))
    ref.set_weights(weights)
    step = nwin * acc_len
    out, in_sub, tune, prev, pending = [], 0, True, None, None
    for k in spans:
        sample = hdr['seq0'] + k * step
        if changes and k in changes:
            pending = changes[k]
        if prev is not None and k != prev + 1:
            tune = True
        prev = k
        if in_sub == 0:
            start = sample
            if pending is not None:
                pulsars, weights = pending
                pending = None
                ref.set_weights(weights)
                ref.set_rotations(_expected_rot(hdr, nfine, nbin, pulsars))
        if tune:
            ref.set_phase(*_expected_phase(hdr, nchan, acc_len, sample, pulsars), ref.n)
            tune = False
        ref.run(x[k * nwin:(k + 1) * nwin])
        in_sub += 1
        if in_sub == nsub:
            o, h = ref.dump(nfscr, normalise, 1)
            out.append((start, o, h))
            in_sub, tune = 0, True
    return out


@pytest.mark.parametrize("stokes,normalise", [('I', True), ('full', False)])
def test_block_subintegrations_within_and_across_sequences(stokes, normalise):
    """Source -> BeamFold -> Sink on in-repo rings, two sequences of 5 spans of 4 windows, nsub = 2: two sub-integrations per
    sequence, each an output sequence of one span, and the fifth span of each sequence dropped with it.  Every one equals the
    restatement driven with fold_phase at the span's own time and fold_rotations at the header's frequencies; pair 1 is left
    out (a plane of +0, hits 0); the header carries nbin, nfscr, nprod, tsamp, nsub, the pulsars, the hits and the start."""
    nchan, npair, N, W, nwin, nspan, nbin, nsub, nfscr = 2, 3, 8, 4, 4, 5, 16, 2, 4
    nfine, nprod = nchan * N, {'I': 1, 'full': 4}[stokes]
    rng = np.random.default_rng(5 + nprod)
    xs = [_powers(rng, nspan * nwin, npair, nfine) for _ in range(2)]
    hdrs = [power_header(nchan, npair, N, W, seq0=100000 * (s + 1)) for s in range(2)]
    pulsars = [PSR_A, None, PSR_B]
    r0, r1 = Ring("ub-output"), Ring("fold-output")
    be = FoldBackend()
    bf = BeamFold(LOG, r0, r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nbin=nbin, pulsars=pulsars, nsub=nsub, nfscr=nfscr, stokes=stokes,
                  normalise=normalise, backend=be)
    shape = (npair, nprod, nfine // nfscr, nbin)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([bf], Source(r0, [(hdrs[s], xs[s], nwin * npair * nfine * 16) for s in range(2)]), [sink])
    assert len(sink.sequences) == 4
    tsamp = W * N * nchan / hdrs[0]['bw_hz']
    for s in range(2):
        exp = _subints(hdrs[s], xs[s], range(nspan), nchan, N, W, nwin, nbin, nprod, nsub, nfscr, normalise, pulsars)
        assert len(exp) == 2
        for j, (start, out, hits) in enumerate(exp):
            hd, tag, spans = sink.sequences[2 * s + j]
            assert tag == start == hdrs[s]['seq0'] + j * nsub * nwin * W * N and hd['subint_start'] == start and hd['seq0'] == start and len(spans) == 1
            got = spans[0].view(np.float32).reshape(shape)
            assert np.array_equal(got.view(np.uint32), out.view(np.uint32))
            assert hd['hits'] == hits.tolist() and hits[0].sum() == hits[2].sum() == nsub * nwin and hits[1].sum() == 0 and (got[1] == 0).all()
            assert (hd['nbin'], hd['nfscr'], hd['nprod'], hd['tsamp'], hd['nsub'], hd['subint_nwindow']) == (nbin, nfscr, nprod, tsamp, nsub, nsub * nwin)
            assert hd['pulsars'] == [PSR_A, None, PSR_B] and hd['normalise'] == normalise and hd['nupchan'] == N and hd['fine_sfreq'] == hdrs[s]['fine_sfreq']
            assert np.abs(got).max() > 0
    per_seq = ['reset', 'set_rotations'] + (['set_phase', 'run', 'run', ('dump', nfscr, normalise, True)]) * 2 + ['set_phase', 'run']
    assert be.calls == ['init', 'set_weights'] + per_seq * 2
    assert [p[4] for p in be.phases] == [0, 2 * nwin, 4 * nwin] * 2            # (n_ref = the count at each re-tune)
    assert bf.stats['nwindow'] == 2 * nspan * nwin and bf.stats['nsubint'] == 4 and bf.stats['ngap'] == 0


def test_block_gap_sets_the_phase_again_and_the_fold_goes_on():
    """Spans 0, 1, 3, 4, 5, 6 of a sequence (2 never read), nsub = 3: nothing is reset; span 3 is folded into the
    sub-integration spans 0 and 1 began, with the oscillator set from span 3's own time and n_ref = the count."""
    nchan, npair, N, W, nwin, nbin, nsub, seq0 = 2, 2, 8, 4, 4, 8, 3, 7000
    nfine = nchan * N
    rng = np.random.default_rng(11)
    x = _powers(rng, 7 * nwin, npair, nfine)
    hdr = power_header(nchan, npair, N, W, seq0=seq0)
    order = (0, 1, 3, 4, 5, 6)
    seen = [(k, np.ascontiguousarray(x[k * nwin:(k + 1) * nwin])) for k in order]
    be = FoldBackend()
    r1 = Ring("fold-output")
    pulsars = [PSR_A, PSR_C]
    bf = BeamFold(LOG, _FakeRing([_FakeSeq(hdr, seen, nwin * npair * nfine * 16)]), r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nbin=nbin,
                  pulsars=pulsars, nsub=nsub, backend=be)
    shape = (npair, 1, 1, nbin)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    sink.start()
    bf.main()
    sink.join(20)
    dump = ('dump', nfine, True, True)
    assert be.calls == ['init', 'set_weights', 'reset', 'set_rotations', 'set_phase', 'run', 'run', 'set_phase', 'run', dump, 'set_phase', 'run', 'run', 'run', dump]
    assert [p[4] for p in be.phases] == [0, 2 * nwin, 3 * nwin] and bf.stats['ngap'] == 1
    step = nwin * W * N
    assert be.phases[1][:4] == tuple(a.tolist() for a in _expected_phase(hdr, nchan, W * N, seq0 + 3 * step, pulsars))
    exp = _subints(hdr, x, order, nchan, N, W, nwin, nbin, 1, nsub, nfine, True, pulsars)
    assert len(sink.sequences) == len(exp) == 2
    for (hd, tag, spans), (start, out, hits) in zip(sink.sequences, exp):
        assert tag == start and hd['hits'] == hits.tolist() and len(spans) == 1
        assert np.array_equal(spans[0].view(np.float32).reshape(shape).view(np.uint32), out.view(np.uint32))
    assert [s[1] for s in sink.sequences] == [seq0, seq0 + 4 * step]


def test_block_commands_land_at_the_next_boundary():
    """`weights` and `pulsars` commands that arrive while the first sub-integration (spans 0, 1) is in progress: it is dumped
    with the old ones, the second (spans 2, 3) is folded and dumped with the new.  A bad command is refused and changes
    nothing."""
    nchan, npair, N, W, nwin, nbin, nsub = 2, 2, 8, 4, 4, 8, 2
    nfine = nchan * N
    rng = np.random.default_rng(13)
    x = _powers(rng, 4 * nwin, npair, nfine)
    hdr = power_header(nchan, npair, N, W)
    w = rng.integers(0, 3, nfine).astype(float).tolist()
    old, new = [PSR_A, PSR_B], [None, PSR_C]
    be = FoldBackend()
    r1 = Ring("fold-output")
    box = {}

    def spans():
        for k in range(4):
            if k == 1:
                box['bf'].process_command_strings(_cmd(weights=w, pulsars=new))
                assert box['bf'].last_response['val']['status'] == 'normal'
                for bad in (dict(weights=w[:-1]), dict(weights=w[:-1] + [float('nan')]), dict(pulsars=[PSR_A]), dict(pulsars=[PSR_A, dict(f0=-1.0, dm=1.0)]),
                            dict(pulsars=[PSR_A, dict(f0=1.0)]), dict(pulsars="B0329+54")):
                    box['bf'].process_command_strings(_cmd("2", **bad))
                    assert box['bf'].last_response['val']['status'] == 'error', bad
            yield k, np.ascontiguousarray(x[k * nwin:(k + 1) * nwin])

    seq = _FakeSeq(hdr, spans(), nwin * npair * nfine * 16)
    bf = box['bf'] = BeamFold(LOG, _FakeRing([seq]), r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nbin=nbin, pulsars=old, nsub=nsub, nfscr=8,
                              normalise=False, backend=be)
    shape = (npair, 1, 2, nbin)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    sink.start()
    bf.main()
    sink.join(20)
    dump = ('dump', 8, False, True)
    assert be.calls == ['init', 'set_weights', 'reset', 'set_rotations', 'set_phase', 'run', 'run', dump, 'set_weights', 'set_rotations', 'set_phase',
                        'run', 'run', dump]
    exp = _subints(hdr, x, range(4), nchan, N, W, nwin, nbin, 1, nsub, 8, False, old, None, changes={1: (new, np.array(w, np.float32))})
    assert len(sink.sequences) == 2
    for (hd, tag, spans_), (start, out, hits) in zip(sink.sequences, exp):
        assert tag == start and hd['hits'] == hits.tolist()
        assert np.array_equal(spans_[0].view(np.float32).reshape(shape).view(np.uint32), out.view(np.uint32))
    assert sink.sequences[0][0]['pulsars'] == old and sink.sequences[1][0]['pulsars'] == [None, dict(PSR_C)]
    assert (exp[1][1][0] == 0).all() and exp[1][2][0].sum() == 0 and exp[0][2][0].sum() == nsub * nwin


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(stokes='Q'), dict(nwin=0), dict(npair=0), dict(nupchan=-8), dict(nbin=0), dict(nbin=1 << 17), dict(nsub=0), dict(nfscr=5),
                                dict(nfscr=0), dict(pulsars=[PSR_A, PSR_B]), dict(pulsars=[dict(f0=1.0)]), dict(pulsars=[dict(f0=0.0, dm=1.0)]),
                                dict(pulsars=[dict(f0=1.0, dm=float('nan'))]), dict(pulsars=[dict(f0=1.0, dm=1.0, period=1.0)]), dict(pulsars="J0000"),
                                dict(weights=np.ones(15)), dict(weights=[float('inf')] * 16)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(npair=1, nchan=2, nupchan=8, nwin=4, nbin=16, pulsars=[PSR_A], nsub=2)
    args.update(kw)
    be = FoldBackend()
    with pytest.raises(ValueError, match="BEAM_FOLD"):
        BeamFold(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.fo is None                    # (refused before the context is made)


@pytest.mark.parametrize("bad", [dict(npol=1), dict(nbit=8), dict(nbeam=2), dict(nchan=4), dict(nupchan=16), dict(nupchan=None), dict(nframe_sum=None),
                                 dict(fine_sfreq=None), dict(fine_bw_hz=0), dict(acc_len=33), dict(ndm=4), dict(nbin=16)])
def test_block_refuses_what_is_not_fine_channel_power_beams(bad):
    """The header checks BeamDedisperse makes, and a span that has been dedispersed or folded already: ValueError before any run."""
    nchan, npair, N, W, nwin = 2, 1, 8, 4, 4
    be = FoldBackend()
    hdr = power_header(nchan, npair, N, W)
    hdr.update(bad)
    x = np.zeros((nwin, npair, nchan * N, 4), np.float32)
    bf = BeamFold(LOG, _FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nbin=16, pulsars=[PSR_A],
                  nsub=1, backend=be)
    with pytest.raises(ValueError, match="BEAM_FOLD"):
        bf.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengFoldInitialize", "xengFoldSetPhase", "xengFoldSetRotations", "xengFoldSetWeights", "xengFoldRun", "xengFoldDump", "xengFoldReset",
         "xengFoldGetInfo", "xengFoldCheckGuards", "xengFoldMark", "xengFoldWait", "xengFoldTicketDone", "xengFoldSync", "xengFoldDestroy")


def test_backend_forwards_every_call_the_block_makes():
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("fold_initialize", "fold_set_phase", "fold_set_rotations", "fold_set_weights", "fold_run", "fold_dump", "fold_reset", "fold_info",
              "fold_guards_intact", "fold_mark", "fold_wait", "fold_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("fold_initialize", "fold_set_phase", "fold_set_rotations", "fold_set_weights", "fold_run", "fold_dump", "fold_reset", "fold_mark", "fold_wait",
              "fold_sync"):
        assert callable(getattr(FoldBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that may wait (the
    setters and Dump among them) are not.  Initialize refuses bad sizes, nprod, nbin, npair and an oversized profile before it
    touches a device; Run, Dump and SetPhase refuse null and misaligned pointers, GetInfo / Mark / TicketDone / CheckGuards null
    results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengFoldRun", "xengFoldReset", "xengFoldMark", "xengFoldTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengFoldInitialize", "xengFoldSetPhase", "xengFoldSetRotations", "xengFoldSetWeights", "xengFoldDump", "xengFoldWait", "xengFoldSync",
                 "xengFoldCheckGuards"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, npair, nfine, nwin, nbin, nprod); the last but one: 16 x 3072 x 4 words x 65536 bins = 51.5 GB of profile
    for args in ((0, 0, 3072, 30, 1024, 1), (0, 16, 0, 30, 1024, 1), (0, 16, 3072, 0, 1024, 1), (0, 16, 3072, 30, 0, 1), (0, 16, 3072, 30, 1024, 2),
                 (0, 16, 3072, 30, 1024, 0), (0, 16, 3072, 30, 65537, 1), (0, 65536, 8, 1, 1, 1), (0, 16, 3072, 30, 65536, 4), (0, -1, 8, 1, 1, 1)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFoldInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    u64, i64, u8 = np.zeros(2, np.uint64), np.zeros(2, np.int64), np.zeros(2, np.uint8)
    pu, pi, pb = (u64.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), i64.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                  u8.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
    for name, args in (("xengFoldRun", (None, 1)), ("xengFoldRun", (4100, 1)), ("xengFoldDump", (None, None, 1, 0, 0)), ("xengFoldDump", (4104, None, 1, 0, 0)),
                       ("xengFoldSetPhase", (None, pu, pi, pb, 0)), ("xengFoldSetPhase", (pu, None, pi, pb, 0)), ("xengFoldSetPhase", (pu, pu, None, pb, 0)),
                       ("xengFoldSetPhase", (pu, pu, pi, None, 0)), ("xengFoldGetInfo", (None, None)), ("xengFoldMark", (None,)),
                       ("xengFoldTicketDone", (1, None)), ("xengFoldCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_fold_gpu.py covers the rest)
    s, n, m, t = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_ulonglong()
    rot = np.zeros(8, np.int32)
    for name, args in (("xengFoldRun", (4096, 1)), ("xengFoldDump", (4096, None, 1, 0, 0)), ("xengFoldSetPhase", (pu, pu, pi, pb, 0)),
                       ("xengFoldSetRotations", (rot.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),)), ("xengFoldSetRotations", (None,)),
                       ("xengFoldSetWeights", (None,)), ("xengFoldReset", ()), ("xengFoldGetInfo", (ctypes.byref(n), ctypes.byref(m))),
                       ("xengFoldMark", (ctypes.byref(t),)), ("xengFoldWait", (1,)), ("xengFoldTicketDone", (1, ctypes.byref(s))), ("xengFoldSync", ()),
                       ("xengFoldCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengFoldDestroy")         # (nothing to destroy: success)
