"""The PFB front end of UpchanBeamform and UpchanCorr without a GPU, both ring implementations: the float64 restatement
(tests/upchan_pfb_ref.py) against a direct loop over the definition of include/xeng.h, the default coefficients and their
leakage, both blocks on CPU rings with oracle backends that keep the history across gulps (resets at sequence starts and gaps,
two-part gulps, UpchanCorr's prime before an integration boundary), no new backend call at pfb_ntap=1, and the C entry points'
argument checks."""
import ctypes
import json
import types

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanBeamform, UpchanCorr
from caltech_bifrost_dsp_amd.blocks.pfb import pfb_coeffs
from caltech_bifrost_dsp_amd.ring import Ring
from oracle import xeng_oracle as orc
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.upchan_pfb_ref import pfb_channelise, pfb_fine_select, tone_leakage_db, upchan_beamform_pfb, upchan_corr_pfb
from tests.upchan_ref import channelise

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def _u8(part):
    return part.numpy().reshape(-1).view(np.uint8)


class _History:
    """The context's PFB state as the C library keeps it: taps, coefficients, the last (P-1)*N samples or None (zeros)."""

    def __init__(self):
        self.ntap, self.h, self.hist = 1, None, None

    def set(self, ntap, coeffs, nupchan):
        assert coeffs is not None and len(coeffs) == ntap * nupchan and coeffs.dtype == np.float32
        self.ntap, self.h, self.hist = ntap, np.asarray(coeffs, np.float64), None

    def stream(self, vin, nupchan):
        """(history + gulp, start of the gulp in it)"""
        nh = (self.ntap - 1) * nupchan
        prev = self.hist if self.hist is not None else np.zeros((nh,) + vin.shape[1:], np.uint8)
        return np.concatenate([prev, vin]), nh

    def taps(self, nupchan):
        """h, or the plain FFT's ones without coefficients"""
        return self.h if self.h is not None else np.ones(nupchan)

    def refresh(self, vin, nupchan):
        nh = (self.ntap - 1) * nupchan
        self.hist = vin[len(vin) - nh:].copy() if nh else None


class PfbUpchanBackend(OracleBackend):
    """The oracle backend plus xengUpchan* with the PFB served by the float64 restatement."""

    def __init__(self):
        super().__init__()
        self.up, self.pfb, self.calls = None, _History(), []

    def upchan_initialize(self, gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum):
        self.up = dict(ninput=ninput, nchan=nchan, ntime=ntime, nupchan=nupchan, nbeam=nbeam, nframe_sum=nframe_sum)
        self.pfb = _History()
        return 0

    def upchan_set_pfb(self, ntap, coeffs):
        self.pfb.set(ntap, coeffs, self.up['nupchan'])
        self.calls.append(('set_pfb', ntap))
        return 0

    def upchan_reset(self):
        self.pfb.hist = None
        self.calls.append('reset')

    def _run(self, vin, out_arr, weights, kind):
        u = self.up
        vin = vin.reshape(u['ntime'], u['nchan'], u['ninput'])
        w = weights.numpy().reshape(u['nchan'], u['nupchan'], u['nbeam'], u['ninput'])
        s, t0 = self.pfb.stream(vin, u['nupchan'])
        r = upchan_beamform_pfb(s, w, u['nupchan'], u['nbeam'], self.pfb.taps(u['nupchan']), t0, u['ntime'], u['nframe_sum'])
        out_arr.numpy().reshape(-1).view(np.float32 if u['nframe_sum'] else np.complex64)[...] = r.reshape(-1)
        self.pfb.refresh(vin, u['nupchan'])
        self.calls.append(kind)
        return 0

    def upchan_run(self, in_arr, out_arr, weights, version=0):
        return self._run(_u8(in_arr), out_arr, weights, 'run')

    def upchan_run_parts(self, part0, ntime0, part1, out_arr, weights, version=0):
        assert ntime0 % self.up['nupchan'] == 0
        return self._run(np.concatenate([_u8(part0), _u8(part1)]), out_arr, weights, ('parts', ntime0))

    def upchan_mark(self):
        return self.beam_mark()

    def upchan_wait(self, ticket):
        self.beam_wait(ticket)

    def upchan_sync(self):
        pass


class PfbUpchanCorrBackend(OracleBackend):
    """The oracle backend plus xengUpchanCorr* with the PFB: the frames of each gulp through the restatement, summed at dump."""

    def __init__(self):
        super().__init__()
        self.uc, self.pfb, self.X, self.calls = None, _History(), [], []

    def upchan_corr_initialize(self, gpu, ninput, nchan, ntime, nupchan, fine_lo, fine_hi, nstage=0):
        self.uc = dict(ninput=ninput, nchan=nchan, ntime=ntime, nupchan=nupchan, fine_lo=fine_lo, fine_hi=fine_hi)
        self.pfb = _History()
        return 0

    def upchan_corr_set_pfb(self, ntap, coeffs):
        self.pfb.set(ntap, coeffs, self.uc['nupchan'])
        self.calls.append(('set_pfb', ntap))
        return 0

    def _gulp(self, v):
        u = self.uc
        return v.reshape(u['ntime'], u['nchan'], u['ninput'])

    def _accumulate(self, vin, kind):
        u = self.uc
        s, t0 = self.pfb.stream(vin, u['nupchan'])
        self.X.append(pfb_fine_select(s, u['nupchan'], self.pfb.taps(u['nupchan']), t0, u['ntime'], u['fine_lo'], u['fine_hi']))
        self.pfb.refresh(vin, u['nupchan'])
        self.calls.append(kind)
        return 0

    def upchan_corr_accumulate(self, in_arr):
        return self._accumulate(self._gulp(_u8(in_arr)), 'run')

    def upchan_corr_accumulate_parts(self, part0, ntime0, part1):
        return self._accumulate(self._gulp(np.concatenate([_u8(part0), _u8(part1)])), 'parts')

    def upchan_corr_prime(self, in_arr):
        self.pfb.refresh(self._gulp(_u8(in_arr)), self.uc['nupchan'])
        self.calls.append('prime')
        return 0

    def upchan_corr_prime_parts(self, part0, ntime0, part1):
        self.pfb.refresh(self._gulp(np.concatenate([_u8(part0), _u8(part1)])), self.uc['nupchan'])
        self.calls.append('prime')
        return 0

    def upchan_corr_dump(self, out_arr):
        V, _ = upchan_corr_pfb(np.concatenate(self.X))
        out_arr.numpy().reshape(-1).view(np.complex64)[...] = V.reshape(-1)
        self.X = []
        self.calls.append('dump')
        return 0

    def upchan_corr_reset(self):
        self.X, self.pfb.hist = [], None
        self.calls.append('reset')

    def upchan_corr_mark(self):
        return self.beam_mark()

    def upchan_corr_wait(self, ticket):
        self.beam_wait(ticket)

    def upchan_corr_sync(self):
        pass


class _Data:
    def __init__(self, a):
        self.a = a.reshape(-1)
        self.nbytes = a.nbytes

    def numpy(self):
        return self.a


class _FakeSeq:
    """An input sequence whose reader saw only some gulps (ispan.offset tells where each one was); split: samples in the first
    of two parts (None: one part)."""

    def __init__(self, hdr, gulps, igulp, split=None, row=None):
        self.header = types.SimpleNamespace(tostring=lambda: json.dumps(hdr).encode())
        self.gulps, self.igulp, self.split, self.row = gulps, igulp, split, row
        self.time_tag = hdr['seq0']

    def read(self, n):
        for k, a in self.gulps:
            parts = None
            if self.split is not None:
                flat = a.reshape(-1)
                parts = [_Data(flat[:self.split * self.row]), _Data(flat[self.split * self.row:])]
            yield types.SimpleNamespace(size=a.nbytes, offset=k * self.igulp, data=_Data(a), parts=parts)


class _FakeRing:
    span_memory_outlives_release = False
    name = "fake-input"

    def __init__(self, seqs):
        self.seqs = seqs

    def read(self, guarantee=True):
        return iter(self.seqs)


# ---------------------------------------------------------------- the restatement and the default coefficients
def test_restatement_is_the_definition():
    """pfb_channelise against a direct loop over y[f, n] = sum_k h[k*N + n] x[(f - P + 1 + k)*N + n] (zeros before `first`)
    and the DFT with the fftshift written out; with P = 1 and h = 1 it is channelise()."""
    rng = np.random.default_rng(11)
    N, P, nchan, ninput = 4, 3, 2, 3
    T = 6 * N
    stream = rng.integers(0, 256, (T, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N)
    re, im = orc.decode(stream)
    x = re + 1j * im
    start, ntime, first = 2 * N, 3 * N, N
    X = pfb_channelise(stream, N, h, start, ntime, first)
    for f in range(ntime // N):
        y = np.zeros((N, nchan, ninput), np.complex128)
        for n in range(N):
            for k in range(P):
                t = start + (f - P + 1 + k) * N + n
                if t >= first:
                    y[n] += h[k * N + n] * x[t]
        for j in range(N):
            kk = (j + N // 2) % N
            d = sum(y[n] * np.exp(-2j * np.pi * kk * n / N) for n in range(N))
            assert np.allclose(X[f, :, :, j], d, atol=1e-9)
    assert np.allclose(pfb_channelise(stream, N, np.ones(N), 0, T), channelise(stream, N), atol=1e-12)
    assert np.allclose(pfb_channelise(stream, N, np.ones(N), start, ntime), channelise(stream[start:start + ntime], N), atol=1e-12)


@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_default_coefficients_and_their_leakage(N):
    """P*N values, symmetric, sum N; the worst steady-state leakage of a tone into channels >= 2 away (float64) is <= -55 dB
    at 4 taps and <= -40 dB at 2, against >= -12 dB for the plain FFT."""
    for P in (1, 2, 4, 8):
        h = pfb_coeffs(P, N)
        assert h.dtype == np.float32 and h.shape == (P * N,)
        assert np.array_equal(h, h[::-1])
        assert abs(float(h.astype(np.float64).sum()) - N) < 1e-4 * N
    assert tone_leakage_db(pfb_coeffs(4, N), N) <= -55
    assert tone_leakage_db(pfb_coeffs(2, N), N) <= -40
    assert tone_leakage_db(np.ones(N), N) >= -12


# ---------------------------------------------------------------- UpchanBeamform
def _beam_out(spans, shape):
    return [s.view(np.complex64).reshape(shape) for s in spans]


def test_upchan_beamform_pfb_over_gulps_sequences_and_two_part_gulps():
    """Two sequences on CPU rings, gulps in two parts split inside the last P-1 frames: every output equals the restatement over
    the sequence's continuous stream; the history is reset at each sequence start; SetPfb gets the default coefficients; the
    header carries pfb_ntap."""
    nchan, nstand, nbeam, N, P, g = 2, 2, 3, 8, 4, 32
    ninput = 2 * nstand
    rng = np.random.default_rng(12)
    vins = [rng.integers(0, 256, (3 * g, nchan, ninput), dtype=np.uint8), rng.integers(0, 256, (2 * g, nchan, ninput), dtype=np.uint8)]
    hdrs = [source_header(nchan, nstand, 2, seq0=s, sfreq=30e6) for s in (1000, 5000)]
    span = g // 2                                   # (the split after 16 samples: the 24-sample tail straddles it)
    r0, r1 = Ring("gpu-input"), Ring("up-output")
    r0.resize(span, 8 * g * nchan * ninput)
    be = PfbUpchanBackend()
    up = UpchanBeamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, backend=be, pfb_ntap=P)
    w = (rng.standard_normal(up.weights_cpu.shape) + 1j * rng.standard_normal(up.weights_cpu.shape)).astype(np.complex64)
    up.weights_cpu[...] = w
    sink = Sink(r1, (g // N) * nbeam * nchan * N * 8)
    run_blocks([up], Source(r0, [(hdrs[0], vins[0], span * nchan * ninput), (hdrs[1], vins[1], span * nchan * ninput)]), [sink])
    assert be.calls == [('set_pfb', P), 'reset', ('parts', span), ('parts', span), ('parts', span), 'reset', ('parts', span), ('parts', span)]
    assert np.array_equal(be.pfb.h, pfb_coeffs(P, N).astype(np.float64))
    assert len(sink.sequences) == 2
    for (ohdr, _, spans), vin in zip(sink.sequences, vins):
        assert ohdr['pfb_ntap'] == P
        got = _beam_out(spans, (g // N, nbeam, nchan, N))
        assert len(got) == len(vin) // g
        for k, o in enumerate(got):
            exp = upchan_beamform_pfb(vin, w, N, nbeam, pfb_coeffs(P, N), k * g, g)
            assert np.allclose(o, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())
        # (the filter really reaches back: gulp 1 differs from the same gulp without its history)
        alone = upchan_beamform_pfb(vin[g:2 * g], w, N, nbeam, pfb_coeffs(P, N), 0, g)
        assert not np.allclose(got[1][0], alone[0], rtol=1e-3, atol=1e-3 * np.abs(alone).max())


@pytest.mark.parametrize("split", [None, 24])
def test_upchan_beamform_pfb_resets_after_a_gap(split):
    """Gulp 3 of 6 never read: the block resets the history before gulp 4 (its first frames see zeros, not gulp 2's tail), and
    at the sequence's start; each output equals the restatement with the samples before the reset taken as zero."""
    nchan, nstand, nbeam, N, P, g, seq0 = 1, 2, 2, 8, 3, 32, 700
    ninput = 2 * nstand
    rng = np.random.default_rng(13)
    vin = rng.integers(0, 256, (6 * g, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32)
    seen = [(k, vin[k * g:(k + 1) * g]) for k in (0, 1, 2, 4, 5)]
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=1e6)
    r1 = Ring("up-output")
    be = PfbUpchanBackend()
    up = UpchanBeamform(LOG, _FakeRing([_FakeSeq(hdr, seen, g * nchan * ninput, split, nchan * ninput)]), r1, nchan=nchan, nbeam=nbeam,
                        ninput=ninput, ntime_gulp=g, nupchan=N, backend=be, pfb_ntap=P, pfb_coeffs=h)
    w = (rng.standard_normal(up.weights_cpu.shape) + 1j * rng.standard_normal(up.weights_cpu.shape)).astype(np.complex64)
    up.weights_cpu[...] = w
    sink = Sink(r1, (g // N) * nbeam * nchan * N * 8)
    sink.start()
    up.main()
    sink.join(20)
    kind = 'run' if split is None else ('parts', split)
    assert be.calls == [('set_pfb', P), 'reset', kind, kind, kind, 'reset', kind, kind]
    got = _beam_out(sink.sequences[0][2], (g // N, nbeam, nchan, N))
    for (k, _), o in zip(seen, got):
        exp = upchan_beamform_pfb(vin, w, N, nbeam, h, k * g, g, first=4 * g if k >= 4 else 0)
        assert np.allclose(o, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())


# ---------------------------------------------------------------- UpchanCorr
def _corr_expect(stream, N, h, gulps, first, fine_lo=0, fine_hi=None, g=None):
    X = np.concatenate([pfb_fine_select(stream, N, h, k * g, g, fine_lo, fine_hi, first) for k in gulps])
    return upchan_corr_pfb(X)[0]


def test_upchan_corr_pfb_keeps_the_history_across_integrations_and_sequences():
    """Two integrations of 2 gulps each in one sequence (two-part gulps): the history carries across the dump between them;
    a second sequence starts from zeros (reset at its start)."""
    nchan, nstand, N, P, g = 2, 2, 4, 4, 16
    ninput = 2 * nstand
    rng = np.random.default_rng(14)
    vins = [rng.integers(0, 256, (4 * g, nchan, ninput), dtype=np.uint8), rng.integers(0, 256, (2 * g, nchan, ninput), dtype=np.uint8)]
    hdrs = [source_header(nchan, nstand, 2, seq0=s, sfreq=40e6, chan_bw=25e3) for s in (0, 9000)]
    span = g // 2
    r0, r1 = Ring("gpu-input"), Ring("uc-output")
    r0.resize(span * nchan * ninput, 8 * g * nchan * ninput)
    be = PfbUpchanCorrBackend()
    uc = UpchanCorr(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=2 * g // N, fine_lo=1,
                    fine_hi=7, backend=be, pfb_ntap=P)
    sink = Sink(r1, 6 * ninput * ninput * 8)
    run_blocks([uc], Source(r0, [(hdrs[0], vins[0], span * nchan * ninput), (hdrs[1], vins[1], span * nchan * ninput)]), [sink])
    assert be.calls == [('set_pfb', P), 'reset', 'parts', 'parts', 'dump', 'parts', 'parts', 'dump', 'reset', 'parts', 'parts', 'dump']
    h = pfb_coeffs(P, N)
    spans = [s for _, _, ss in sink.sequences for s in ss]
    exps = [_corr_expect(vins[0], N, h, (0, 1), 0, 1, 7, g), _corr_expect(vins[0], N, h, (2, 3), 0, 1, 7, g),
            _corr_expect(vins[1], N, h, (0, 1), 0, 1, 7, g)]
    assert len(spans) == 3 and all(hd['pfb_ntap'] == P for hd, _, _ in sink.sequences)
    for s, e in zip(spans, exps):
        assert np.allclose(s.view(np.complex64).reshape(e.shape), e, rtol=1e-5, atol=1e-5 * np.abs(e).max())
    cold = _corr_expect(vins[0][2 * g:], N, h, (0, 1), 0, 1, 7, g)      # (the second integration without the first's tail)
    assert not np.allclose(spans[1].view(np.complex64).reshape(cold.shape), cold, rtol=1e-3, atol=1e-3 * np.abs(cold).max())


R, D = 'run', 'dump'


@pytest.mark.parametrize("missing,calls", [
    ((3,), ['reset', R, R, D, R, 'reset', R, R, D, R, R, D, R, R, D]),                 # (gulp 3 was the one before the boundary)
    ((2, 3), ['reset', R, R, D, 'reset', R, R, D, R, R, D, R, R, D]),                  # (a gap right after a dump resets too)
    ((4,), ['reset', R, R, D, R, R, D, 'reset', 'prime', R, R, D, R, R, D]),
    ((4, 5, 6), ['reset', R, R, D, R, R, D, 'reset', 'prime', R, R, D]),
])
def test_upchan_corr_pfb_gap_resets_and_primes_before_the_boundary(missing, calls):
    """2 gulps per integration, 10 gulps, `missing` never read.  Every gap resets the history -- also right after a dump, when
    no integration is in progress -- and while the block waits for the next boundary it primes with the gulp before it, so the
    integration after the gap sees that gulp's tail; each written integration equals the restatement."""
    nchan, nstand, N, P, g, ngulp, seq0 = 1, 2, 4, 3, 8, 10, 500
    ninput = 2 * nstand
    rng = np.random.default_rng(15)
    vin = rng.integers(0, 256, (ngulp * g, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32)
    seen = [(k, vin[k * g:(k + 1) * g]) for k in range(ngulp) if k not in missing]
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=1e6)
    r1 = Ring("uc-output")
    be = PfbUpchanCorrBackend()
    uc = UpchanCorr(LOG, _FakeRing([_FakeSeq(hdr, seen, g * nchan * ninput)]), r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N,
                    nframe_per_integration=2 * g // N, backend=be, pfb_ntap=P, pfb_coeffs=h)
    sink = Sink(r1, nchan * N * ninput * ninput * 8)
    sink.start()
    uc.main()
    sink.join(20)
    assert be.calls[0] == ('set_pfb', P) and be.calls[1:] == calls
    done = [k for k in range(0, ngulp, 2) if k not in missing and k + 1 not in missing]
    spans = [s for _, _, ss in sink.sequences for s in ss]
    assert len(spans) == len(done)
    last_gap = max(missing)
    for k, s in zip(done, spans):
        # the samples seen without a break up to this integration: from the gap (or seq0), primed with the gulp before k
        first = 0 if k < last_gap else (last_gap + 1) * g
        e = _corr_expect(vin, N, h, (k, k + 1), first, g=g)
        assert np.allclose(s.view(np.complex64).reshape(e.shape), e, rtol=1e-5, atol=1e-5 * np.abs(e).max())


# ---------------------------------------------------------------- pfb_ntap=1: nothing new is called
class _NoPfbMixin:
    def upchan_set_pfb(self, *a):
        raise AssertionError("upchan_set_pfb called at pfb_ntap=1")

    def upchan_reset(self, *a):
        raise AssertionError("upchan_reset called at pfb_ntap=1")

    def upchan_corr_set_pfb(self, *a):
        raise AssertionError("upchan_corr_set_pfb called at pfb_ntap=1")

    def upchan_corr_prime(self, *a):
        raise AssertionError("upchan_corr_prime called at pfb_ntap=1")

    def upchan_corr_prime_parts(self, *a):
        raise AssertionError("upchan_corr_prime_parts called at pfb_ntap=1")


class _NoPfbUpchan(_NoPfbMixin, PfbUpchanBackend):
    pass


class _NoPfbCorr(_NoPfbMixin, PfbUpchanCorrBackend):
    pass


def test_pfb_ntap_1_makes_no_new_backend_call():
    """Both blocks at the default pfb_ntap=1 through a sequence with a gap: none of the new methods is called, the output is the
    plain FFT's, the header has no pfb_ntap, and UpchanCorr resets only when an integration was in progress (as before)."""
    nchan, nstand, nbeam, N, g = 1, 2, 2, 8, 16
    ninput = 2 * nstand
    rng = np.random.default_rng(16)
    vin = rng.integers(0, 256, (8 * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=1e6)
    seen = [(k, vin[k * g:(k + 1) * g]) for k in (0, 1, 3, 4, 5, 6, 7)]
    be = _NoPfbUpchan()
    r1 = Ring("up-output")
    up = UpchanBeamform(LOG, _FakeRing([_FakeSeq(hdr, seen, g * nchan * ninput)]), r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g,
                        nupchan=N, backend=be)
    up.weights_cpu[...] = 1
    sink = Sink(r1, (g // N) * nbeam * nchan * N * 8)
    sink.start()
    up.main()
    sink.join(20)
    assert be.calls == ['run'] * 7 and 'pfb_ntap' not in sink.sequences[0][0]
    for (k, _), o in zip(seen, _beam_out(sink.sequences[0][2], (g // N, nbeam, nchan, N))):
        exp = upchan_beamform_pfb(vin[k * g:(k + 1) * g], np.ones((nchan, N, nbeam, ninput)), N, nbeam, np.ones(N), 0, g)
        assert np.allclose(o, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())

    be = _NoPfbCorr()
    r1 = Ring("uc-output")
    uc = UpchanCorr(LOG, _FakeRing([_FakeSeq(hdr, seen, g * nchan * ninput)]), r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N,
                    nframe_per_integration=2 * g // N, backend=be)
    sink = Sink(r1, nchan * N * ninput * ninput * 8)
    sink.start()
    uc.main()
    sink.join(20)
    assert be.calls == ['run', 'run', 'dump', 'run', 'run', 'dump', 'run', 'run', 'dump']      # (gulp 2 missing after a dump: no reset, gulp 3 skipped)
    assert all('pfb_ntap' not in hd for hd, _, _ in sink.sequences)


# ---------------------------------------------------------------- argument checks
@pytest.mark.parametrize("kw", [dict(pfb_ntap=0), dict(pfb_ntap=9), dict(pfb_ntap=2.0), dict(pfb_ntap=2, pfb_coeffs=np.ones(8)),
                                dict(pfb_ntap=2, pfb_coeffs=np.r_[np.ones(15), np.nan]), dict(pfb_ntap=1, pfb_coeffs=np.r_[np.ones(7), np.inf]),
                                dict(pfb_ntap=6)])
def test_block_constructors_refuse_bad_pfb_arguments(kw):
    """Taps outside 1..8, a wrong number of coefficients, non-finite ones, a gulp (32 samples) shorter than the history."""
    with pytest.raises(ValueError, match="UPCHAN"):
        UpchanBeamform(LOG, Ring("a"), Ring("b"), nchan=1, nbeam=1, ninput=4, ntime_gulp=32, nupchan=8, backend=PfbUpchanBackend(), **kw)
    with pytest.raises(ValueError, match="UPCHAN_CORR"):
        UpchanCorr(LOG, Ring("a"), Ring("b"), nchan=1, ninput=4, ntime_gulp=32, nupchan=8, nframe_per_integration=4,
                   backend=PfbUpchanCorrBackend(), **kw)


def test_pfb_ntap_1_with_coefficients_is_a_windowed_fft():
    """pfb_ntap=1 with coefficients: SetPfb is called (a windowed FFT), no history call is made."""
    be = PfbUpchanBackend()
    h = np.hanning(8).astype(np.float32)
    up = UpchanBeamform(LOG, Ring("a"), Ring("b"), nchan=1, nbeam=1, ninput=4, ntime_gulp=32, nupchan=8, backend=be, pfb_ntap=1, pfb_coeffs=h)
    assert be.calls == [('set_pfb', 1)] and np.array_equal(be.pfb.h, h.astype(np.float64)) and up.pfb
    assert up.output_header(source_header(1, 2, 2))['pfb_ntap'] == 1


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Reset and Prime are enqueue-only, SetPfb (it waits) is not.  SetPfb refuses
    ntap 0 or 9 and NULL coefficients with ntap > 1 before it looks for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in ("xengUpchanSetPfb", "xengUpchanReset", "xengUpchanCorrSetPfb", "xengUpchanCorrPrime", "xengUpchanCorrPrimeParts"):
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengUpchanReset", "xengUpchanCorrReset", "xengUpchanCorrPrime", "xengUpchanCorrPrimeParts"):
        assert name in ffi.ENQUEUE_ONLY, name
    assert "xengUpchanSetPfb" not in ffi.ENQUEUE_ONLY and "xengUpchanCorrSetPfb" not in ffi.ENQUEUE_ONLY
    h = np.ones(64 * 8, np.float32)
    hp = h.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name in ("xengUpchanSetPfb", "xengUpchanCorrSetPfb"):
        for ntap, coeffs in ((0, hp), (9, hp), (-1, None), (2, None), (8, None)):
            with pytest.raises(ffi.XengError) as ei:
                ffi.call(name, ntap, coeffs)
            assert ei.value.status == INVALID_ARGUMENT, (name, ntap)
    for name, args in (("xengUpchanCorrPrime", (None,)), ("xengUpchanCorrPrimeParts", (4096, 0, 4096)), ("xengUpchanCorrPrimeParts", (4096, 32, None))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_upchan_pfb_gpu.py covers the rest)
    for name, args in (("xengUpchanSetPfb", (4, hp)), ("xengUpchanSetPfb", (1, None)), ("xengUpchanReset", ()),
                       ("xengUpchanCorrSetPfb", (4, hp)), ("xengUpchanCorrPrime", (4096,)), ("xengUpchanCorrPrimeParts", (4096, 32, 4096))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
