"""UpchanSumBeams without a GPU, both ring implementations: the float64 restatement (tests/upchan_beams_ref.py) against a
frame-by-frame np.fft loop and, through the linearity of the beamformer, against UpchanBeamform's dual-pol PFB restatement;
windows spanning gulps against one long window; the block on CPU rings with an oracle backend that keeps the context's state
(window position, accumulator, PFB history) -- windows within and across gulps, alignment to seq0, gaps (dropped windows,
realignment, a new output sequence, the PFB primed before the boundary), sequence restarts, pair selection, header keys,
refusals -- and the C entry points' argument checks."""
import ctypes

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanSumBeams
from caltech_bifrost_dsp_amd.ring import Ring
from oracle import xeng_oracle as orc
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.upchan_beams_ref import beam_channelise, sum_beams, upchan_sum_beams
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq
from tests.upchan_pfb_ref import upchan_beamform_pfb

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def _beams(rng, nchan, nbeam, ntime):
    return (rng.standard_normal((nchan, nbeam, ntime)) + 1j * rng.standard_normal((nchan, nbeam, ntime))).astype(np.complex64)


def _gulps(v, g):
    """The gulps of a beam stream as Beamform writes them: cf32 [nchan][nbeam][g] each."""
    return [np.ascontiguousarray(v[..., k * g:(k + 1) * g]) for k in range(v.shape[-1] // g)]


def _ring_bytes(v, g):
    """The stream as the ring holds it: its gulps one after the other."""
    return np.concatenate([a.reshape(-1) for a in _gulps(v, g)])


def beam_header(nchan, nbeam, seq0=0, **extra):
    hdr = source_header(nchan, nbeam, 1, seq0=seq0, sfreq=1e6)
    hdr.update(nbeam=nbeam, nstand=nbeam, npol=1, nbit=32, complex=True)
    hdr.update(extra)
    return hdr


class SumBeamsBackend(OracleBackend):
    """The oracle backend plus xengUpchanSumBeams* served by the float64 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.ub, self.calls = None, []

    def upchan_sum_beams_initialize(self, gpu, nchan, nbeam, ntime, nupchan, pair0, npair, nframe_sum):
        self.ub = dict(nchan=nchan, nbeam=nbeam, ntime=ntime, N=nupchan, pair0=pair0, npair=npair, W=nframe_sum, F=ntime // nupchan)
        self.gpw = max(1, nframe_sum // (ntime // nupchan))
        self.pos, self.acc, self.ntap, self.h, self.hist = 0, None, 1, None, None
        return 0

    def upchan_sum_beams_set_pfb(self, ntap, coeffs):
        assert coeffs is not None and coeffs.dtype == np.float32 and coeffs.size == ntap * self.ub['N']
        self.ntap, self.h, self.hist = ntap, np.asarray(coeffs, np.float64), None
        self.calls.append(('set_pfb', ntap))
        return 0

    def _gulp(self, in_arr):
        u = self.ub
        return in_arr.numpy().reshape(-1).view(np.uint8).view(np.complex64).reshape(u['nchan'], u['nbeam'], u['ntime'])

    def _keep_tail(self, v):
        nh = (self.ntap - 1) * self.ub['N']
        self.hist = v[..., v.shape[-1] - nh:].copy() if nh else None

    def upchan_sum_beams_run(self, in_arr, out_arr):
        u = self.ub
        v = self._gulp(in_arr)
        nh = (self.ntap - 1) * u['N']
        prev = self.hist if self.hist is not None else np.zeros(v.shape[:2] + (nh,), np.complex64)
        V = beam_channelise(np.concatenate([prev, v], axis=-1), u['N'], self.h, nh, u['ntime'])
        if self.gpw == 1:
            r = sum_beams(V, u['W'], u['pair0'], u['npair'])
        else:
            part = sum_beams(V, u['F'], u['pair0'], u['npair'])
            self.acc = part if self.pos == 0 else self.acc + part
            r = self.acc
        if self.pos == self.gpw - 1:
            out_arr.numpy().reshape(-1).view(np.uint8).view(np.float32)[...] = r.reshape(-1)
        else:
            assert out_arr is None
        self.pos = (self.pos + 1) % self.gpw
        self._keep_tail(v)
        self.calls.append('run')
        return 0

    def upchan_sum_beams_prime(self, in_arr):
        self._keep_tail(self._gulp(in_arr))
        self.calls.append('prime')
        return 0

    def upchan_sum_beams_reset(self):
        self.pos, self.acc, self.hist = 0, None, None
        self.calls.append('reset')

    def upchan_sum_beams_mark(self):
        return self.beam_mark()

    def upchan_sum_beams_wait(self, ticket):
        self.beam_wait(ticket)

    def upchan_sum_beams_sync(self):
        pass


def _out(spans, shape):
    return [s.view(np.float32).reshape(shape) for s in spans]


def _close(got, exp):
    assert np.allclose(got, exp, rtol=1e-5, atol=1e-5 * np.abs(exp).max())


# ---------------------------------------------------------------- the restatement
def test_restatement_is_np_fft_per_frame():
    """Frame by frame: np.fft of each beam's N samples, fftshifted, the 2x2 products of beams 2p / 2p+1 added per window."""
    nchan, nbeam, N, W, nframe = 2, 6, 8, 3, 6
    rng = np.random.default_rng(1)
    v = _beams(rng, nchan, nbeam, N * nframe)
    got = upchan_sum_beams(v, N, W, 0, N * nframe, pair0=1, npair=2)
    exp = np.zeros((nframe // W, 2, nchan, N, 4))
    for f in range(nframe):
        for c in range(nchan):
            for q, p in enumerate((1, 2)):
                X = np.fft.fftshift(np.fft.fft(v[c, 2 * p, f * N:(f + 1) * N].astype(np.complex128)))
                Y = np.fft.fftshift(np.fft.fft(v[c, 2 * p + 1, f * N:(f + 1) * N].astype(np.complex128)))
                exp[f // W, q, c, :, 0] += np.abs(X) ** 2
                exp[f // W, q, c, :, 1] += np.abs(Y) ** 2
                exp[f // W, q, c, :, 2] += X.real * Y.real + X.imag * Y.imag
                exp[f // W, q, c, :, 3] += X.imag * Y.real - X.real * Y.imag
    assert np.allclose(got, exp, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("P", [1, 3])
def test_pfb_path_is_upchan_beamform_dual_pol_with_coarse_weights(P):
    """Beams formed from 4-bit input with coarse weights, then the restatement (PFB, FFT, products), equal upchan_pfb_ref's
    dual-pol UpchanBeamform of the same input with the weights copied to every fine channel: the linearity the feature rests on."""
    nchan, ninput, nbeam, N, W, ntime = 2, 8, 4, 8, 2, 64
    rng = np.random.default_rng(2 + P)
    vin = rng.integers(0, 256, (2 * ntime, nchan, ninput), dtype=np.uint8)
    w = rng.standard_normal((nchan, nbeam, ninput)) + 1j * rng.standard_normal((nchan, nbeam, ninput))
    h = rng.standard_normal(P * N) if P > 1 else np.ones(N)
    re, im = orc.decode(vin)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    v = np.einsum('cbi,tci->cbt', w, x)
    got = upchan_sum_beams(v, N, W, ntime, ntime, h)
    wf = np.broadcast_to(w[:, None], (nchan, N, nbeam, ninput))
    exp = upchan_beamform_pfb(vin, wf, N, nbeam, h, ntime, ntime, W, dual_pol=True)
    assert np.allclose(got, exp, rtol=1e-10, atol=1e-9 * np.abs(exp).max())


def test_windows_spanning_gulps_equal_one_long_window():
    """G = 3 gulps per window with a 4-tap PFB: the per-gulp partial sums (each gulp's frames with the history of the one
    before), added in order, equal the restatement of one window over the three gulps."""
    nchan, nbeam, N, g, P = 2, 4, 16, 64, 4
    rng = np.random.default_rng(4)
    v = _beams(rng, nchan, nbeam, 3 * g)
    h = rng.standard_normal(P * N)
    parts = [sum_beams(beam_channelise(v, N, h, k * g, g), g // N) for k in range(3)]
    assert np.allclose(parts[0] + parts[1] + parts[2], upchan_sum_beams(v, N, 3 * g // N, 0, 3 * g, h), rtol=1e-12, atol=1e-9)


# ---------------------------------------------------------------- the block on CPU rings
@pytest.mark.parametrize("span", [False, True])
def test_block_windows_within_and_across_gulps_over_two_sequences(span):
    """Source -> UpchanSumBeams -> Sink on in-repo rings, two sequences of 4 gulps.  W = F/2: one span per gulp holding two
    windows; W = 2F: one span per two gulps.  Each sequence starts from a reset (the second does not see the first's tail);
    every span equals the restatement; the header carries the keys of UpchanBeamform's dual-pol output."""
    nchan, nbeam, N, g, P = 2, 6, 8, 64, 2
    F = g // N
    W = 2 * F if span else F // 2
    rng = np.random.default_rng(5 + span)
    vs = [_beams(rng, nchan, nbeam, 4 * g) for _ in range(2)]
    h = rng.standard_normal(P * N).astype(np.float32)
    hdrs = [beam_header(nchan, nbeam, seq0=1000 * (s + 1)) for s in range(2)]
    r0, r1 = Ring("bf-output"), Ring("ub-output")
    be = SumBeamsBackend()
    ub = UpchanSumBeams(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ntime_gulp=g, nupchan=N, nframe_sum=W, backend=be, pfb_ntap=P, pfb_coeffs=h)
    shape = (max(F // W, 1), nbeam // 2, nchan, N, 4)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([ub], Source(r0, [(hdrs[s], _ring_bytes(vs[s], g), nchan * nbeam * g * 8) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    per = 2 if span else 1
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hdrs[s]['seq0'] and hd['seq0'] == hdrs[s]['seq0']
        assert len(spans) == 4 // per
        for k, o in enumerate(_out(spans, shape)):
            _close(o, upchan_sum_beams(vs[s], N, W, k * per * g, per * g, h))
    hd = sink.sequences[0][0]
    assert hd['nupchan'] == N and hd['nframe_sum'] == W and hd['acc_len'] == W * N and hd['pfb_ntap'] == P and hd['pair0'] == 0
    assert hd['nbeam'] == hd['nstand'] == nbeam // 2 and hd['npol'] == 2 and hd['complex'] is True and hd['nbit'] == 32
    chan_bw = hdrs[0]['bw_hz'] / nchan
    assert hd['fine_bw_hz'] == chan_bw / N and hd['fine_sfreq'] == hdrs[0]['sfreq'] - chan_bw / 2
    assert be.calls == [('set_pfb', P)] + (['reset'] + ['run'] * 4) * 2


def test_block_pair_selection():
    """pair0 = 1, npair = 1 of 3 pairs: beams 2 and 3 only; the header says so."""
    nchan, nbeam, N, g = 1, 6, 16, 64
    rng = np.random.default_rng(6)
    v = _beams(rng, nchan, nbeam, 2 * g)
    r0, r1 = Ring("bf-output"), Ring("ub-output")
    ub = UpchanSumBeams(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ntime_gulp=g, nupchan=N, nframe_sum=2, pair0=1, npair=1, backend=SumBeamsBackend())
    shape = (2, 1, nchan, N, 4)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([ub], Source(r0, [(beam_header(nchan, nbeam), _ring_bytes(v, g), nchan * nbeam * g * 8)]), [sink])
    hd, _, spans = sink.sequences[0]
    assert hd['pair0'] == 1 and hd['nbeam'] == 1 and 'pfb_ntap' not in hd
    for k, o in enumerate(_out(spans, shape)):
        _close(o, upchan_sum_beams(v, N, 2, k * g, g, pair0=1, npair=1))


R = 'run'


@pytest.mark.parametrize("missing,calls", [
    # G = 2 gulps per window, 10 gulps of the sequence, `missing` never read
    ((3,), ['reset', R, R, R, 'reset', R, R, R, R, R, R]),                          # (window 2-3 lost; gulp 4 is a boundary)
    ((4,), ['reset', R, R, R, R, 'reset', 'prime', R, R, R, R]),                    # (gulp 5 primes the window 6-7)
    ((0,), ['reset', 'reset', 'prime', R, R, R, R, R, R, R, R]),                    # (alignment to seq0: gulp 1 only primes)
    ((4, 5, 6), ['reset', R, R, R, R, 'reset', 'prime', R, R]),
])
def test_block_gap_mid_window_drops_realigns_and_primes(missing, calls):
    """Every gap resets the context (the window in progress and the PFB history go); the output restarts in a new sequence at
    the next window boundary (aligned to seq0, which is not a multiple of the window), primed with the gulp before it when that
    gulp was read.  Each written window equals the restatement of the samples seen without a break."""
    nchan, nbeam, N, g, P, ngulp, seq0 = 1, 4, 8, 32, 3, 10, 700
    rng = np.random.default_rng(sum(missing) + 17)
    v = _beams(rng, nchan, nbeam, ngulp * g)
    h = rng.standard_normal(P * N).astype(np.float32)
    seen = [(k, a) for k, a in enumerate(_gulps(v, g)) if k not in missing]
    be = SumBeamsBackend()
    r1 = Ring("ub-output")
    ub = UpchanSumBeams(LOG, _FakeRing([_FakeSeq(beam_header(nchan, nbeam, seq0=seq0), seen, nchan * nbeam * g * 8)]), r1, nchan=nchan, nbeam=nbeam,
                        ntime_gulp=g, nupchan=N, nframe_sum=2 * g // N, backend=be, pfb_ntap=P, pfb_coeffs=h)
    shape = (1, nbeam // 2, nchan, N, 4)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    sink.start()
    ub.main()
    sink.join(20)
    assert be.calls[0] == ('set_pfb', P) and be.calls[1:] == calls
    done = [k for k in range(0, ngulp, 2) if k not in missing and k + 1 not in missing]
    spans = [(hd, s) for hd, _, ss in sink.sequences for s in ss]
    assert len(spans) == len(done)
    last_gap = max(missing)
    before, after = [k for k in done if k < last_gap], [k for k in done if k > last_gap]
    assert [hd['seq0'] for hd, _, _ in sink.sequences] == [seq0 + ks[0] * g for ks in (before, after) if ks]
    for k, (hd, s) in zip(done, spans):
        first = 0 if k < last_gap else (last_gap + 1) * g
        _close(s.view(np.float32).reshape(shape), upchan_sum_beams(v, N, 2 * g // N, k * g, 2 * g, h, first=first))
    assert ub.stats['ndropped'] >= 1


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(nupchan=4), dict(nupchan=128), dict(ntime_gulp=60), dict(nframe_sum=3), dict(nframe_sum=12),
                                dict(nframe_sum=0), dict(pair0=2), dict(pair0=1, npair=2), dict(npair=0), dict(pfb_ntap=9),
                                dict(pfb_ntap=2, pfb_coeffs=np.ones(8)), dict(pfb_ntap=8, nupchan=16, nframe_sum=2)])
def test_constructor_refuses_bad_arguments(kw):
    """nupchan outside 8..64, gulps that are not whole frames, windows that neither divide nor are whole gulps (8 frames per
    gulp), pairs outside the 2 of 4 beams, bad PFB taps or coefficients, a gulp (64 samples) shorter than the history (7 x 16)."""
    args = dict(nchan=1, nbeam=4, ntime_gulp=64, nupchan=8, nframe_sum=4)
    args.update(kw)
    be = SumBeamsBackend()
    with pytest.raises(ValueError, match="UPCHAN_SUM_BEAMS"):
        UpchanSumBeams(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.ub is None                    # (refused before the context is made)


@pytest.mark.parametrize("bad", [dict(npol=2), dict(nbit=8), dict(complex=False), dict(nbeam=8), dict(nchan=2), dict(acc_len=24),
                                 dict(nupchan=32)])
def test_block_refuses_what_is_not_beamform_voltage_output(bad):
    """Dual-pol power (BeamformSumBeams), integrated or channelised products, other sizes: ValueError before any run."""
    nchan, nbeam, g = 1, 4, 64
    be = SumBeamsBackend()
    hdr = beam_header(nchan, nbeam)
    hdr.update(bad)
    ub = UpchanSumBeams(LOG, _FakeRing([_FakeSeq(hdr, [(0, np.zeros((nchan, nbeam, g), np.complex64))], nchan * nbeam * g * 8)]), Ring("b"),
                        nchan=nchan, nbeam=nbeam, ntime_gulp=g, nupchan=8, backend=be)
    with pytest.raises(ValueError, match="UPCHAN_SUM_BEAMS"):
        ub.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengUpchanSumBeamsInitialize", "xengUpchanSumBeamsGetInfo", "xengUpchanSumBeamsRun", "xengUpchanSumBeamsSetPfb", "xengUpchanSumBeamsPrime",
         "xengUpchanSumBeamsReset", "xengUpchanSumBeamsMark", "xengUpchanSumBeamsWait", "xengUpchanSumBeamsTicketDone", "xengUpchanSumBeamsSync",
         "xengUpchanSumBeamsDestroy")


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Prime, Reset, Mark and TicketDone are enqueue-only, the calls that wait are
    not.  Initialize refuses bad sizes before it touches a device; Run / Prime refuse null and misaligned pointers, SetPfb bad
    taps, GetInfo null results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengUpchanSumBeamsRun", "xengUpchanSumBeamsPrime", "xengUpchanSumBeamsReset", "xengUpchanSumBeamsMark", "xengUpchanSumBeamsTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengUpchanSumBeamsInitialize", "xengUpchanSumBeamsSetPfb", "xengUpchanSumBeamsWait", "xengUpchanSumBeamsSync"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, nchan, nbeam, ntime, nupchan, pair0, npair, nframe_sum): 30 frames of 32 per gulp
    for args in ((0, 0, 32, 960, 32, 0, 16, 30), (0, 96, 32, 960, 32, 0, 0, 30), (0, 96, 32, 960, 32, -1, 16, 30), (0, 96, 32, 960, 4, 0, 16, 30),
                 (0, 96, 32, 960, 128, 0, 16, 30), (0, 96, 32, 1000, 32, 0, 16, 25), (0, 96, 32, 960, 32, 0, 16, 20), (0, 96, 32, 960, 32, 0, 16, 45),
                 (0, 96, 32, 960, 32, 0, 16, 0), (0, 96, 32, 960, 32, 1, 16, 30), (0, 96, 32, 960, 32, 15, 2, 30)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanSumBeamsInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    h = np.ones(64 * 8, np.float32)
    hp = h.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name, args in (("xengUpchanSumBeamsRun", (None, 4096)), ("xengUpchanSumBeamsRun", (4104, 4096)), ("xengUpchanSumBeamsRun", (4096, 4100)),
                       ("xengUpchanSumBeamsPrime", (None,)), ("xengUpchanSumBeamsPrime", (4100,)), ("xengUpchanSumBeamsSetPfb", (0, hp)),
                       ("xengUpchanSumBeamsSetPfb", (9, hp)), ("xengUpchanSumBeamsSetPfb", (2, None)), ("xengUpchanSumBeamsGetInfo", (None, None, None)),
                       ("xengUpchanSumBeamsMark", (None,)), ("xengUpchanSumBeamsTicketDone", (1, None))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_upchan_beams_gpu.py covers the rest)
    i = ctypes.c_int()
    t = ctypes.c_ulonglong()
    for name, args in (("xengUpchanSumBeamsRun", (4096, 4096)), ("xengUpchanSumBeamsPrime", (4096,)), ("xengUpchanSumBeamsSetPfb", (4, hp)),
                       ("xengUpchanSumBeamsReset", ()), ("xengUpchanSumBeamsGetInfo", (ctypes.byref(i), ctypes.byref(i), ctypes.byref(i))),
                       ("xengUpchanSumBeamsMark", (ctypes.byref(t),)), ("xengUpchanSumBeamsWait", (1,)), ("xengUpchanSumBeamsSync", ())):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengUpchanSumBeamsDestroy")       # (nothing to destroy: success)
