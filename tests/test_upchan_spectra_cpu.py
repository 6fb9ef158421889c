"""UpchanSpectra without a GPU: the float64 restatement (tests/upchan_spectra_ref.py) against a frame-by-frame np.fft loop and
against the real diagonal of UpchanCorr's restatement; windows spanning gulps against one long window, PFB gulp sequences
against one long stream; the block on CPU rings (both implementations) with an oracle backend that keeps the context's state
(window position, accumulator, PFB history) -- windows within and across gulps, alignment to seq0, gaps (dropped windows,
realignment, a new output sequence, the PFB primed before the boundary), sequence restarts, two-part spans, header keys,
refusals -- the C entry points' argument checks, and the spectral-kurtosis helpers on seeded Gaussian noise."""
import ctypes

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanSpectra, incoherent_beam, sk_flags, sk_limits, spectral_kurtosis
from caltech_bifrost_dsp_amd.blocks.spectral_kurtosis import sk_variance
from caltech_bifrost_dsp_amd.ring import Ring
from oracle import xeng_oracle as orc
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq, _History, _u8
from tests.upchan_corr_ref import upchan_corr
from tests.upchan_spectra_ref import upchan_spectra, upchan_spectra_int

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


class SpectraBackend(OracleBackend):
    """The oracle backend plus xengUpchanSpectra* served by the float64 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.us, self.pfb, self.calls = None, _History(), []

    def upchan_spectra_initialize(self, gpu, ninput, nchan, ntime, nupchan, nframe_sum):
        self.us = dict(ninput=ninput, nchan=nchan, ntime=ntime, N=nupchan, W=nframe_sum, F=ntime // nupchan)
        self.gpw = max(1, nframe_sum // (ntime // nupchan))
        self.pos, self.acc, self.pfb = 0, None, _History()
        return 0

    def upchan_spectra_info(self):
        return self.gpw, max(1, self.us['F'] // self.us['W']), self.pos

    def upchan_spectra_set_pfb(self, ntap, coeffs):
        self.pfb.set(ntap, coeffs, self.us['N'])
        self.calls.append(('set_pfb', ntap))
        return 0

    def _gulp(self, v):
        u = self.us
        return v.reshape(u['ntime'], u['nchan'], u['ninput'])

    def _run(self, vin, out_arr, kind):
        u = self.us
        s, t0 = self.pfb.stream(vin, u['N'])
        r = upchan_spectra(s, u['N'], min(u['W'], u['F']), t0, u['ntime'], self.pfb.h)
        if self.gpw > 1:
            self.acc = r if self.pos == 0 else self.acc + r
            r = self.acc
        if self.pos == self.gpw - 1:
            out_arr.numpy().reshape(-1).view(np.uint8).view(np.float32)[...] = r.reshape(-1)
        else:
            assert out_arr is None
        self.pos = (self.pos + 1) % self.gpw
        self.pfb.refresh(vin, u['N'])
        self.calls.append(kind)
        return 0

    def upchan_spectra_run(self, in_arr, out_arr):
        return self._run(self._gulp(_u8(in_arr)), out_arr, 'run')

    def upchan_spectra_run_parts(self, part0, ntime0, part1, out_arr):
        assert ntime0 % self.us['N'] == 0 and ntime0 * self.us['nchan'] * self.us['ninput'] == part0.nbytes
        return self._run(self._gulp(np.concatenate([_u8(part0), _u8(part1)])), out_arr, 'parts')

    def upchan_spectra_prime(self, in_arr):
        self.pfb.refresh(self._gulp(_u8(in_arr)), self.us['N'])
        self.calls.append('prime')
        return 0

    def upchan_spectra_prime_parts(self, part0, ntime0, part1):
        self.pfb.refresh(self._gulp(np.concatenate([_u8(part0), _u8(part1)])), self.us['N'])
        self.calls.append('prime')
        return 0

    def upchan_spectra_reset(self):
        self.pos, self.acc, self.pfb.hist = 0, None, None
        self.calls.append('reset')

    def upchan_spectra_mark(self):
        return self.beam_mark()

    def upchan_spectra_wait(self, ticket):
        self.beam_wait(ticket)

    def upchan_spectra_sync(self):
        pass


def _volts(rng, ntime, nchan, ninput):
    return rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)


def _out(spans, shape):
    return [s.view(np.float32).reshape(shape) for s in spans]


def _close(got, exp):
    """fp32 storage of a float64 result: 1e-6 of each plane's largest value"""
    for pl in range(2):
        assert np.allclose(got[:, pl], exp[:, pl], rtol=1e-6, atol=1e-6 * np.abs(exp[:, pl]).max())


# ---------------------------------------------------------------- the restatement
def test_restatement_is_np_fft_per_frame():
    """Frame by frame: np.fft of each input's N decoded samples, fftshifted, |X|^2 and |X|^4 added per window."""
    nchan, ninput, N, W, nframe = 2, 5, 8, 3, 6
    vin = _volts(np.random.default_rng(1), N * nframe, nchan, ninput)
    got = upchan_spectra(vin, N, W, 0, N * nframe)
    re, im = orc.decode(vin)
    x = re.astype(np.float64) + 1j * im.astype(np.float64)
    exp = np.zeros((nframe // W, 2, nchan, N, ninput))
    for f in range(nframe):
        for c in range(nchan):
            for i in range(ninput):
                p = np.abs(np.fft.fftshift(np.fft.fft(x[f * N:(f + 1) * N, c, i]))) ** 2
                exp[f // W, 0, c, :, i] += p
                exp[f // W, 1, c, :, i] += p * p
    assert got.shape == exp.shape
    assert np.allclose(got, exp, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("N", [1, 2, 4, 16])
def test_s1_is_the_diagonal_of_the_correlator_restatement(N):
    """S1 over one window of all the frames equals the real diagonal of tests/upchan_corr_ref.py's visibilities of the same
    frames: two independent restatements agree to float64 rounding; for N <= 4 the int64 restatement agrees exactly."""
    nchan, ninput, nframe = 3, 6, 10
    vin = _volts(np.random.default_rng(2 + N), N * nframe, nchan, ninput)
    got = upchan_spectra(vin, N, nframe, 0, N * nframe)[0]
    V = upchan_corr(vin, N)                                     # [c*N + j][i][i']
    d = np.diagonal(V, axis1=1, axis2=2)
    assert np.abs(d.imag).max() <= 1e-9 * np.abs(d.real).max()
    assert np.allclose(got[0].reshape(nchan * N, ninput), d.real, rtol=1e-12, atol=1e-9)
    if N <= 4:
        exact = upchan_spectra_int(vin, N, nframe)[0]
        assert np.array_equal(np.rint(got), exact)


def test_windows_spanning_gulps_equal_one_long_window():
    """G = 3 gulps per window with a 4-tap PFB: the per-gulp sums (each gulp's frames with the history of the one before), added
    in order, equal the restatement of one window over the three gulps; and the gulps of a PFB stream taken one by one equal
    the windows of the long stream."""
    nchan, ninput, N, g, P = 2, 4, 16, 64, 4
    rng = np.random.default_rng(4)
    vin = _volts(rng, 3 * g, nchan, ninput)
    h = rng.standard_normal(P * N)
    parts = [upchan_spectra(vin, N, g // N, k * g, g, h) for k in range(3)]
    assert np.allclose(parts[0] + parts[1] + parts[2], upchan_spectra(vin, N, 3 * g // N, 0, 3 * g, h), rtol=1e-12, atol=1e-9)
    assert np.allclose(np.concatenate([upchan_spectra(vin, N, 2, k * g, g, h) for k in range(3)]), upchan_spectra(vin, N, 2, 0, 3 * g, h),
                       rtol=1e-12, atol=1e-9)


def test_backend_state_reset_is_a_fresh_context():
    """The oracle backend's context (which the block tests rest on): after a reset in mid-window it gives what a fresh context
    gives -- window position 0, no accumulator, zeros before the gulp."""
    from caltech_bifrost_dsp_amd.ndarray import XArray
    nchan, ninput, N, g, P = 1, 3, 8, 32, 3
    rng = np.random.default_rng(5)
    vin = _volts(rng, 3 * g, nchan, ninput)
    h = rng.standard_normal(P * N).astype(np.float32)

    def arr(a):
        x = XArray(shape=[a.size], dtype='u8', space='system')
        x.numpy().reshape(-1).view(np.uint8)[...] = a.reshape(-1)
        return x

    def window(be, gulps):
        out = XArray(shape=[2 * nchan * N * ninput * 4], dtype='u8', space='system')
        be.upchan_spectra_run(arr(vin[gulps[0] * g:(gulps[0] + 1) * g]), None)
        be.upchan_spectra_run(arr(vin[gulps[1] * g:(gulps[1] + 1) * g]), out)
        return out.numpy().reshape(-1).view(np.uint8).view(np.float32).copy()

    a, b = SpectraBackend(), SpectraBackend()
    for be in (a, b):
        be.upchan_spectra_initialize(0, ninput, nchan, g, N, 2 * g // N)
        be.upchan_spectra_set_pfb(P, h)
    a.upchan_spectra_run(arr(vin[:g]), None)
    assert a.upchan_spectra_info() == (2, 1, 1)
    a.upchan_spectra_reset()
    assert a.upchan_spectra_info() == (2, 1, 0)
    got = window(a, (1, 2))
    assert np.array_equal(got, window(b, (1, 2)))
    exp = upchan_spectra(vin, N, 2 * g // N, g, 2 * g, h, first=g)
    assert np.allclose(got, exp.reshape(-1), rtol=1e-6, atol=1e-6 * exp.max())


# ---------------------------------------------------------------- the block on CPU rings
@pytest.mark.parametrize("span", [False, True])
def test_block_windows_within_and_across_gulps_over_two_sequences(ring_impl, span):
    """Source -> UpchanSpectra -> Sink on in-repo rings, two sequences of 4 gulps.  W = F/2: one span per gulp holding two
    windows; W = 2F: one span per two gulps.  Each sequence starts from a reset (the second does not see the first's tail);
    every span equals the restatement; the header carries the keys of the issue."""
    nchan, nstand, N, g, P = 2, 3, 8, 64, 2
    ninput = 2 * nstand
    F = g // N
    W = 2 * F if span else F // 2
    rng = np.random.default_rng(5 + span)
    vs = [_volts(rng, 4 * g, nchan, ninput) for _ in range(2)]
    h = rng.standard_normal(P * N).astype(np.float32)
    hdrs = [source_header(nchan, nstand, 2, seq0=1000 * (s + 1), sfreq=1e6, complex=True) for s in range(2)]
    r0, r1 = Ring("gpu-input"), Ring("us-output")
    be = SpectraBackend()
    us = UpchanSpectra(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=W, backend=be, pfb_ntap=P, pfb_coeffs=h)
    shape = (max(F // W, 1), 2, nchan, N, ninput)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([us], Source(r0, [(hdrs[s], vs[s], g * nchan * ninput) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    per = 2 if span else 1
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hdrs[s]['seq0'] and hd['seq0'] == hdrs[s]['seq0']
        assert len(spans) == 4 // per
        for k, o in enumerate(_out(spans, shape)):
            _close(o, upchan_spectra(vs[s], N, W, k * per * g, per * g, h))
    hd = sink.sequences[0][0]
    assert hd['nupchan'] == N and hd['nframe_sum'] == W and hd['acc_len'] == W * N and hd['pfb_ntap'] == P
    assert hd['nbit'] == 32 and hd['nmoment'] == 2 and 'complex' not in hd
    assert hd['nstand'] == nstand and hd['npol'] == 2 and hd['nchan'] == nchan and hd['input_to_ant'] == hdrs[0]['input_to_ant']
    chan_bw = hdrs[0]['bw_hz'] / nchan
    assert hd['fine_bw_hz'] == chan_bw / N and hd['fine_sfreq'] == hdrs[0]['sfreq'] - chan_bw / 2
    assert be.calls == [('set_pfb', P)] + (['reset'] + ['run'] * 4) * 2
    assert us.stats['nwindow'] == (4 if span else 16) and us.stats['ndropped'] == 0


def test_block_two_part_spans_and_the_plain_fft(ring_impl):
    """The input ring hands every gulp out in two spans (the writer's spans are half gulps): RunParts with the split in whole
    frames, each output equal to the restatement; without PFB arguments no PFB call is made and the header has no pfb_ntap."""
    nchan, nstand, N, g = 2, 2, 8, 32
    ninput = 2 * nstand
    vin = _volts(np.random.default_rng(8), 3 * g, nchan, ninput)
    half = g // 2
    r0, r1 = Ring("gpu-input"), Ring("us-output")
    r0.resize(half, 8 * g * nchan * ninput)
    be = SpectraBackend()
    us = UpchanSpectra(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, backend=be)
    shape = (1, 2, nchan, N, ninput)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([us], Source(r0, [(source_header(nchan, nstand, 2, seq0=40), vin, half * nchan * ninput)]), [sink])
    assert be.calls == ['reset', 'parts', 'parts', 'parts']
    (hd, _, spans), = sink.sequences
    assert 'pfb_ntap' not in hd and hd['nframe_sum'] == g // N
    for k, o in enumerate(_out(spans, shape)):
        _close(o, upchan_spectra(vin, N, g // N, k * g, g))


R = 'run'


@pytest.mark.parametrize("split", [None, 16])
@pytest.mark.parametrize("missing,calls", [
    # G = 2 gulps per window, 10 gulps of the sequence, `missing` never read
    ((3,), ['reset', R, R, R, 'reset', R, R, R, R, R, R]),                          # (window 2-3 lost; gulp 4 is a boundary)
    ((4,), ['reset', R, R, R, R, 'reset', 'prime', R, R, R, R]),                    # (gulp 5 primes the window 6-7)
    ((0,), ['reset', 'reset', 'prime', R, R, R, R, R, R, R, R]),                    # (alignment to seq0: gulp 1 only primes)
    ((4, 5, 6), ['reset', R, R, R, R, 'reset', 'prime', R, R]),
])
def test_block_gap_mid_window_drops_realigns_and_primes(ring_impl, missing, calls, split):
    """Every gap resets the context (the window in progress and the PFB history go); the output restarts in a new sequence at
    the next window boundary (aligned to seq0, which is not a multiple of the window), primed with the gulp before it when that
    gulp was read.  Each written window equals the restatement of the samples seen without a break.  With split, every gulp
    comes in two parts."""
    nchan, nstand, N, g, P, ngulp, seq0 = 1, 2, 8, 32, 3, 10, 700
    ninput = 2 * nstand
    rng = np.random.default_rng(sum(missing) + 17)
    vin = _volts(rng, ngulp * g, nchan, ninput)
    h = rng.standard_normal(P * N).astype(np.float32)
    seen = [(k, vin[k * g:(k + 1) * g]) for k in range(ngulp) if k not in missing]
    be = SpectraBackend()
    r1 = Ring("us-output")
    us = UpchanSpectra(LOG, _FakeRing([_FakeSeq(source_header(nchan, nstand, 2, seq0=seq0), seen, g * nchan * ninput, split, nchan * ninput)]), r1,
                       nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=2 * g // N, backend=be, pfb_ntap=P, pfb_coeffs=h)
    shape = (1, 2, nchan, N, ninput)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    sink.start()
    us.main()
    sink.join(20)
    if split is not None:
        calls = ['parts' if c == R else c for c in calls]
    assert be.calls[0] == ('set_pfb', P) and be.calls[1:] == calls
    done = [k for k in range(0, ngulp, 2) if k not in missing and k + 1 not in missing]
    spans = [(hd, s) for hd, _, ss in sink.sequences for s in ss]
    assert len(spans) == len(done)
    last_gap = max(missing)
    before, after = [k for k in done if k < last_gap], [k for k in done if k > last_gap]
    assert [hd['seq0'] for hd, _, _ in sink.sequences] == [seq0 + ks[0] * g for ks in (before, after) if ks]
    for k, (hd, s) in zip(done, spans):
        first = 0 if k < last_gap else (last_gap + 1) * g
        _close(s.view(np.float32).reshape(shape), upchan_spectra(vin, N, 2 * g // N, k * g, 2 * g, h, first=first))
    assert us.stats['ndropped'] >= 1


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(nupchan=3), dict(nupchan=128), dict(ntime_gulp=60), dict(nframe_sum=3), dict(nframe_sum=12),
                                dict(nframe_sum=0), dict(ninput=0), dict(nchan=0), dict(pfb_ntap=9),
                                dict(pfb_ntap=2, pfb_coeffs=np.ones(8)), dict(pfb_ntap=8, nupchan=16, nframe_sum=2)])
def test_constructor_refuses_bad_arguments(kw):
    """nupchan outside the set, gulps that are not whole frames, windows that neither divide nor are whole gulps (8 frames per
    gulp), empty sizes, bad PFB taps or coefficients, a gulp (64 samples) shorter than the history (7 x 16)."""
    args = dict(nchan=1, ninput=4, ntime_gulp=64, nupchan=8, nframe_sum=4)
    args.update(kw)
    be = SpectraBackend()
    with pytest.raises(ValueError, match="UPCHAN_SPECTRA"):
        UpchanSpectra(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.us is None                    # (refused before the context is made)


@pytest.mark.parametrize("bad", [dict(nchan=2), dict(nstand=3), dict(npol=1)])
def test_block_refuses_a_header_of_another_size(bad):
    nchan, nstand, g = 1, 2, 64
    be = SpectraBackend()
    hdr = source_header(nchan, nstand, 2)
    hdr.update(bad)
    us = UpchanSpectra(LOG, _FakeRing([_FakeSeq(hdr, [(0, np.zeros((g, nchan, 2 * nstand), np.uint8))], g * nchan * 2 * nstand)]), Ring("b"),
                       nchan=nchan, ninput=2 * nstand, ntime_gulp=g, nupchan=8, backend=be)
    with pytest.raises(ValueError, match="UPCHAN_SPECTRA"):
        us.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengUpchanSpectraInitialize", "xengUpchanSpectraGetInfo", "xengUpchanSpectraRun", "xengUpchanSpectraRunParts", "xengUpchanSpectraSetPfb",
         "xengUpchanSpectraPrime", "xengUpchanSpectraPrimeParts", "xengUpchanSpectraReset", "xengUpchanSpectraMark", "xengUpchanSpectraWait",
         "xengUpchanSpectraTicketDone", "xengUpchanSpectraSync", "xengUpchanSpectraDestroy")


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, RunParts, Prime, PrimeParts, Reset, Mark and TicketDone are enqueue-only, the
    calls that wait are not.  Initialize refuses bad sizes before it touches a device; Run / Prime refuse null and misaligned
    pointers and empty first parts, SetPfb bad taps, GetInfo null results, before looking for a context; without one,
    INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengUpchanSpectraRun", "xengUpchanSpectraRunParts", "xengUpchanSpectraPrime", "xengUpchanSpectraPrimeParts", "xengUpchanSpectraReset",
                 "xengUpchanSpectraMark", "xengUpchanSpectraTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengUpchanSpectraInitialize", "xengUpchanSpectraSetPfb", "xengUpchanSpectraWait", "xengUpchanSpectraSync"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, ninput, nchan, ntime, nupchan, nframe_sum): 30 frames of 32 per gulp
    for args in ((0, 0, 96, 960, 32, 30), (0, 704, 0, 960, 32, 30), (0, 704, 96, 0, 32, 30), (0, 704, 96, 960, 3, 30), (0, 704, 96, 960, 128, 30),
                 (0, 704, 96, 1000, 32, 25), (0, 704, 96, 960, 32, 20), (0, 704, 96, 960, 32, 45), (0, 704, 96, 960, 32, 0),
                 (0, 704, 96, 960, 32, -30), (0, 1 << 20, 96, 960, 32, 30)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanSpectraInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    h = np.ones(64 * 8, np.float32)
    hp = h.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name, args in (("xengUpchanSpectraRun", (None, 4096)), ("xengUpchanSpectraRun", (4096, 4100)),
                       ("xengUpchanSpectraRunParts", (None, 32, 4096, 4096)), ("xengUpchanSpectraRunParts", (4096, 32, None, 4096)),
                       ("xengUpchanSpectraRunParts", (4096, 0, 8192, 4096)), ("xengUpchanSpectraRunParts", (4096, 32, 8192, 4100)),
                       ("xengUpchanSpectraPrime", (None,)), ("xengUpchanSpectraPrimeParts", (4096, 32, None)),
                       ("xengUpchanSpectraPrimeParts", (4096, -32, 8192)), ("xengUpchanSpectraSetPfb", (0, hp)),
                       ("xengUpchanSpectraSetPfb", (9, hp)), ("xengUpchanSpectraSetPfb", (2, None)), ("xengUpchanSpectraGetInfo", (None, None, None)),
                       ("xengUpchanSpectraMark", (None,)), ("xengUpchanSpectraTicketDone", (1, None))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_upchan_spectra_gpu.py covers the rest)
    i = ctypes.c_int()
    t = ctypes.c_ulonglong()
    for name, args in (("xengUpchanSpectraRun", (4096, 4096)), ("xengUpchanSpectraRunParts", (4096, 32, 8192, 4096)), ("xengUpchanSpectraPrime", (4096,)),
                       ("xengUpchanSpectraPrimeParts", (4096, 32, 8192)), ("xengUpchanSpectraSetPfb", (4, hp)), ("xengUpchanSpectraReset", ()),
                       ("xengUpchanSpectraGetInfo", (ctypes.byref(i), ctypes.byref(i), ctypes.byref(i))),
                       ("xengUpchanSpectraMark", (ctypes.byref(t),)), ("xengUpchanSpectraWait", (1,)),
                       ("xengUpchanSpectraTicketDone", (1, ctypes.byref(i))), ("xengUpchanSpectraSync", ())):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengUpchanSpectraDestroy")        # (nothing to destroy: success)


# ---------------------------------------------------------------- the helpers
def _noise_moments(rng, m, ncell, chunk=20000):
    """S1, S2 of ncell cells of unit complex Gaussian noise over m frames, float64, no quantisation."""
    s1, s2 = np.empty(ncell), np.empty(ncell)
    for a in range(0, ncell, chunk):
        n = min(chunk, ncell - a)
        p = rng.standard_normal((m, n)) ** 2 + rng.standard_normal((m, n)) ** 2
        s1[a:a + n] = p.sum(axis=0)
        s2[a:a + n] = (p * p).sum(axis=0)
    return s1, s2


@pytest.mark.parametrize("m,ncell,max_flagged", [(30, 400000, 0.02), (750, 100000, 0.01)])
def test_sk_statistics_on_gaussian_noise(m, ncell, max_flagged):
    """Seeded complex Gaussian noise without quantisation: the mean of SK within 5 standard errors of 1, its variance within
    5 % of 4 M^2 / ((M-1)(M+2)(M+3)), clean cells flagged at nsigma = 3 at most 2 % (M = 30) / 1 % (M = 750).  A 10 %-duty burst
    in one cell is flagged at both M.  A steady tone in another is flagged at M = 750; at M = 30 it cannot be by these limits:
    SK >= 0 for any data (M S2 >= S1^2) and the lower 3-sigma limit is 1 - 3 * 0.343 < 0 there, which the test states."""
    rng = np.random.default_rng(1000 + m)
    s1, s2 = _noise_moments(rng, m, ncell)
    sk = spectral_kurtosis(s1, s2, m)
    var = sk_variance(m)
    assert var == pytest.approx(4.0 * m * m / ((m - 1) * (m + 2) * (m + 3)), rel=1e-14)
    print("M = %d: mean SK %.5f, variance %.4f of the formula" % (m, sk.mean(), sk.var() / var))
    assert abs(sk.mean() - 1.0) <= 5 * np.sqrt(var / ncell)
    assert abs(sk.var() / var - 1.0) <= 0.05
    lo, hi = sk_limits(m)
    assert (lo, hi) == pytest.approx((1 - 3 * np.sqrt(var), 1 + 3 * np.sqrt(var)), rel=1e-14)
    flags = sk_flags(s1, s2, m)
    assert np.array_equal(flags, (sk < lo) | (sk > hi))
    print("M = %d: %.3f %% of clean cells flagged" % (m, 100 * flags.mean()))
    assert flags.mean() <= max_flagged
    # a tone of 10 x the noise amplitude in one cell, a burst of the same amplitude in 10 % of the frames of another
    z = (rng.standard_normal((m, 2)) + 1j * rng.standard_normal((m, 2)))
    z[:, 0] += 10 * np.sqrt(2) * np.exp(2j * np.pi * 0.123 * np.arange(m))
    z[::10, 1] += 10 * np.sqrt(2) * np.exp(2j * np.pi * rng.random(len(z[::10])))
    p = np.abs(z) ** 2
    t1, t2 = p.sum(axis=0), (p * p).sum(axis=0)
    tsk = spectral_kurtosis(t1, t2, m)
    tf = sk_flags(t1, t2, m)
    assert tsk[1] > hi and tf[1]
    assert 0 <= tsk[0] < 0.1
    if lo > 0:
        assert tf[0]
    else:
        assert m == 30 and not tf[0]        # (no SK is below a negative limit)


def test_sk_helpers_shapes_nan_and_incoherent_beam():
    """Cells with S1 = 0 give NaN and are flagged; the helpers keep the shape of S1; the incoherent beam sums S1 over stands per
    pol, leaves flagged cells out and counts what went in."""
    rng = np.random.default_rng(3)
    nchan, N, nstand, m = 2, 4, 5, 40
    s1, s2 = _noise_moments(rng, m, nchan * N * nstand * 2)
    s1, s2 = s1.reshape(nchan, N, nstand * 2), s2.reshape(nchan, N, nstand * 2)
    s1[1, 2, 3] = s2[1, 2, 3] = 0.0
    sk = spectral_kurtosis(s1.astype(np.float32), s2.astype(np.float32), m)
    assert sk.shape == s1.shape and sk.dtype == np.float64 and np.isnan(sk[1, 2, 3]) and np.isnan(sk).sum() == 1
    flags = sk_flags(s1, s2, m)
    assert flags.shape == s1.shape and flags.dtype == bool and flags[1, 2, 3]
    beam, count = incoherent_beam(s1)
    assert beam.shape == count.shape == (nchan, N, 2)
    assert np.allclose(beam, s1.reshape(nchan, N, nstand, 2).sum(axis=2)) and (count == nstand).all()
    f = np.zeros(s1.shape, bool)
    f[0, 1, 4] = f[0, 1, 6] = f[1, 0, 1] = True         # stands 2 and 3 of pol 0, stand 0 of pol 1
    beam2, count2 = incoherent_beam(s1, npol=2, flags=f)
    assert beam2[0, 1, 0] == pytest.approx(beam[0, 1, 0] - s1[0, 1, 4] - s1[0, 1, 6]) and count2[0, 1, 0] == nstand - 2
    assert beam2[1, 0, 1] == pytest.approx(beam[1, 0, 1] - s1[1, 0, 1]) and count2[1, 0, 1] == nstand - 1
    assert count2.sum() == count.sum() - 3
    with pytest.raises(ValueError):
        incoherent_beam(s1[..., :5], npol=2)
    with pytest.raises(ValueError):
        spectral_kurtosis(s1, s2, 1)
    with pytest.raises(ValueError):
        sk_limits(1)
