"""xengUpchanSpectra* and UpchanSpectra on the MI355X: S1 and S2 against the float64 restatement (tests/upchan_spectra_ref.py)
within 1e-5 of each plane's RMS and, at every small shape, each cell within 1e-5 (S1) and 2e-5 (S2) of its own value, for
N = 8..64 and P = 1..8, windows within and across gulps, small sizes and the live size;
the int64 restatement at N = 1, 2, 4 word for word; S1 against the diagonal of xengUpchanCorr*; the spectral-kurtosis flags of
the device's sums against the restatement's; bit identity (repeats, two-part gulps, Reset, Prime, beside the X-engine and the
beamformer); the argument checks that need a context; and the block on device rings.  No wall-clock assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import UpchanSpectra, sk_flags, sk_limits, spectral_kurtosis  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_upchan_pfb_gpu import _DevRing, _DevSeq  # noqa: E402
from tests.upchan_spectra_local_ref import cell_ratios, check_cells  # noqa: E402
from tests.upchan_spectra_ref import upchan_spectra, upchan_spectra_int  # noqa: E402

POISON = 0xA5
GUARD = 4096
INVALID_ARGUMENT = 1


def _fp(h):
    return h.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ffi.call("xengUpchanSpectraGetInfo", ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


class US:
    """One xengUpchanSpectra context, the gulps of a test in one device buffer, and one poisoned output span per completed
    window (or group of F / W windows) with a guard after the last."""

    def __init__(self, ninput, nchan, ntime, nupchan, nframe_sum, ngulp=1, ntap=1, h=None):
        self.ninput, self.nchan, self.ntime, self.N, self.W = ninput, nchan, ntime, nupchan, nframe_sum
        ffi.call("xengUpchanSpectraInitialize", 0, ninput, nchan, ntime, nupchan, nframe_sum)
        if h is not None:
            ffi.call("xengUpchanSpectraSetPfb", ntap, _fp(h))
        self.gpw, self.wpg, _ = _info()
        self.shape = (self.wpg, 2, nchan, nupchan, ninput)
        self.span = int(np.prod(self.shape)) * 4
        self.gulp = ntime * nchan * ninput
        self.ngulp = ngulp
        self.din = ffi.DeviceBuffer(ngulp * self.gulp)
        self.nspan = max(1, ngulp // self.gpw)
        self.dout = ffi.DeviceBuffer(self.nspan * self.span + GUARD)

    def run(self, vin=None, gulps=None, split=None, prime=(), download=True):
        """Gulps `gulps` of the buffer (all of them by default; vin uploaded first when given) in order, each whole or split
        after `split` samples; a gulp listed in `prime` only primes the history.  Returns the output spans, f32 each of
        self.shape, after checking that nothing was written past the last."""
        if vin is not None:
            self.din.upload(np.ascontiguousarray(vin).reshape(-1))
        gulps = range(self.ngulp) if gulps is None else gulps
        ffi.call("xengMemset", self.dout.ptr, POISON, self.nspan * self.span + GUARD)
        row = self.nchan * self.ninput
        nout = 0
        for k in gulps:
            p = self.din.ptr + k * self.gulp
            if k in prime:
                if split is None:
                    ffi.call("xengUpchanSpectraPrime", p)
                else:
                    ffi.call("xengUpchanSpectraPrimeParts", p, split, p + split * row)
                continue
            last = _info()[2] == self.gpw - 1
            out = self.dout.ptr + nout * self.span if last else None
            if split is None:
                ffi.call("xengUpchanSpectraRun", p, out)
            else:
                ffi.call("xengUpchanSpectraRunParts", p, split, p + split * row, out)
            nout += last
        ffi.call("xengUpchanSpectraSync")
        guard = self.dout.download(np.uint8, GUARD + (self.nspan - nout) * self.span, nout * self.span)
        assert (guard == POISON).all(), "bytes past the output were written"
        if not download:
            return nout
        return [self.dout.download(np.float32, self.span // 4, s * self.span).reshape(self.shape) for s in range(nout)]

    def close(self):
        ffi.call("xengUpchanSpectraDestroy")


@pytest.fixture
def us():
    yield US
    ffi.call("xengUpchanSpectraDestroy")


def check(got, exp, what="", cells=True):
    """S1 within 1e-5 of the RMS of the S1 plane, S2 within 1e-5 of the RMS of the S2 plane (the bar of UpchanBeamform's power);
    and (cells) every S1 within 1e-5 and every S2 within 2e-5 of its own value (check_cells).  At the live size
    the worst cell is printed, not asserted."""
    cell = cell_ratios(got, exp)
    got = np.asarray(got, np.float64)
    worst = []
    for pl in range(2):
        rms = np.sqrt(np.mean(exp[:, pl] ** 2))
        worst.append(np.abs(got[:, pl] - exp[:, pl]).max() / rms)
    print("%s max |err| / plane RMS: S1 %.3g, S2 %.3g; max |err| / own cell: S1 %.3g, S2 %.3g"
          % (what, worst[0], worst[1], cell[:, 0].max(), cell[:, 1].max()))
    assert worst[0] <= 1e-5 and worst[1] <= 1e-5, worst
    if cells:
        check_cells(got, exp)


# ---------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("N,P,F,W,ngulp", [
    (8, 1, 12, 4, 3), (8, 4, 12, 36, 3), (8, 8, 12, 12, 3), (16, 2, 10, 5, 3), (16, 8, 10, 20, 4), (16, 1, 750, 750, 1),
    (32, 4, 30, 30, 3), (32, 1, 30, 90, 3), (32, 8, 30, 15, 3), (32, 2, 30, 60, 4), (64, 2, 6, 3, 3), (64, 1, 6, 12, 4), (64, 4, 6, 6, 3),
    (64, 8, 9, 27, 3)])
def test_against_the_float64_restatement(us, N, P, F, W, ngulp):
    """70 inputs (not a multiple of the 64 of a work-group) x 3 channels, every byte value, random asymmetric h: every window of
    the consecutive gulps within the bar; nothing past the output written."""
    ninput, nchan = 70, 3
    if F >= 750:
        ninput, nchan = 20, 1
    ntime = F * N
    rng = np.random.default_rng(1000 * N + 10 * P + W)
    vin = rng.integers(0, 256, (ngulp * ntime, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32) if P > 1 else None
    u = us(ninput, nchan, ntime, N, W, ngulp=ngulp, ntap=P, h=h)
    outs = u.run(vin)
    per = max(1, W // F)
    assert len(outs) == ngulp // per
    for k, o in enumerate(outs):
        exp = upchan_spectra(vin, N, W, k * per * ntime, per * ntime, h)
        check(o, exp, "N %d P %d W %d span %d:" % (N, P, W, k))


@pytest.mark.parametrize("P,W,ngulp", [(4, 30, 3), (1, 750, 25)])
def test_live_size(us, P, W, ngulp):
    """704 inputs x 96 channels x 960 samples, N = 32: W = 30 (one window per gulp, three consecutive gulps, a 4-tap PFB) and
    W = 750 (one window over 25 gulps).  The restatement of the whole output is minutes of float64 FFTs on the host, so a
    sample of coarse channels (first, last, two inside) is compared, every input and fine channel of them, each plane's RMS
    taken over the sample."""
    ninput, nchan, ntime, N = 704, 96, 960, 32
    rng = np.random.default_rng(W + P)
    vin = rng.integers(0, 256, (ngulp * ntime, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32) if P > 1 else None
    u = us(ninput, nchan, ntime, N, W, ngulp=ngulp, ntap=P, h=h)
    outs = u.run(vin)
    per = max(1, W // 30)
    assert len(outs) == ngulp // per
    chans = [0, 37, 64, 95]
    for k, o in enumerate(outs):
        exp = upchan_spectra(vin, N, W, k * per * ntime, per * ntime, h, chans=chans)
        check(o[:, :, chans], exp, "live size P %d W %d span %d:" % (P, W, k), cells=False)


@pytest.mark.parametrize("N", [1, 2, 4])
def test_small_n_equals_the_int64_restatement(us, N):
    """|re|, |im| <= 2 and windows of at most 1024 frames: |X|^2 <= 128, S2 <= 1024 * 16384 = 2^24, every fp32 operation exact.
    A window of 64 frames within the gulp and a window of 1024 frames over 4 gulps, 130 inputs: word for word."""
    ninput, nchan, F = 130, 2, 256
    ntime = F * N
    rng = np.random.default_rng(N)
    re, im = rng.integers(-2, 3, (4 * ntime, nchan, ninput)), rng.integers(-2, 3, (4 * ntime, nchan, ninput))
    vin = (((re & 0xF) << 4) | (im & 0xF)).astype(np.uint8)
    for W in (64, 1024):
        u = us(ninput, nchan, ntime, N, W, ngulp=4)
        got = np.concatenate(u.run(vin))
        exp = upchan_spectra_int(vin, N, W)
        assert exp.max() <= 2 ** 24
        assert got.shape == exp.shape and np.array_equal(got, exp.astype(np.float32)), (N, W)


# ---------------------------------------------------------------- the same frames through the correlator
@pytest.mark.parametrize("P", [1, 4])
def test_s1_equals_the_diagonal_of_upchan_corr(us, P):
    """Three gulps through xengUpchanCorr* over one integration and through xengUpchanSpectra* with W = the integration: S1
    equals the real part of the diagonal within the sum of the two bars (1e-6 of the diagonal element, the correlator's, plus
    1e-5 of the S1 plane's RMS), with and without the same PFB."""
    ninput, nchan, N, F, ngulp = 48, 2, 16, 10, 3
    ntime = F * N
    rng = np.random.default_rng(40 + P)
    vin = rng.integers(0, 256, (ngulp * ntime, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32) if P > 1 else None
    u = us(ninput, nchan, ntime, N, ngulp * F, ngulp=ngulp, ntap=P, h=h)
    s, = u.run(vin)
    ffi.call("xengUpchanCorrInitialize", 0, ninput, nchan, ntime, N, 0, nchan * N, 0)
    try:
        if h is not None:
            ffi.call("xengUpchanCorrSetPfb", P, _fp(h))
        dv = ffi.DeviceBuffer(nchan * N * ninput * ninput * 8)
        for k in range(ngulp):
            ffi.call("xengUpchanCorrAccumulate", u.din.ptr + k * u.gulp)
        ffi.call("xengUpchanCorrDump", dv.ptr)
        ffi.call("xengUpchanCorrSync")
        v = dv.download(np.complex64).reshape(nchan * N, ninput, ninput)
    finally:
        ffi.call("xengUpchanCorrDestroy")
    d = np.diagonal(v, axis1=1, axis2=2).real.astype(np.float64)          # [c*N + j][i]
    s1 = s[0, 0].reshape(nchan * N, ninput).astype(np.float64)
    rms = np.sqrt(np.mean(s1 ** 2))
    err = np.abs(s1 - d)
    print("P %d: max |S1 - diag| / (1e-6 diag + 1e-5 rms) = %.3g" % (P, (err / (1e-6 * d + 1e-5 * rms)).max()))
    assert (err <= 1e-6 * d + 1e-5 * rms).all()


# ---------------------------------------------------------------- the flags
def test_sk_flags_of_the_device_sums_equal_the_restatements(us):
    """Seeded 4-bit Gaussian data (sigma 2.5, clipped to -7..7), N = 32, M = 30, 64 x 16 x 32 = 32768 cells: sk_flags of the
    device's S1, S2 equals sk_flags of the restatement's in every cell whose float64 SK is farther than 1e-4 (relative) from
    both limits; the cells that rule leaves out are at most 1 % of all (expected: about 1e-5 of them)."""
    ninput, nchan, N, M = 64, 16, 32, 30
    ntime = M * N
    rng = np.random.default_rng(77)
    q = np.clip(np.rint(rng.normal(0, 2.5, (2, ntime, nchan, ninput))), -7, 7).astype(np.int64)
    vin = (((q[0] & 0xF) << 4) | (q[1] & 0xF)).astype(np.uint8)
    u = us(ninput, nchan, ntime, N, M)
    o, = u.run(vin)
    exp = upchan_spectra(vin, N, M, 0, ntime)
    check(o, exp, "4-bit noise:")
    sk = spectral_kurtosis(exp[0, 0], exp[0, 1], M)
    lo, hi = sk_limits(M)
    near = (np.abs(sk - lo) <= 1e-4 * abs(lo)) | (np.abs(sk - hi) <= 1e-4 * abs(hi))
    fd, fr = sk_flags(o[0, 0], o[0, 1], M), sk_flags(exp[0, 0], exp[0, 1], M)
    print("SK mean %.4f, flagged %.3f %%, cells near a limit %d of %d, flags differing away from the limits %d"
          % (sk.mean(), 100 * fr.mean(), near.sum(), near.size, (fd != fr)[~near].sum()))
    assert near.mean() <= 0.01
    assert np.array_equal(fd[~near], fr[~near])
    assert 0 < fr.mean() < 0.03


# ---------------------------------------------------------------- bit identity
def test_repeats_parts_reset_and_prime_are_bit_identical(us):
    """A 3-tap PFB, W = 2 gulps, 4 gulps, 70 inputs: the same bits run to run, with every gulp in two parts at several split
    points, after a Reset in mid-window versus a fresh context, and with the gulp before a window primed instead of run."""
    ninput, nchan, N, F, P, ngulp = 70, 3, 16, 9, 3, 4
    ntime = F * N
    rng = np.random.default_rng(8)
    vin = rng.integers(0, 256, (ngulp * ntime, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32)
    u = us(ninput, nchan, ntime, N, 2 * F, ngulp=ngulp, ntap=P, h=h)
    ref = u.run(vin)
    assert len(ref) == 2
    for k, o in enumerate(ref):
        check(o, upchan_spectra(vin, N, 2 * F, 2 * k * ntime, 2 * ntime, h), "window %d:" % k)

    def same(a, b):
        return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    ffi.call("xengUpchanSpectraReset")
    assert same(u.run(), ref)                                   # run to run
    for split in (N, 4 * N, 8 * N):                             # two-part gulps
        ffi.call("xengUpchanSpectraReset")
        assert same(u.run(split=split), ref), split
    # Reset in mid-window: gulps 2, 3 then give what a fresh context gives for them
    ffi.call("xengUpchanSpectraReset")
    ffi.call("xengUpchanSpectraRun", u.din.ptr, None)
    assert _info() == (2, 1, 1)
    ffi.call("xengUpchanSpectraReset")
    assert _info() == (2, 1, 0)
    after_reset = u.run(gulps=(2, 3))
    u2 = us(ninput, nchan, ntime, N, 2 * F, ngulp=ngulp, ntap=P, h=h)
    fresh = u2.run(vin, gulps=(2, 3))
    assert same(after_reset, fresh) and not same(fresh, ref[1:])  # (zeros before gulp 2, not gulp 1's tail)
    # Prime with gulp 1, then gulps 2, 3: the window the full run gave
    ffi.call("xengUpchanSpectraReset")
    assert same(u2.run(gulps=(1, 2, 3), prime=(1,)), ref[1:])
    ffi.call("xengUpchanSpectraReset")
    assert same(u2.run(gulps=(1, 2, 3), prime=(1,), split=5 * N), ref[1:])
    # parts that are not whole frames are refused, nothing launched
    for bad in (4 * N + 1, ntime, 0):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanSpectraRunParts", u2.din.ptr, bad, u2.din.ptr + 4 * N * nchan * ninput, u2.dout.ptr)
        assert ei.value.status == INVALID_ARGUMENT


def test_beside_xengine_and_beamformer_is_bit_identical(us):
    """Once (not a loop): the kernel while the X-engine's MFMA contraction and xengBeamformRun run on their streams gives the
    bits it gives alone, at 704 inputs, N = 32, a 4-tap PFB."""
    ninput, nchan, ntime, N, P = 704, 8, 960, 32, 4
    rng = np.random.default_rng(9)
    vin = rng.integers(0, 256, (3 * ntime, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32)
    u = us(ninput, nchan, ntime, N, 30, ngulp=3, ntap=P, h=h)
    alone = u.run(vin)
    nbeam = 16
    w = (rng.uniform(-1, 1, (nchan, nbeam, ninput)) + 1j * rng.uniform(-1, 1, (nchan, nbeam, ninput))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, ninput, nchan, ntime, nbeam, 0)
    dw = ffi.DeviceBuffer(w.nbytes).upload(w)
    db = ffi.DeviceBuffer(nchan * nbeam * ntime * 8)
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    x = Xgpu(352, 96, 480, max_gulps=4)
    try:
        x.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        ffi.call("xengUpchanSpectraReset")
        for k in range(4):
            ffi.call("xengXgpuKernelAsync", x.inbuf.ptr + k * x.gulp_bytes, x.out.ptr, int(k == 3))
        for k in range(3):
            ffi.call("xengBeamformRun", u.din.ptr + k * u.gulp, db.ptr, dw.ptr)
        beside = u.run()
        ffi.call("xengXgpuSync")
        ffi.call("xengBeamformSync")
    finally:
        x.close()
        ffi.call("xengBeamformDestroy")
    assert len(beside) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(alone, beside))


# ---------------------------------------------------------------- what needs a context
def test_argument_checks_with_a_context(us):
    """A NULL output on a gulp that completes a window, misaligned outputs, SetPfb with a gulp shorter than the history:
    INVALID_ARGUMENT, nothing launched; GetInfo reports the window shape."""
    u = us(8, 2, 64, 16, 8)                 # F = 4, W = 8: two gulps per window
    assert _info() == (2, 1, 0)
    for args in ((u.din.ptr, u.dout.ptr + 4), (None, u.dout.ptr)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanSpectraRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengUpchanSpectraRun", u.din.ptr, None)
    assert _info() == (2, 1, 1)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanSpectraRun", u.din.ptr, None)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (2, 1, 1)
    hh = np.ones(6 * 16, np.float32)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanSpectraSetPfb", 6, _fp(hh))          # (5 x 16 samples of history > 64)
    assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengUpchanSpectraReset")
    assert _info() == (2, 1, 0)
    ffi.call("xengUpchanSpectraInitialize", 0, 8, 2, 64, 16, 2)
    assert _info() == (1, 2, 0)
    ffi.call("xengUpchanSpectraSync")


# ---------------------------------------------------------------- the block on device rings
def test_block_on_device_rings_streaming(us):
    """Source -> UpchanSpectra -> Sink on device rings (gulps in flight on tickets), two sequences of 6 gulps, W = 2 gulps, a
    4-tap PFB with the default coefficients: every window equals the restatement."""
    from caltech_bifrost_dsp_amd.blocks.pfb import pfb_coeffs
    nchan, nstand, N, g, P = 3, 40, 16, 96, 4
    ninput = 2 * nstand
    W = 2 * g // N
    rng = np.random.default_rng(21)
    vs = [rng.integers(0, 256, (6 * g, nchan, ninput), dtype=np.uint8) for _ in range(2)]
    hdrs = [source_header(nchan, nstand, 2, seq0=5000 * (s + 1), sfreq=40e6) for s in range(2)]
    r0, r1 = Ring("gpu-input", space="cuda"), Ring("us-output", space="cuda")
    blk = UpchanSpectra(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=W, pfb_ntap=P, gpu=0)
    shape = (1, 2, nchan, N, ninput)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([blk], Source(r0, [(hdrs[s], vs[s], g * nchan * ninput) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    for s, (hd, _, spans) in enumerate(sink.sequences):
        assert hd['seq0'] == hdrs[s]['seq0'] and hd['nmoment'] == 2 and hd['pfb_ntap'] == P and len(spans) == 3
        for k, o in enumerate(spans):
            check(o.view(np.float32).reshape(shape), upchan_spectra(vs[s], N, W, 2 * k * g, 2 * g, pfb_coeffs(P, N)), "seq %d window %d:" % (s, k))


def test_block_on_device_rings_with_a_gap(us):
    """Sequence 1 misses gulp 4 of 8 (two-part gulps), sequence 2 starts fresh; W = 2 gulps, a 4-tap PFB: windows [0,1], [2,3];
    gulp 4 missing loses [4,5]; gulp 5 waits for the boundary and primes; [6,7] sees its tail, in a new output sequence."""
    from caltech_bifrost_dsp_amd.blocks.pfb import pfb_coeffs
    nchan, nstand, N, P, g = 2, 4, 16, 4, 64
    ninput = 2 * nstand
    rng = np.random.default_rng(9)
    s1 = rng.integers(0, 256, (8 * g, nchan, ninput), dtype=np.uint8)
    s2 = rng.integers(0, 256, (2 * g, nchan, ninput), dtype=np.uint8)
    h1, h2 = source_header(nchan, nstand, 2, seq0=0, sfreq=40e6), source_header(nchan, nstand, 2, seq0=20000, sfreq=40e6)
    seen1 = [(k, s1[k * g:(k + 1) * g]) for k in range(8) if k != 4]
    seen2 = [(k, s2[k * g:(k + 1) * g]) for k in range(2)]
    igulp = g * nchan * ninput
    h = pfb_coeffs(P, N)
    ro = Ring("us-output", space="cuda")
    blk = UpchanSpectra(LOG, _DevRing([_DevSeq(h1, seen1, igulp, 48 * nchan * ninput), _DevSeq(h2, seen2, igulp)]), ro, nchan=nchan, ninput=ninput,
                        ntime_gulp=g, nupchan=N, nframe_sum=2 * g // N, pfb_ntap=P, gpu=0)
    shape = (1, 2, nchan, N, ninput)
    sink = Sink(ro, int(np.prod(shape)) * 4)
    sink.start()
    try:
        blk.main()
    finally:
        sink.join(30)
    spans = [(hd['seq0'], s) for hd, _, ss in sink.sequences for s in ss]
    expect = [(s1, 0, 0), (s1, 2, 0), (s1, 6, 5 * g), (s2, 0, 0)]
    assert [sq for sq, _ in spans] == [0, 0, 6 * g, 20000]
    for (stream, k, first), (_, s) in zip(expect, spans):
        check(s.view(np.float32).reshape(shape), upchan_spectra(stream, N, 2 * g // N, k * g, 2 * g, h, first=first), "gulps %d-%d:" % (k, k + 1))
    assert blk.stats['ndropped'] == 1 and blk.stats['nwindow'] == 4
