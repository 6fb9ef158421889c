"""UpchanSumBeams on the MI355X: xengUpchanSumBeams* against the float64 restatement (tests/upchan_beams_ref.py; the whole
output and every row of it) for every nupchan, PFB taps 1..8 with random asymmetric coefficients, windows within a gulp and
spanning gulps, pair subsets, and at the live size; bytes past the output untouched; bit identity from run to run and beside
an X-engine contraction; the sign of Im(XY*); the cross-path equality with UpchanBeamform's dual-pol mode on the same 4-bit
input; and the block on device rings beside BeamformSumBeams.  No wall-clock assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Beamform, BeamformSumBeams, UpchanSumBeams  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_blocks_cpu import _beam_cmds  # noqa: E402
from tests.upchan_beams_ref import beam_channelise, sum_beams, upchan_sum_beams  # noqa: E402
from tests.upchan_local_ref import check_rows, row_ratios  # noqa: E402
from tests.upchan_pfb_ref import upchan_beamform_pfb  # noqa: E402

POISON = 0xA5
GUARD = 4096
INVALID_ARGUMENT = 1


def _fp(h):
    return None if h is None else h.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def check(got, exp, bar=1e-5, rows=True):
    """Within `bar` of the output's RMS, and every row within `bar` of its own scale (tests/upchan_local_ref.py check_rows);
    rows=False (the live size): the worst row's figure is printed, not asserted."""
    rms = np.sqrt(np.mean(np.abs(exp) ** 2))
    err = np.max(np.abs(got.astype(np.float64) - exp))
    assert rms > 0 and err <= bar * rms, "max |err| %.3g = %.3g of RMS %.3g" % (err, err / rms, rms)
    if rows:
        check_rows(got, exp, bar)
    else:
        print("live size %s: max |err| = %.3g of the RMS, worst row %.3g of its own" % (got.shape, err / rms, np.max(row_ratios(got, exp))))


def _info():
    g, w, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ffi.call("xengUpchanSumBeamsGetInfo", ctypes.byref(g), ctypes.byref(w), ctypes.byref(p))
    return g.value, w.value, p.value


class UB:
    """The xengUpchanSumBeams context (one per process), a gulp buffer and a poisoned output with a guard after it."""

    def __init__(self, nchan, nbeam, ntime, N, W, pair0=0, npair=None, ntap=None, h=None):
        self.nchan, self.nbeam, self.ntime, self.N, self.W = nchan, nbeam, ntime, N, W
        self.pair0, self.npair = pair0, (nbeam // 2 - pair0 if npair is None else npair)
        ffi.call("xengUpchanSumBeamsInitialize", 0, nchan, nbeam, ntime, N, self.pair0, self.npair, W)
        self.h = None if h is None else np.ascontiguousarray(h, np.float32)
        if ntap is not None:
            ffi.call("xengUpchanSumBeamsSetPfb", ntap, _fp(self.h))
        F = ntime // N
        self.shape = (max(F // W, 1), self.npair, nchan, N, 4)
        self.nout = int(np.prod(self.shape)) * 4
        self.din = ffi.DeviceBuffer(nchan * nbeam * ntime * 8)
        self.dout = ffi.DeviceBuffer(self.nout + GUARD)
        self.poison()

    def poison(self):
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def run(self, gulp, out=True):
        self.din.upload(np.ascontiguousarray(gulp, np.complex64))
        ffi.call("xengUpchanSumBeamsRun", self.din.ptr, self.dout.ptr if out else None)
        ffi.call("xengUpchanSumBeamsSync")

    def result(self):
        raw = self.dout.download(np.uint8)
        assert (raw[self.nout:] == POISON).all(), "bytes past the output were written"
        return raw[:self.nout].view(np.float32).reshape(self.shape)

    def untouched(self):
        return (self.dout.download(np.uint8) == POISON).all()


def _beams(rng, nchan, nbeam, ntime):
    return (rng.standard_normal((nchan, nbeam, ntime)) + 1j * rng.standard_normal((nchan, nbeam, ntime))).astype(np.complex64)


# ---------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("N", [8, 16, 32, 64])
@pytest.mark.parametrize("P", [1, 2, 4, 8])
@pytest.mark.parametrize("span", [False, True])
def test_kernel_matches_the_restatement(N, P, span):
    """nchan 3, nbeam 8 (pairs 1..2 of 4 selected), gulps of 512 samples, 6 gulps in a row: the PFB history crosses gulps;
    windows of F/2 frames (two per gulp) or of 2F frames (one per two gulps, the other gulp's output NULL or untouched)."""
    nchan, nbeam, ntime, pair0, npair, ngulp = 3, 8, 512, 1, 2, 6
    F = ntime // N
    W = 2 * F if span else F // 2
    rng = np.random.default_rng(1000 * N + 10 * P + span)
    h = rng.standard_normal(P * N).astype(np.float32) if P > 1 else None
    ub = UB(nchan, nbeam, ntime, N, W, pair0, npair, ntap=P if P > 1 else None, h=h)
    v = _beams(rng, nchan, nbeam, ngulp * ntime)
    for g in range(ngulp):
        ub.poison()
        last = not span or g % 2 == 1
        ub.run(v[..., g * ntime:(g + 1) * ntime], out=last or g == 0)
        if not last:
            assert ub.untouched() and _info() == (2, 1, 1)
            continue
        t0 = (g - 1) * ntime if span else g * ntime
        exp = upchan_sum_beams(v, N, W, t0, 2 * ntime if span else ntime, h, pair0, npair)
        check(ub.result(), exp)
    ffi.call("xengUpchanSumBeamsDestroy")


@pytest.mark.parametrize("P", [1, 4])
def test_live_size_long_window(P):
    """96 channels x 32 beams x 960 samples, N = 32, W = 750 frames (25 gulps per window), all 16 pairs: two windows, the
    second after a Reset (a new sequence: the history counts as zero again)."""
    nchan, nbeam, ntime, N, W = 96, 32, 960, 32, 750
    G = W // (ntime // N)
    rng = np.random.default_rng(7 + P)
    h = rng.standard_normal(P * N).astype(np.float32) if P > 1 else None
    ub = UB(nchan, nbeam, ntime, N, W, ntap=P if P > 1 else None, h=h)
    assert _info() == (G, 1, 0)
    for win in range(2):
        if win:
            ffi.call("xengUpchanSumBeamsReset")
        exp, prev = 0.0, None
        for g in range(G):
            gulp = _beams(rng, nchan, nbeam, ntime)
            ub.run(gulp, out=g == G - 1)
            s = gulp if prev is None else np.concatenate([prev, gulp], axis=-1)
            V = beam_channelise(s, N, h, s.shape[-1] - ntime, ntime)
            exp = exp + sum_beams(V, ntime // N)
            prev = gulp
        check(ub.result(), exp, rows=False)
    ffi.call("xengUpchanSumBeamsDestroy")


# ---------------------------------------------------------------- bit identity, the sign convention
def test_bit_identical_repeats_and_beside_an_xengine_contraction():
    """The same two windows three times (Reset between): bit for bit, the third while X-engine contractions run on their own
    stream."""
    nchan, nbeam, ntime, N, W, P = 8, 16, 960, 32, 60, 4
    rng = np.random.default_rng(11)
    h = rng.standard_normal(P * N).astype(np.float32)
    ub = UB(nchan, nbeam, ntime, N, W, ntap=P, h=h)
    v = _beams(rng, nchan, nbeam, 4 * ntime)

    def windows():
        ffi.call("xengUpchanSumBeamsReset")
        outs = []
        for g in range(4):
            ub.run(v[..., g * ntime:(g + 1) * ntime], out=g % 2 == 1)
            if g % 2:
                outs.append(ub.result().copy())
        return outs

    a = windows()
    b = windows()
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    x = Xgpu(352, 96, 480, max_gulps=4)
    try:
        x.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        for k in range(4):
            ffi.call("xengXgpuKernelAsync", x.inbuf.ptr + k * x.gulp_bytes, x.out.ptr, int(k == 3))
        c = windows()
        ffi.call("xengXgpuSync")
    finally:
        x.close()
    for o in (b, c):
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, o))
    ffi.call("xengUpchanSumBeamsDestroy")


def test_sign_of_the_cross_term():
    """Y = -i X: X conj(Y) = i |X|^2, so Im(XY*) = XX = YY and Re(XY*) = 0."""
    nchan, nbeam, ntime, N = 2, 4, 256, 16
    rng = np.random.default_rng(5)
    v = _beams(rng, nchan, nbeam, ntime)
    v[:, 1::2] = -1j * v[:, 0::2]
    ub = UB(nchan, nbeam, ntime, N, ntime // N)
    ub.run(v)
    o = ub.result().astype(np.float64)
    xx = o[..., 0]
    assert (xx > 0).all() and np.allclose(o[..., 1], xx, rtol=1e-5)
    assert np.allclose(o[..., 3], xx, rtol=1e-5) and np.abs(o[..., 2]).max() <= 1e-5 * xx.max()
    ffi.call("xengUpchanSumBeamsDestroy")


# ---------------------------------------------------------------- the same beams as UpchanBeamform's dual-pol mode
@pytest.mark.parametrize("P", [1, 4])
def test_cross_path_matches_upchan_beamform_dual_pol(P):
    """4-bit input -> xengBeamformRun -> xengUpchanSumBeamsRun equals xengUpchanInitializeDualPol on the same input with the
    coarse weights copied to every fine channel (the same PFB coefficients), over 3 gulps, within 1e-4 of the RMS (the
    beamformer itself holds 1e-5)."""
    nstand, nchan, nbeam, ntime, N, W, ngulp = 96, 4, 4, 192, 16, 4, 3
    ninput = 2 * nstand
    rng = np.random.default_rng(20 + P)
    vin = synth_voltages(ngulp * ntime, nchan, nstand, seed=31 + P).reshape(ngulp * ntime, nchan, ninput)
    w = (rng.uniform(-1, 1, (nchan, nbeam, ninput)) + 1j * rng.uniform(-1, 1, (nchan, nbeam, ninput))).astype(np.complex64)
    h = rng.standard_normal(P * N).astype(np.float32) if P > 1 else None
    ffi.call("xengBeamformInitialize", 0, ninput, nchan, ntime, nbeam, 0)
    dw = ffi.DeviceBuffer(w.nbytes).upload(w)
    db = ffi.DeviceBuffer(nchan * nbeam * ntime * 8)
    ub = UB(nchan, nbeam, ntime, N, W, ntap=P if P > 1 else None, h=h)
    ffi.call("xengUpchanInitializeDualPol", 0, ninput, nchan, ntime, N, nbeam, W)
    if P > 1:
        ffi.call("xengUpchanSetPfb", P, _fp(h))
    wf = np.ascontiguousarray(np.broadcast_to(w[:, None], (nchan, N, nbeam, ninput)))
    dwf = ffi.DeviceBuffer(wf.nbytes).upload(wf)
    din = ffi.DeviceBuffer(ntime * nchan * ninput)
    nout = ub.nout
    dref = ffi.DeviceBuffer(nout)
    for g in range(ngulp):
        din.upload(vin[g * ntime:(g + 1) * ntime])
        ffi.call("xengBeamformRun", din.ptr, db.ptr, dw.ptr)
        ffi.call("xengUpchanSumBeamsRun", db.ptr, ub.dout.ptr)
        ffi.call("xengUpchanRun", din.ptr, dref.ptr, dwf.ptr, 0)
        ffi.call("xengBeamformSync")
        got = ub.result()
        ref = dref.download(np.float32).reshape(ub.shape).astype(np.float64)
        check(got, ref, 1e-4)
        exp = upchan_beamform_pfb(vin[:(g + 1) * ntime], wf, N, nbeam, h if h is not None else np.ones(N), g * ntime, ntime, W, dual_pol=True)
        check(got, exp, 1e-4)
    for name in ("xengUpchanSumBeamsDestroy", "xengUpchanDestroy", "xengBeamformDestroy"):
        ffi.call(name)


# ---------------------------------------------------------------- what needs a context
def test_argument_checks_with_a_context():
    """A NULL output on a gulp that completes a window, misaligned pointers, SetPfb with a gulp shorter than the history:
    INVALID_ARGUMENT, nothing launched; GetInfo reports the window shape."""
    ub = UB(2, 4, 64, 16, 8)                # F = 4, W = 8: two gulps per window
    assert _info() == (2, 1, 0)
    for args in ((ub.din.ptr, ub.dout.ptr + 4), (ub.din.ptr + 8, ub.dout.ptr), (None, ub.dout.ptr)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanSumBeamsRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengUpchanSumBeamsRun", ub.din.ptr, None)
    assert _info() == (2, 1, 1)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanSumBeamsRun", ub.din.ptr, None)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (2, 1, 1)
    h = np.ones(6 * 16, np.float32)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanSumBeamsSetPfb", 6, _fp(h))          # (5 x 16 samples of history > 64)
    assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengUpchanSumBeamsReset")
    assert _info() == (2, 1, 0)
    ffi.call("xengUpchanSumBeamsInitialize", 0, 2, 4, 64, 16, 0, 2, 2)
    assert _info() == (1, 2, 0)
    ffi.call("xengUpchanSumBeamsSync")
    ffi.call("xengUpchanSumBeamsDestroy")


# ---------------------------------------------------------------- the block beside BeamformSumBeams on device rings
def _beam_chain(with_reader, vin, nchan, nstand, nbeam, g, ns, N, W, P, h):
    """Source -> Beamform -> {BeamformSumBeams, UpchanSumBeams (with_reader)} on device rings, the power outputs in pinned host
    memory as the live pipeline has them; returns the sinks' sequences (beams, BeamformSumBeams, UpchanSumBeams or None)."""
    ninput = 2 * nstand
    rng = np.random.default_rng(0x5eed)
    r0, r1, r2 = Ring("gpu-input", space="cuda"), Ring("bf-output", space="cuda"), Ring("bf-pow-output", space="cuda_host")
    bf = Beamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, gpu=0)
    sb = BeamformSumBeams(LOG, r1, r2, nchan=nchan, ntime_gulp=g, ntime_sum=ns, gpu=0)
    sfreq, bw = 40e6, 23925.78125
    bf.freqs = sfreq + bw * np.arange(nchan)
    bf.process_command_strings(_beam_cmds(nchan, nbeam, ninput, rng)[0])
    blocks = [bf, sb]
    s1, s2 = Sink(r1, g * nchan * nbeam * 8), Sink(r2, (nbeam // 2) * (g // ns) * nchan * 16)
    sinks = [s1, s2]
    if with_reader:
        r3 = Ring("ub-output", space="cuda_host")
        blocks.append(UpchanSumBeams(LOG, r1, r3, nchan=nchan, nbeam=nbeam, ntime_gulp=g, nupchan=N, nframe_sum=W, pfb_ntap=P, pfb_coeffs=h, gpu=0))
        sinks.append(Sink(r3, (nbeam // 2) * nchan * N * 16))
    run_blocks(blocks, Source(r0, [(source_header(nchan, nstand, 2, sfreq=sfreq, chan_bw=bw), vin, g * nchan * ninput)]), sinks)
    return [s.sequences for s in sinks] + ([None] if not with_reader else [])


def test_block_beside_beamform_sum_beams_on_device_rings():
    """8 gulps through Beamform to both readers, W = 2 gulps, a 4-tap PFB: UpchanSumBeams' windows equal the restatement of the
    beams Beamform wrote, its header is UpchanBeamform's dual-pol one, and BeamformSumBeams' output is bit for bit what it is
    without the new reader."""
    nchan, nstand, nbeam, g, ns, N, P, ngulp = 4, 32, 8, 96, 24, 16, 4, 8
    W = 2 * g // N
    rng = np.random.default_rng(0xc0ffee)
    vin = rng.integers(0, 256, (ngulp * g, nchan, 2 * nstand), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32)
    beams, pow_with, ub = _beam_chain(True, vin, nchan, nstand, nbeam, g, ns, N, W, P, h)
    _, pow_without, _ = _beam_chain(False, vin, nchan, nstand, nbeam, g, ns, N, W, P, h)
    (_, _, sp1), = beams
    (hd, _, sp3), = ub
    assert len(sp1) == ngulp and len(sp3) == ngulp // 2
    v = np.concatenate([s.view(np.complex64).reshape(nchan, nbeam, g) for s in sp1], axis=-1)
    for k, s in enumerate(sp3):
        check(s.view(np.float32).reshape(1, nbeam // 2, nchan, N, 4), upchan_sum_beams(v, N, W, 2 * k * g, 2 * g, h))
    assert hd['nupchan'] == N and hd['nframe_sum'] == W and hd['npol'] == 2 and hd['nbeam'] == nbeam // 2 and hd['pfb_ntap'] == P
    (_, _, a), = pow_with
    (_, _, b), = pow_without
    assert len(a) == len(b) == ngulp and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
