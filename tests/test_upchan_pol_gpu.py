"""UpchanBeamform's dual-pol mode on the MI355X (xengUpchanInitializeDualPol): [XX, YY, Re(XY*), Im(XY*)] per pair of beams
against the float64 restatement (tests/upchan_pol_ref.py) at 1e-5 of the output's RMS and of every row's own for every
nupchan; bytes past the output untouched; XX / YY bit-identical to the power mode; the sign of Im(XY*) pinned by Y = -iX;
two-part gulps, repeats and beside-the-X-engine bit identity; the power mode again after a dual-pol context; the block on
device rings.  No wall-clock assertions."""
import json
import os
import struct
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Copy, TbfSource, UpchanBeamform  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.upchan_pol_ref import upchan_dual_pol  # noqa: E402
from tests.upchan_local_ref import check_rows, row_ratios  # noqa: E402
from tests.upchan_ref import upchan_beamform  # noqa: E402

POISON = 0xA5
GUARD = 4096


def rand_weights(rng, nchan, nupchan, nbeam, ninput):
    return (rng.standard_normal((nchan, nupchan, nbeam, ninput)) + 1j * rng.standard_normal((nchan, nupchan, nbeam, ninput))).astype(np.complex64)


class UpchanCtx:
    """One xengUpchan context (dual-pol, power or voltage) plus device buffers for a gulp, its weights and a poisoned output with
    a guard after it."""

    def __init__(self, ninput, nchan, ntime, nupchan, nbeam, nframe_sum, dual=True):
        self.ninput, self.nchan, self.ntime, self.nupchan, self.nbeam, self.nframe_sum = ninput, nchan, ntime, nupchan, nbeam, nframe_sum
        nframe = ntime // nupchan
        if dual:
            ffi.call("xengUpchanInitializeDualPol", 0, ninput, nchan, ntime, nupchan, nbeam, nframe_sum)
            self.shape, self.dtype = (nframe // nframe_sum, nbeam // 2, nchan, nupchan, 4), np.float32
        else:
            ffi.call("xengUpchanInitialize", 0, ninput, nchan, ntime, nupchan, nbeam, nframe_sum)
            self.shape = (nframe // nframe_sum if nframe_sum else nframe, nbeam, nchan, nupchan)
            self.dtype = np.float32 if nframe_sum else np.complex64
        self.nout = int(np.prod(self.shape)) * np.dtype(self.dtype).itemsize
        self.din = ffi.DeviceBuffer(ntime * nchan * ninput)
        self.dw = ffi.DeviceBuffer(nchan * nupchan * nbeam * ninput * 8)
        self.dout = ffi.DeviceBuffer(self.nout + GUARD)

    def run(self, vin=None, w=None, version=0, parts=None):
        if vin is not None:
            self.din.upload(vin)
        if w is not None:
            self.dw.upload(w)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.nout + GUARD)
        if parts is None:
            ffi.call("xengUpchanRun", self.din.ptr, self.dout.ptr, self.dw.ptr, version)
        else:
            p0, p1, ntime0 = parts
            ffi.call("xengUpchanRunParts", p0.ptr, ntime0, p1.ptr, self.dout.ptr, self.dw.ptr, version)
        ffi.call("xengUpchanSync")
        raw = self.dout.download(np.uint8)
        assert (raw[self.nout:] == POISON).all(), "bytes past the output were written"
        return raw[:self.nout].view(self.dtype).reshape(self.shape)


@pytest.fixture
def upchan():
    yield UpchanCtx
    ffi.call("xengUpchanDestroy")


def check(got, exp, rows=True):
    """Within 1e-5 of the output's RMS, and every row within 1e-5 of its own (tests/upchan_local_ref.py check_rows); rows=False
    (the full-size point): the worst row's figure is printed, not asserted."""
    rms = np.sqrt(np.mean(np.abs(exp) ** 2))
    err = np.max(np.abs(got.astype(exp.dtype) - exp))
    assert rms > 0 and err <= 1e-5 * rms, "max |err| %.3g = %.3g of RMS %.3g" % (err, err / rms, rms)
    if rows:
        check_rows(got, exp)
    else:
        print("full size %s: max |err| = %.3g of the RMS, worst row %.3g of its own" % (got.shape, err / rms, np.max(row_ratios(got, exp))))


def _parity_points():
    pts = []
    for N in (8, 16, 32, 64):
        for nbeam in sorted({2, 16, 1024 // N}):
            for nframe, ns in ((10, 5), (12, 12), (9, 1), (30, 30)):
                pts.append((N, nbeam, nframe, ns))
    return pts


@pytest.mark.parametrize("nupchan,nbeam,nframe,nframe_sum", _parity_points())
def test_small_shapes_against_restatement(upchan, nupchan, nbeam, nframe, nframe_sum):
    """every nupchan; one and two pairs per thread (nbeam * N up to 1024); windows shorter and longer than the kernel's 8-frame
    tile; a partial input chunk (20 inputs), every byte value, random complex weights; nothing past the output written"""
    ninput, nchan = 20, 3
    ntime = nframe * nupchan
    rng = np.random.default_rng(nupchan * 1000 + nbeam * 100 + nframe * 10 + nframe_sum)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    vin.reshape(-1)[:256] = np.arange(256)
    w = rand_weights(rng, nchan, nupchan, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, nupchan, nbeam, nframe_sum)
    check(u.run(vin, w, version=1), upchan_dual_pol(vin, w, nupchan, nbeam, nframe_sum))


def test_full_size_against_restatement(upchan):
    """704 inputs x 96 channels x 960 samples, N = 32 (30 frames), two pairs, windows of 10 frames"""
    ninput, nchan, ntime, N, nbeam, ns = 704, 96, 960, 32, 4, 10
    rng = np.random.default_rng(77)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, N, nbeam, ns)
    check(u.run(vin, w, version=3), upchan_dual_pol(vin, w, N, nbeam, ns), rows=False)


@pytest.mark.parametrize("nupchan", [8, 16, 32, 64])
@pytest.mark.parametrize("nbeam_of", ["2", "6", "max"])
@pytest.mark.parametrize("nframe,nframe_sum", [(10, 5), (12, 12)])
def test_xx_yy_are_the_power_mode_bit_for_bit(nupchan, nbeam_of, nframe, nframe_sum):
    """The power mode (xengUpchanInitialize), then the dual-pol mode, on the same input and weights: XX / YY of pair p are the
    power outputs of beams 2p / 2p+1 word for word (whatever beams-per-thread either launch picks)."""
    ninput, nchan = 36, 2
    nbeam = 1024 // nupchan if nbeam_of == "max" else int(nbeam_of)
    ntime = nframe * nupchan
    rng = np.random.default_rng(nupchan + nbeam + nframe)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_weights(rng, nchan, nupchan, nbeam, ninput)
    try:
        p = UpchanCtx(ninput, nchan, ntime, nupchan, nbeam, nframe_sum, dual=False).run(vin, w, version=1)
        d = UpchanCtx(ninput, nchan, ntime, nupchan, nbeam, nframe_sum).run(vin, w, version=1)
    finally:
        ffi.call("xengUpchanDestroy")
    assert np.ascontiguousarray(d[..., 0]).tobytes() == np.ascontiguousarray(p[:, 0::2]).tobytes()
    assert np.ascontiguousarray(d[..., 1]).tobytes() == np.ascontiguousarray(p[:, 1::2]).tobytes()


@pytest.mark.parametrize("nupchan", [8, 32, 64])
def test_sign_of_im_xy_from_a_quarter_turn(upchan, nupchan):
    """Every Y input carries its X partner's samples turned by -90 degrees (re_y = im_x, im_y = -re_x, exact in 4 bits for
    X in -7..7), and beams 2p / 2p+1 weight their own pol's inputs alike and the other pol's by zero: Y = -iX, so
    X conj(Y) = i |X|^2.  In every fine channel Im(XY*) = XX and Re(XY*) = 0 (within 1e-5 of XX's RMS), and YY = XX."""
    nstand, nchan, nbeam, nframe, ns = 10, 3, 4, 6, 3
    ninput, N = 2 * nstand, nupchan
    ntime = nframe * N
    rng = np.random.default_rng(40 + N)
    rx = rng.integers(-7, 8, (ntime, nchan, nstand))
    ix = rng.integers(-7, 8, (ntime, nchan, nstand))
    vin = np.zeros((ntime, nchan, nstand, 2), np.uint8)
    vin[..., 0] = ((rx & 0xF) << 4) | (ix & 0xF)
    vin[..., 1] = ((ix & 0xF) << 4) | (-rx & 0xF)
    vin = vin.reshape(ntime, nchan, ninput)
    w = np.zeros((nchan, N, nbeam, ninput), np.complex64)
    ws = rand_weights(rng, nchan, N, nbeam // 2, nstand)
    w[:, :, 0::2, 0::2] = ws
    w[:, :, 1::2, 1::2] = ws
    got = upchan(ninput, nchan, ntime, N, nbeam, ns).run(vin, w, version=1).astype(np.float64)
    xx, yy, re, im = got[..., 0], got[..., 1], got[..., 2], got[..., 3]
    rms = np.sqrt(np.mean(xx ** 2))
    assert rms > 0 and (xx > 0).all()
    assert np.max(np.abs(im - xx)) <= 1e-5 * rms
    assert np.max(np.abs(re)) <= 1e-5 * rms
    assert np.max(np.abs(yy - xx)) <= 1e-5 * rms


def test_parts_and_repeats_are_bit_identical(upchan):
    ninput, nchan, N, nbeam, ns = 64, 6, 32, 6, 4
    ntime = 20 * N
    rng = np.random.default_rng(55)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, N, nbeam, ns)
    a = u.run(vin, w, version=1)
    check(a, upchan_dual_pol(vin, w, N, nbeam, ns))
    assert u.run(version=1).tobytes() == a.tobytes()                # run to run
    ntime0 = 7 * N                                                  # (the split falls inside a window)
    p0 = ffi.DeviceBuffer(ntime0 * nchan * ninput).upload(vin[:ntime0])
    p1 = ffi.DeviceBuffer((ntime - ntime0) * nchan * ninput).upload(vin[ntime0:])
    assert u.run(version=1, parts=(p0, p1, ntime0)).tobytes() == a.tobytes()


def test_beside_xengine_contraction_is_bit_identical(upchan):
    """Once (not a loop): the dual-pol kernel while the X-engine's MFMA contraction runs on its own stream gives the bits it
    gives alone (the cross products are the arithmetic hipcc would pack)."""
    ninput, nchan, ntime, N, nbeam, ns = 704, 96, 960, 32, 16, 5
    rng = np.random.default_rng(19)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, N, nbeam, ns)
    alone = u.run(vin, w, version=1).tobytes()
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    x = Xgpu(352, 96, 480, max_gulps=4)
    try:
        x.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        for k in range(4):
            ffi.call("xengXgpuKernelAsync", x.inbuf.ptr + k * x.gulp_bytes, x.out.ptr, int(k == 3))
        ffi.call("xengMemset", u.dout.ptr, POISON, u.nout + GUARD)
        for _ in range(3):                  # (three launches so that one of them overlaps the contractions)
            ffi.call("xengUpchanRun", u.din.ptr, u.dout.ptr, u.dw.ptr, 1)
        ffi.call("xengUpchanSync")
        ffi.call("xengXgpuSync")
        beside = u.dout.download(np.uint8)[:u.nout].tobytes()
    finally:
        x.close()
    assert beside == alone


def test_power_mode_again_after_dual_pol(upchan):
    """xengUpchanInitialize after a dual-pol context gives the power layout and values again, bit for bit; so does the
    voltage mode."""
    ninput, nchan, N, nbeam, ns = 24, 4, 16, 4, 2
    ntime = 8 * N
    rng = np.random.default_rng(66)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    before = upchan(ninput, nchan, ntime, N, nbeam, ns, dual=False).run(vin, w, version=1)
    volt = upchan(ninput, nchan, ntime, N, nbeam, 0, dual=False).run(vin, w, version=1)
    check(before, upchan_beamform(vin, w, N, nbeam, ns))
    check(upchan(ninput, nchan, ntime, N, nbeam, ns).run(vin, w, version=1), upchan_dual_pol(vin, w, N, nbeam, ns))
    after = upchan(ninput, nchan, ntime, N, nbeam, ns, dual=False).run(vin, w, version=1)
    assert after.shape == (4, nbeam, nchan, N) and after.tobytes() == before.tobytes()
    upchan(ninput, nchan, ntime, N, nbeam, ns).run(vin, w, version=1)
    assert upchan(ninput, nchan, ntime, N, nbeam, 0, dual=False).run(vin, w, version=1).tobytes() == volt.tobytes()


# ---------------------------------------------------------------- the block on device rings
def test_block_on_device_rings():
    """Source -> UpchanBeamform(dual_pol=True) -> Sink on device rings, against the restatement; the header's pair keys."""
    nchan, nstand, nbeam, g, N, ns = 4, 8, 4, 128, 32, 2
    ninput = 2 * nstand
    rng = np.random.default_rng(23)
    vin = rng.integers(0, 256, (3 * g, nchan, ninput), dtype=np.uint8)
    r0, ru = Ring("gpu-input", space="cuda"), Ring("up-output", space="cuda")
    up = UpchanBeamform(LOG, r0, ru, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=ns, dual_pol=True)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    up.weights_cpu[...] = w
    nout = (g // N // ns) * (nbeam // 2) * nchan * N * 16
    su = Sink(ru, nout)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=40e6)
    try:
        run_blocks([up], Source(r0, [(hdr, vin, g * nchan * ninput)]), [su])
    finally:
        ffi.call("xengUpchanDestroy")
    ohdr, _, spans = su.sequences[0]
    assert len(spans) == 3
    assert (ohdr['nbeam'], ohdr['nstand'], ohdr['npol'], ohdr['nbit'], ohdr['complex']) == (nbeam // 2, nbeam // 2, 2, 32, True)
    for k in range(3):
        check(spans[k].view(np.float32).reshape(-1, nbeam // 2, nchan, N, 4), upchan_dual_pol(vin[k * g:(k + 1) * g], w, N, nbeam, ns))


def test_tbf_file_to_copy_to_dual_pol(tmp_path):
    """TbfSource (host ring) -> Copy (device ring) -> UpchanBeamform(dual_pol=True), from a .tbf file written here."""
    nchan, nstand, nbeam, g, N, ns = 3, 4, 2, 64, 16, 4
    ninput = 2 * nstand
    rng = np.random.default_rng(34)
    vin = rng.integers(0, 256, (3 * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=30e6)
    hdr['seq'] = 6000
    path = os.path.join(str(tmp_path), "lwa-dump-2.00.tbf.0")
    hjson = json.dumps(hdr).encode()
    with open(path, "wb") as fh:
        fh.write(struct.pack('<II', len(hjson), 512) + hjson)
        fh.write(b"\0" * (512 - 8 - len(hjson)))
        fh.write(vin.tobytes())
    rh, rd, ru = Ring("tbf", space="system"), Ring("tbf-gpu", space="cuda"), Ring("up-output", space="cuda")
    src = TbfSource(LOG, rh, [path], ntime_gulp=g)
    cp = Copy(LOG, rh, rd, ntime_gulp=g, nbyte_per_time=nchan * ninput)
    up = UpchanBeamform(LOG, rd, ru, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=ns, dual_pol=True)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    up.weights_cpu[...] = w
    su = Sink(ru, (g // N // ns) * (nbeam // 2) * nchan * N * 16)
    ths = [threading.Thread(target=b.main, daemon=True) for b in (src, cp, up)]
    try:
        su.start()
        for t in ths[::-1]:
            t.start()
        for t in ths + [su]:
            t.join(60)
            assert not t.is_alive()
    finally:
        ffi.call("xengUpchanDestroy")
    ohdr, _, spans = su.sequences[0]
    assert ohdr['seq0'] == 6000 and ohdr['nframe_sum'] == ns and ohdr['npol'] == 2 and len(spans) == 3
    for k in range(3):
        check(spans[k].view(np.float32).reshape(-1, nbeam // 2, nchan, N, 4), upchan_dual_pol(vin[k * g:(k + 1) * g], w, N, nbeam, ns))
