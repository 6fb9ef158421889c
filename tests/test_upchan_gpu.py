"""xengUpchan* and UpchanBeamform on the MI355X: the fused FFT + beamform kernel against the float64 restatement of the
reference's chain (tests/upchan_ref.py) at 1e-5 of the output's RMS and of every row's own, in both modes and for every
nupchan; a tone that pins sign, shift and order of the fine channels; bytes past the output untouched; two-part gulps,
weight versions, run-to-run and beside-the-X-engine bit identity; and the blocks on device rings.  No wall-clock assertions."""
import json
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Beamform, Copy, TbfSource, UpchanBeamform  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from oracle import xeng_oracle as orc  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_blocks_cpu import _beam_cmds  # noqa: E402
from tests.upchan_ref import upchan_beamform  # noqa: E402
from tests.upchan_local_ref import check_rows, row_ratios  # noqa: E402

POISON = 0xA5
GUARD = 4096


def rand_weights(rng, nchan, nupchan, nbeam, ninput):
    return (rng.standard_normal((nchan, nupchan, nbeam, ninput)) + 1j * rng.standard_normal((nchan, nupchan, nbeam, ninput))).astype(np.complex64)


def out_shape(ntime, nchan, nupchan, nbeam, nframe_sum):
    nframe = ntime // nupchan
    return (nframe // nframe_sum if nframe_sum else nframe, nbeam, nchan, nupchan), (np.float32 if nframe_sum else np.complex64)


class Upchan:
    """One xengUpchan context plus device buffers for a gulp, its weights and a poisoned output (with a guard after it)."""

    def __init__(self, ninput, nchan, ntime, nupchan, nbeam, nframe_sum=0):
        self.ninput, self.nchan, self.ntime, self.nupchan, self.nbeam, self.nframe_sum = ninput, nchan, ntime, nupchan, nbeam, nframe_sum
        ffi.call("xengUpchanInitialize", 0, ninput, nchan, ntime, nupchan, nbeam, nframe_sum)
        self.shape, self.dtype = out_shape(ntime, nchan, nupchan, nbeam, nframe_sum)
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

    def close(self):
        ffi.call("xengUpchanDestroy")


@pytest.fixture
def upchan():
    made = []

    def make(*a, **k):
        u = Upchan(*a, **k)
        made.append(u)
        return u
    yield make
    for u in made:
        u.close()


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


@pytest.mark.parametrize("nupchan", [8, 16, 32, 64])
@pytest.mark.parametrize("nframe,nframe_sum", [(10, 0), (10, 5), (12, 12), (9, 1)])
@pytest.mark.parametrize("nbeam", [3, 16])
def test_small_shapes_against_restatement(upchan, nupchan, nframe, nframe_sum, nbeam):
    """every nupchan, voltage and power (windows shorter and longer than the kernel's 8-frame tile), 1..4 beams per thread, a
    partial input chunk (20 inputs), every byte value, random complex weights; nothing past the output written"""
    ninput, nchan = 20, 3
    ntime = nframe * nupchan
    rng = np.random.default_rng(nupchan * 100 + nframe * 10 + nframe_sum + nbeam)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    vin.reshape(-1)[:256] = np.arange(256)
    w = rand_weights(rng, nchan, nupchan, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, nupchan, nbeam, nframe_sum)
    check(u.run(vin, w, version=1), upchan_beamform(vin, w, nupchan, nbeam, nframe_sum))


@pytest.mark.parametrize("nbeam", [4, 16])
@pytest.mark.parametrize("nframe_sum", [0, 10])
def test_full_size_against_restatement(upchan, nbeam, nframe_sum):
    """the benchmark point: 704 inputs x 96 channels x 960 samples, N = 32 (30 frames)"""
    ninput, nchan, ntime, N = 704, 96, 960, 32
    rng = np.random.default_rng(nbeam + nframe_sum)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, N, nbeam, nframe_sum)
    check(u.run(vin, w, version=7), upchan_beamform(vin, w, N, nbeam, nframe_sum), rows=False)


@pytest.mark.parametrize("nupchan", [8, 32, 64])
def test_tone_lands_in_its_fine_channel(upchan, nupchan):
    """Input 5 of channel 1 carries 7 exp(2 pi i delta n), delta = (j - N/2) / N, every other input is zero: the fine
    channel j of coarse channel 1 gets it.  For delta in {0, +-1/4, -1/2} the 4-bit samples are exact and ALL the power is
    in j (this pins sign, shift and order); for every other j, j is the brightest fine channel."""
    ninput, nchan, nframe = 8, 2, 2
    N = nupchan
    ntime = nframe * N
    w = np.zeros((nchan, N, 1, ninput), np.complex64)
    w[:, :, 0, 5] = 1
    u = upchan(ninput, nchan, ntime, N, 1, 0)
    u.dw.upload(w)
    n = np.arange(ntime)
    for j in range(N):
        delta = (j - N / 2) / N
        tone = 7 * np.exp(2j * np.pi * delta * n)
        re, im = np.rint(tone.real).astype(int), np.rint(tone.imag).astype(int)
        vin = np.zeros((ntime, nchan, ninput), np.uint8)
        vin[:, 1, 5] = ((re & 0xF) << 4) | (im & 0xF)
        p = np.abs(u.run(vin)[:, 0, :, :]) ** 2                     # [frame][chan][j]
        assert (p[:, 0, :] == 0).all()
        assert (np.argmax(p[:, 1, :], axis=1) == j).all(), j
        if (j - N // 2) % (N // 4) == 0:
            assert np.allclose(p[:, 1, j], (7 * N) ** 2, rtol=1e-6)
            others = np.delete(p[:, 1, :], j, axis=1)
            assert others.max() <= 1e-6 * (7 * N) ** 2, j


def test_parts_versions_and_repeats_are_bit_identical(upchan):
    ninput, nchan, N, nbeam = 64, 6, 32, 5
    ntime = 20 * N
    rng = np.random.default_rng(5)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w0 = rand_weights(rng, nchan, N, nbeam, ninput)
    w1 = rand_weights(rng, nchan, N, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, N, nbeam, 0)
    a = u.run(vin, w0, version=1)
    check(a, upchan_beamform(vin, w0, N, nbeam))
    assert u.run(version=1).tobytes() == a.tobytes()                # run to run
    ntime0 = 7 * N
    p0 = ffi.DeviceBuffer(ntime0 * nchan * ninput).upload(vin[:ntime0])
    p1 = ffi.DeviceBuffer((ntime - ntime0) * nchan * ninput).upload(vin[ntime0:])
    assert u.run(version=1, parts=(p0, p1, ntime0)).tobytes() == a.tobytes()
    # new weights, same pointer, a new version: they take effect (and version 0 as well)
    b = u.run(w=w1, version=2)
    check(b, upchan_beamform(vin, w1, N, nbeam))
    assert u.run(w=w0, version=0).tobytes() == a.tobytes()
    # parts that are not whole frames are refused, nothing launched
    for bad in (ntime0 + 1, ntime, 0):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanRunParts", p0.ptr, bad, p1.ptr, u.dout.ptr, u.dw.ptr, 1)
        assert ei.value.status == 1


def test_beside_xengine_contraction_is_bit_identical(upchan):
    """Once (not a loop): the kernel while the X-engine's MFMA contraction runs on its own stream gives the bits it gives
    alone."""
    ninput, nchan, ntime, N, nbeam = 704, 96, 960, 32, 16
    rng = np.random.default_rng(9)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    u = upchan(ninput, nchan, ntime, N, nbeam, 0)
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


# ---------------------------------------------------------------- the blocks on device rings
def test_upchan_beside_beamform_on_one_input_ring():
    """Beamform and UpchanBeamform read one device input ring (both kernels on the beamformer's stream); UpchanBeamform's
    output spans equal the stand-alone call on the same gulp and weights, bit for bit; Beamform's its oracle."""
    nchan, nstand, nbeam, g, N = 4, 8, 2, 128, 32
    ninput = 2 * nstand
    rng = np.random.default_rng(21)
    vin = rng.integers(0, 256, (3 * g, nchan, ninput), dtype=np.uint8)
    r0, rb, ru = Ring("gpu-input", space="cuda"), Ring("bf-output", space="cuda"), Ring("up-output", space="cuda")
    bf = Beamform(LOG, r0, rb, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g)
    up = UpchanBeamform(LOG, r0, ru, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=40e6)
    cmds, _, _, _ = _beam_cmds(nchan, nbeam, ninput, rng)
    bf.freqs = hdr['sfreq'] + hdr['bw_hz'] / nchan * np.arange(nchan)
    bf.process_command_strings(cmds)
    up_cmds = [c for c in cmds if 'beamcoeffs' in c]
    up.process_command_strings(up_cmds)
    nfr = g // N
    sb = Sink(rb, g * nchan * nbeam * 8)
    su = Sink(ru, nfr * nbeam * nchan * N * 8)
    run_blocks([bf, up], Source(r0, [(hdr, vin, g * nchan * ninput)], wait_readers=2), [sb, su])
    spans = su.sequences[0][2]
    assert len(spans) == 3 and len(sb.sequences[0][2]) == 3
    w = up.weights_cpu
    u = Upchan(ninput, nchan, g, N, nbeam, 0)
    try:
        for k in range(3):
            alone = u.run(vin[k * g:(k + 1) * g], w, version=1)
            assert spans[k].tobytes() == alone.tobytes()
            check(alone, upchan_beamform(vin[k * g:(k + 1) * g], w, N, nbeam))
            beams = orc.beamform(vin[k * g:(k + 1) * g], bf.gains_cpu, g, nchan, ninput, nbeam)
            got = sb.sequences[0][2][k].view(np.complex64).reshape(beams.shape)
            assert np.max(np.abs(got - beams)) <= 1e-5 * np.sqrt(np.mean(np.abs(beams) ** 2))
    finally:
        u.close()


def test_tbf_file_to_copy_to_upchan(tmp_path):
    """TbfSource (host ring) -> Copy (device ring) -> UpchanBeamform in power mode, from a .tbf file."""
    nchan, nstand, nbeam, g, N, ns = 3, 4, 2, 64, 16, 2
    ninput = 2 * nstand
    rng = np.random.default_rng(33)
    vin = rng.integers(0, 256, (3 * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=30e6)
    hdr['seq'] = 5000
    path = os.path.join(str(tmp_path), "lwa-dump-1.00.tbf.0")
    hjson = json.dumps(hdr).encode()
    with open(path, "wb") as fh:
        fh.write(struct.pack('<II', len(hjson), 512) + hjson)
        fh.write(b"\0" * (512 - 8 - len(hjson)))
        fh.write(vin.tobytes())
    rh, rd, ru = Ring("tbf", space="system"), Ring("tbf-gpu", space="cuda"), Ring("up-output", space="cuda")
    src = TbfSource(LOG, rh, [path], ntime_gulp=g)
    cp = Copy(LOG, rh, rd, ntime_gulp=g, nbyte_per_time=nchan * ninput)
    up = UpchanBeamform(LOG, rd, ru, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=ns)
    w = rand_weights(rng, nchan, N, nbeam, ninput)
    up.weights_cpu[...] = w
    nout = (g // N // ns) * nbeam * nchan * N * 4
    su = Sink(ru, nout)
    import threading
    ths = [threading.Thread(target=b.main, daemon=True) for b in (src, cp, up)]
    su.start()
    for t in ths[::-1]:
        t.start()
    for t in ths + [su]:
        t.join(60)
        assert not t.is_alive()
    ohdr, _, spans = su.sequences[0]
    assert ohdr['seq0'] == 5000 and ohdr['nframe_sum'] == ns and len(spans) == 3
    for k in range(3):
        check(spans[k].view(np.float32).reshape(-1, nbeam, nchan, N), upchan_beamform(vin[k * g:(k + 1) * g], w, N, nbeam, ns))
