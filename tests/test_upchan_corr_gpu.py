"""xengUpchanCorr* and UpchanCorr on the MI355X: the FFT + fp32-MFMA correlator against golden_corr's file at N = 1 and the
X-engine at 704 inputs (bit for bit), the int64 restatement at N = 2 and 4 (bit for bit), the float64 restatement
(tests/upchan_corr_ref.py) within 1e-6 of sum_f |X_i||X_j| at N = 8..64; Hermitian symmetry, diagonal, a tone, bytes past
the output; fine-range, staging-depth, two-part, run-to-run and beside-the-X-engine bit identity; the full-size point; and
the blocks on device rings.  No wall-clock assertions."""
import json
import os
import struct
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Copy, TbfSource, UpchanCorr  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from oracle import xeng_oracle as orc  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, source_header  # noqa: E402
from tests.upchan_corr_ref import upchan_corr, upchan_corr_int, upchan_corr_scale  # noqa: E402

POISON = 0xA5
GUARD = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_64t_32a_8c_32s_2p_deadbeef.npz")


class UC:
    """One xengUpchanCorr context, the gulps of a test in one device buffer, and a poisoned output with a guard after it."""

    def __init__(self, ninput, nchan, ntime, nupchan, fine_lo=0, fine_hi=None, nstage=0, ngulp=1):
        fine_hi = nchan * nupchan if fine_hi is None else fine_hi
        self.ninput, self.nchan, self.ntime, self.nupchan = ninput, nchan, ntime, nupchan
        self.nfine = fine_hi - fine_lo
        ffi.call("xengUpchanCorrInitialize", 0, ninput, nchan, ntime, nupchan, fine_lo, fine_hi, nstage)
        self.gulp = ntime * nchan * ninput
        self.din = ffi.DeviceBuffer(ngulp * self.gulp)
        self.nout = self.nfine * ninput * ninput * 8
        self.dout = ffi.DeviceBuffer(self.nout + GUARD)

    def info(self):
        import ctypes
        a, b = ctypes.c_int(), ctypes.c_int()
        ffi.call("xengUpchanCorrGetInfo", ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def integrate(self, vin=None, ngulp=None, split=None, download=True):
        """Accumulate gulps 0 .. ngulp-1 of the buffer (vin uploaded first when given), dump; split: each gulp in two parts
        at that sample.  Returns cf32 [nfine][ninput][ninput] (nothing past the output written)."""
        if vin is not None:
            self.din.upload(np.ascontiguousarray(vin).reshape(-1))
            ngulp = vin.shape[0] // self.ntime
        ffi.call("xengMemset", self.dout.ptr, POISON, self.nout + GUARD)
        row = self.nchan * self.ninput
        for k in range(ngulp):
            p = self.din.ptr + k * self.gulp
            if split is None:
                ffi.call("xengUpchanCorrAccumulate", p)
            else:
                ffi.call("xengUpchanCorrAccumulateParts", p, split, p + split * row)
        ffi.call("xengUpchanCorrDump", self.dout.ptr)
        ffi.call("xengUpchanCorrSync")
        guard = self.dout.download(np.uint8, GUARD, self.nout)
        assert (guard == POISON).all(), "bytes past the output were written"
        if not download:
            return None
        return self.dout.download(np.complex64, self.nout // 8).reshape(self.nfine, self.ninput, self.ninput)

    def close(self):
        ffi.call("xengUpchanCorrDestroy")


@pytest.fixture
def uc():
    made = []

    def make(*a, **k):
        u = UC(*a, **k)
        made.append(u)
        return u
    yield make
    for u in made:
        u.close()


def check_structure(v):
    """Hermitian bit for bit, real diagonal."""
    assert np.array_equal(v, np.conj(v.transpose(0, 2, 1)))
    d = np.diagonal(v, axis1=1, axis2=2)
    assert (d.imag == 0).all()


def check_tol(v, vin, N, lo=0, hi=None):
    exp = upchan_corr(vin, N, lo, hi)
    scale = upchan_corr_scale(vin, N, lo, hi)
    err = np.abs(v.astype(np.complex128) - exp)
    worst = np.max(err / np.maximum(scale, 1e-30))
    assert (err <= 1e-6 * scale).all(), "worst |err| / sum|X_i||X_j| = %.3g" % worst


# ---------------------------------------------------------------- exact cross-checks
def test_n1_equals_the_golden_file(uc):
    """N = 1, two 32-frame integrations: the golden file's corr_re / corr_im (make_golden_inputs.py), bit for bit."""
    d = np.load(GOLDEN)
    vin = d['vin']
    ntime, nchan, nstand, npol = vin.shape
    u = uc(nstand * npol, nchan, 32, 1, ngulp=2)
    u.din.upload(vin.reshape(-1))
    for k in range(2):
        ffi.call("xengMemset", u.dout.ptr, POISON, u.nout + GUARD)
        ffi.call("xengUpchanCorrAccumulate", u.din.ptr + k * u.gulp)
        ffi.call("xengUpchanCorrDump", u.dout.ptr)
        ffi.call("xengUpchanCorrSync")
        raw = u.dout.download(np.uint8)
        assert (raw[u.nout:] == POISON).all()
        v = raw[:u.nout].view(np.complex64).reshape(nchan, nstand, npol, nstand, npol).transpose(0, 1, 3, 2, 4)
        assert np.array_equal(v.real, d['corr_re'][k].astype(np.float32))
        assert np.array_equal(v.imag, d['corr_im'][k].astype(np.float32))


def test_n1_at_704_inputs_equals_the_xengine(uc):
    """352 stands x 2 pols, N = 1: the X-engine's visibilities of the same voltages (read through xgpu_lookup_numpy, which
    gives conj(x_s0) x_s1 for s1 >= s0: the conjugate of this convention), bit for bit."""
    nstand, nchan, ntime = 352, 4, 96
    vin = synth_voltages(ntime, nchan, nstand, "full", seed=11)
    x = Xgpu(nstand, nchan, ntime)
    try:
        planar = x.run(vin)
    finally:
        ffi.call("xengXgpuDestroy")
    re, im = orc.xgpu_lookup_numpy(planar, nstand, nchan)          # [c][s0][s1][p0][p1]
    u = uc(2 * nstand, nchan, ntime, 1)
    v = u.integrate(vin.reshape(ntime, nchan, 2 * nstand))
    v = v.reshape(nchan, nstand, 2, nstand, 2).transpose(0, 1, 3, 2, 4)
    s0, s1 = np.triu_indices(nstand)
    assert np.array_equal(v.real[:, s0, s1], re[:, s0, s1].astype(np.float32))
    assert np.array_equal(v.imag[:, s0, s1], -im[:, s0, s1].astype(np.float32))


@pytest.mark.parametrize("nupchan", [2, 4])
def test_n2_n4_equal_the_int64_restatement(uc, nupchan):
    """every byte value, 40 inputs (padded to 64 inside), odd frame counts per gulp (a zero pad frame), two gulps, a fine range
    across coarse channels; |partial sums| < 2^24, so fp32 is exact: bit for bit."""
    ninput, nchan, nframe = 40, 3, 15
    ntime = nframe * nupchan
    rng = np.random.default_rng(nupchan)
    vin = rng.integers(0, 256, (2 * ntime, nchan, ninput), dtype=np.uint8)
    vin.reshape(-1)[:256] = np.arange(256)
    lo, hi = 1, 3 * nupchan - 1
    u = uc(ninput, nchan, ntime, nupchan, lo, hi, ngulp=2)
    v = u.integrate(vin)
    re, im = upchan_corr_int(vin, nupchan, lo, hi)
    assert np.abs(re).max() < 2 ** 24
    assert np.array_equal(v.real, re.astype(np.float32)) and np.array_equal(v.imag, im.astype(np.float32))
    check_structure(v)


# ---------------------------------------------------------------- tolerance and structure
@pytest.mark.parametrize("nupchan,nframe,ngulp", [(8, 125, 16), (16, 61, 4), (32, 30, 8), (64, 15, 4)])
def test_against_the_float64_restatement(uc, nupchan, nframe, ngulp):
    """N = 8..64, up to 2000 frames, 48 inputs: every element within 1e-6 of sum_f |X_i||X_j|; Hermitian, real diagonal,
    nothing past the output written."""
    ninput, nchan = 48, 2
    ntime = nframe * nupchan
    rng = np.random.default_rng(nupchan + nframe)
    vin = rng.integers(0, 256, (ngulp * ntime, nchan, ninput), dtype=np.uint8)
    u = uc(ninput, nchan, ntime, nupchan, ngulp=ngulp)
    v = u.integrate(vin)
    check_tol(v, vin, nupchan)
    check_structure(v)


@pytest.mark.parametrize("nupchan", [8, 32, 64])
def test_tone_lands_in_its_fine_channel(uc, nupchan):
    """Input 5 of channel 1 carries 7 exp(2 pi i delta n), delta = (j - N/2) / N, every other input is zero: merged fine channel
    N + j has the largest autocorrelation of input 5; for delta in {0, +-1/4, -1/2} the samples are exact and all of it is there."""
    ninput, nchan, nframe = 8, 2, 2
    N = nupchan
    ntime = nframe * N
    u = uc(ninput, nchan, ntime, N)
    n = np.arange(ntime)
    for j in range(N):
        delta = (j - N / 2) / N
        tone = 7 * np.exp(2j * np.pi * delta * n)
        re, im = np.rint(tone.real).astype(int), np.rint(tone.imag).astype(int)
        vin = np.zeros((ntime, nchan, ninput), np.uint8)
        vin[:, 1, 5] = ((re & 0xF) << 4) | (im & 0xF)
        v = u.integrate(vin)
        auto = v[:, 5, 5].real
        assert (auto[:N] == 0).all() and np.argmax(auto) == N + j, j
        assert np.count_nonzero(np.delete(v.reshape(2 * N, -1), 5 * ninput + 5, axis=1)) == 0
        if (j - N // 2) % (N // 4) == 0:
            assert auto[N + j] == pytest.approx(nframe * (7 * N) ** 2, rel=1e-6)
            assert np.delete(auto, N + j).max() <= 1e-6 * nframe * (7 * N) ** 2


# ---------------------------------------------------------------- bit identity
def test_range_depth_parts_and_repeats_are_bit_identical(uc):
    ninput, nchan, N, nframe, ngulp = 70, 3, 16, 9, 5
    ntime = nframe * N
    rng = np.random.default_rng(8)
    vin = rng.integers(0, 256, (ngulp * ntime, nchan, ninput), dtype=np.uint8)
    u = uc(ninput, nchan, ntime, N, ngulp=ngulp)
    assert u.info() == (nchan * N, 8)
    full = u.integrate(vin)
    check_tol(full, vin, N)
    assert u.integrate(ngulp=ngulp).tobytes() == full.tobytes()                         # run to run
    assert u.integrate(ngulp=ngulp, split=4 * N).tobytes() == full.tobytes()            # two-part gulps
    # Reset drops what was accumulated; Dump with nothing accumulated writes zeros
    ffi.call("xengUpchanCorrAccumulate", u.din.ptr)
    ffi.call("xengUpchanCorrReset")
    assert u.integrate(ngulp=ngulp).tobytes() == full.tobytes()
    assert not u.integrate(ngulp=0).any()
    u.close()
    for nstage in (1, 2):
        u = uc(ninput, nchan, ntime, N, nstage=nstage, ngulp=ngulp)
        assert u.info() == (nchan * N, nstage)
        assert u.integrate(vin).tobytes() == full.tobytes(), nstage
        u.close()
    lo, hi = 13, 37
    u = uc(ninput, nchan, ntime, N, lo, hi, ngulp=ngulp)
    assert u.integrate(vin).tobytes() == full[lo:hi].tobytes()
    # parts that are not whole frames are refused, nothing launched
    for bad in (4 * N + 1, ntime, 0):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanCorrAccumulateParts", u.din.ptr, bad, u.din.ptr + 4 * N * nchan * ninput)
        assert ei.value.status == 1


def test_beside_xengine_contraction_is_bit_identical(uc):
    """Once (not a loop): the kernels while the X-engine's MFMA contraction runs on its own stream give the bits they give
    alone."""
    ninput, nchan, ntime, N = 704, 8, 960, 32
    rng = np.random.default_rng(9)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    u = uc(ninput, nchan, ntime, N)
    alone = u.integrate(vin).tobytes()
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    x = Xgpu(352, 96, 480, max_gulps=4)
    try:
        x.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        for k in range(4):
            ffi.call("xengXgpuKernelAsync", x.inbuf.ptr + k * x.gulp_bytes, x.out.ptr, int(k == 3))
        ffi.call("xengMemset", u.dout.ptr, POISON, u.nout + GUARD)
        for _ in range(3):                  # (three integrations so that one of them overlaps the contractions)
            ffi.call("xengUpchanCorrAccumulate", u.din.ptr)
            ffi.call("xengUpchanCorrDump", u.dout.ptr)
        ffi.call("xengUpchanCorrSync")
        ffi.call("xengXgpuSync")
        beside = u.dout.download(np.uint8)[:u.nout].tobytes()
    finally:
        ffi.call("xengXgpuDestroy")
    assert beside == alone


def test_full_size_point(uc):
    """704 inputs x 96 channels x 960 samples, N = 32 (3072 fine channels, 30 frames a gulp), three gulps in one integration:
    a sample of fine channels against the restatement, Hermitian, nothing past the 12 GB output written."""
    ninput, nchan, ntime, N, ngulp = 704, 96, 960, 32, 3
    rng = np.random.default_rng(12)
    vin = rng.integers(0, 256, (ngulp * ntime, nchan, ninput), dtype=np.uint8)
    u = uc(ninput, nchan, ntime, N, ngulp=ngulp)
    u.integrate(vin, download=False)
    per = ninput * ninput
    for m in (0, 31, 17 * 32 + 5, 48 * 32 + 16, 3071):
        v = u.dout.download(np.complex64, per, m * per * 8).reshape(1, ninput, ninput)
        c = m // N
        part = vin[:, c:c + 1, :]
        check_tol(v, part, N, m % N, m % N + 1)
        check_structure(v)


# ---------------------------------------------------------------- the blocks on device rings
def test_tbf_file_to_copy_to_upchan_corr(tmp_path):
    """TbfSource (host ring) -> Copy (device ring) -> UpchanCorr, from a .tbf file: two integrations of two gulps each over a
    fine range, each within 1e-6 of the restatement; the header's seq0 is the file's."""
    nchan, nstand, g, N = 3, 4, 64, 16
    ninput = 2 * nstand
    rng = np.random.default_rng(33)
    vin = rng.integers(0, 256, (4 * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=30e6)
    hdr['seq'] = 5000
    path = os.path.join(str(tmp_path), "lwa-dump-1.00.tbf.0")
    hjson = json.dumps(hdr).encode()
    with open(path, "wb") as fh:
        fh.write(struct.pack('<II', len(hjson), 512) + hjson)
        fh.write(b"\0" * (512 - 8 - len(hjson)))
        fh.write(vin.tobytes())
    lo, hi = 7, 40
    rh, rd, ru = Ring("tbf", space="system"), Ring("tbf-gpu", space="cuda"), Ring("uc-output", space="cuda")
    src = TbfSource(LOG, rh, [path], ntime_gulp=g)
    cp = Copy(LOG, rh, rd, ntime_gulp=g, nbyte_per_time=nchan * ninput)
    up = UpchanCorr(LOG, rd, ru, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=2 * g // N, fine_lo=lo, fine_hi=hi)
    su = Sink(ru, (hi - lo) * ninput * ninput * 8)
    ths = [threading.Thread(target=b.main, daemon=True) for b in (src, cp, up)]
    su.start()
    for t in ths[::-1]:
        t.start()
    for t in ths + [su]:
        t.join(60)
        assert not t.is_alive()
    ffi.call("xengUpchanCorrDestroy")
    ohdr, _, spans = su.sequences[0]
    assert ohdr['seq0'] == 5000 and ohdr['nfine'] == hi - lo and len(spans) == 2
    for k in range(2):
        part = vin[2 * k * g:(2 * k + 2) * g]
        check_tol(spans[k].view(np.complex64).reshape(hi - lo, ninput, ninput), part, N, lo, hi)
