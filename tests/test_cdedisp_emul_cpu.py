"""cdedisp_filter_kernel without a GPU: the kernel's own source (csrc/cdedisp_kernels.h) compiled as host C++ against the stand-in
for <hip/hip_runtime.h> of tests/period_emul/ and run as 256 host threads per work-group, barriers included, by a driver of its own
(tests/cdedisp_emul/).  What this can show is the kernel's logic -- the swizzled addressing on both sides of its LN >= 12 fold, the
fused stages of the forward transform and their mirror image for both parities of log2 NFFT, the table in bit-reversed order, the
overlap moved behind the barrier, the discard region -- not its arithmetic on the GPU (no fused multiply-adds here).

The bar is the float bar of tests/test_cdedisp_gpu.py: five times the worst gap between the complex64 and the float64 evaluation
of the restatement on this test's own inputs, per row and block as max |y - y_ref| / rms(y_ref).  Measured here with numpy's
single-precision FFT (numpy 2.2): gaps of 1.7e-7 (NFFT 256), 1.5e-7 and 1.6e-7 (512, M 0 and 256), 1.7e-7 (4096) and 2.0e-7 (8192),
so bars of 7.5e-7 to 9.9e-7; the emulated kernel's own worst row stands at 4.4e-7, 5.5e-7 and 5.0e-7, 6.2e-7 and 7.1e-7."""
import os
import subprocess

import numpy as np
import pytest

from tests.cdedisp_ref import filter_blocks, float_gap, gaussian_rows, row_error, unit_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "cdedisp_emul")
STANDIN = os.path.join(ROOT, "tests", "period_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "cdedisp_kernels.h")
LDS_LINE = "extern __shared__ float2 cd_lds[];"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cdedisp_emul")
    src = open(KERNELS).read()
    assert src.count(LDS_LINE) == 1
    with open(os.path.join(d, "cdedisp_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float2* cd_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wno-unknown-pragmas", "-I", str(d), "-I", STANDIN,
                           os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, rows, table, nfft, overlap, nblk):
    exe, d = driver
    nchan, nb, _ = rows.shape
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.ascontiguousarray(table, np.complex64).tobytes())
        f.write(np.ascontiguousarray(rows, np.complex64).tobytes())
    subprocess.check_call([exe] + [str(v) for v in (nfft, overlap, nchan, nb // 2, nblk)] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    return np.fromfile(os.path.join(d, "out.bin"), np.complex64).reshape(nblk, nchan, nb, nfft - overlap)


@pytest.mark.parametrize("nfft,overlap", [(256, 64), (512, 0), (512, 256), (4096, 1216), (8192, 2432)])
def test_kernel_source_on_host_threads(driver, nfft, overlap):
    """Two channels x two pairs of Gaussian rows of scales 0.5 to 50, one row of zeros, unit-modulus tables of random phase (one per
    pair and channel), three blocks: every row and block within five times the complex64 restatement's own gap of the float64
    restatement; the zero row exactly zero; nothing written outside the time buffer and the output (the driver's canaries)."""
    nchan, npair, nblk = 2, 2, 3
    L = nfft - overlap
    rng = np.random.default_rng(nfft + overlap)
    rows = gaussian_rows(rng, nchan, 2 * npair, nfft + (nblk - 1) * L)
    rows[1, 2] = 0
    table = unit_tables(rng, npair, nchan, nfft)
    gap = float_gap(rows, table, nfft, overlap)
    got = run(driver, rows, table, nfft, overlap, nblk)
    ref = filter_blocks(rows, table, nfft, overlap)
    err = row_error(got, ref)
    print("NFFT %d M %d: complex64 gap %.2e, bar %.2e, emulated kernel %.2e" % (nfft, overlap, gap, 5 * gap, err.max()))
    assert 1e-7 < gap < 1e-6          # (the restatement's own sanity: a few ulp)
    assert (err <= 5 * gap).all(), err.max()
    assert (got[:, 1, 2] == 0).all()


def test_delay_table_shifts_the_stream(driver):
    """T = exp(-2 pi i k d / NFFT) / NFFT delays by d samples: with d = M/2 output sample i is input sample i, with d = -M/2 input
    sample i + M, seamless across the blocks.  A wrong discard region or a wrong overlap shows as wrapped samples."""
    nfft, overlap, nchan, npair, nblk = 256, 64, 1, 1, 3
    L, k = nfft - overlap, np.arange(nfft)
    rng = np.random.default_rng(3)
    rows = gaussian_rows(rng, nchan, 2, nfft + (nblk - 1) * L, 1.0, 1.0)
    for d in (overlap // 2, 0, -overlap // 2):
        table = np.broadcast_to(np.exp(-2j * np.pi * k * d / nfft) / nfft, (npair, nchan, nfft)).astype(np.complex64)
        got = run(driver, rows, table, nfft, overlap, nblk).transpose(1, 2, 0, 3).reshape(nchan, 2, nblk * L)
        exp = rows[:, :, overlap // 2 - d:overlap // 2 - d + nblk * L]
        assert np.max(np.abs(got - exp)) <= 3e-6 * np.sqrt(np.mean(np.abs(exp) ** 2)), d
