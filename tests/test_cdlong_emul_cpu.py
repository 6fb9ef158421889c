"""The kernels of csrc/cdlong_kernels.h without a GPU: their own source compiled as host C++ against the stand-in for
<hip/hip_runtime.h> of tests/period_emul/ and run as 256 host threads per work-group, barriers included, launch after launch as
cdlong.hip enqueues them, by a driver of its own (tests/cdlong_emul/).  What this can show is the kernels' logic -- the split of
the index, both LDS layouts, the fused stages over a tile of columns and over several rows of a work-group, the step twiddle on the
load and on the store, the table in pass B's order, the overlap copy behind pass A, the discard region -- not their arithmetic on
the GPU (no fused multiply-adds here).

The bar is that of tests/test_cdlong_gpu.py: per row and block, max |y - y_ref| / rms(y_ref) against the float64 restatement
(tests/cdedisp_ref.py filter_blocks) at most five times a complex64 gap on this test's own inputs, the larger of the direct
complex64 evaluation's and the four-step complex64 evaluation's (tests/cdlong_ref.py).  Measured here (numpy 2.2), as direct gap,
four-step gap, emulated kernel's worst row:
  (2^14, 4560)  1 channel x 1 pair  1.71e-7, 2.67e-7, 7.18e-7 (0.54 of the bar)   2 x 2 pairs  1.95e-7, 3.26e-7, 8.33e-7 (0.51)
  (2^15, 0)     1 channel x 1 pair  1.83e-7, 2.68e-7, 7.88e-7 (0.59)              2 x 2 pairs  2.05e-7, 3.23e-7, 8.07e-7 (0.50)
  (2^15, 2^14)  1 channel x 1 pair  1.92e-7, 2.71e-7, 7.46e-7 (0.55)              2 x 2 pairs  2.38e-7, 2.89e-7, 9.24e-7 (0.64)"""
import os
import subprocess

import numpy as np
import pytest

from tests.cdedisp_ref import filter_blocks, gaussian_rows, row_error, unit_tables
from tests.cdlong_ref import gaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "cdlong_emul")
STANDIN = os.path.join(ROOT, "tests", "period_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "cdlong_kernels.h")
LDS_LINE = "extern __shared__ float2 cl_lds[];"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cdlong_emul")
    src = open(KERNELS).read()
    assert src.count(LDS_LINE) == 3
    with open(os.path.join(d, "cdlong_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float2* cl_lds = g_lds;"))
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


@pytest.mark.parametrize("nchan,npair", [(1, 1), (2, 2)])
@pytest.mark.parametrize("nfft,overlap", [(1 << 14, 4560), (1 << 15, 0), (1 << 15, 1 << 14)])
def test_kernel_source_on_host_threads(driver, nfft, overlap, nchan, npair):
    """(2^14, 4560): N1 = N2 = 128 and an overlap whose half, 2280, is no multiple of the column tile of 16; (2^15, 0) and
    (2^15, 2^14): N1 = 128, N2 = 256, the extreme overlaps.  Gaussian rows of scales 0.5 to 50, one row of zeros, unit-modulus tables
    of random phase (one per pair and channel), three blocks: every row and block within five times the larger complex64 gap; the
    zero row exactly zero; nothing written outside the time buffer, the scratch buffer and the output (the driver's canaries)."""
    nblk = 3
    L = nfft - overlap
    rng = np.random.default_rng(nfft + overlap + nchan)
    rows = gaussian_rows(rng, nchan, 2 * npair, nfft + (nblk - 1) * L)
    zc, zb = nchan - 1, 2 * npair - 2
    rows[zc, zb] = 0
    table = unit_tables(rng, npair, nchan, nfft)
    ref = filter_blocks(rows, table, nfft, overlap)
    direct, four = gaps(rows, table, nfft, overlap, ref)
    gap = max(direct, four)
    got = run(driver, rows, table, nfft, overlap, nblk)
    err = row_error(got, ref)
    print("NFFT %d M %d, %d x %d: direct gap %.2e, four-step gap %.2e, bar %.2e, emulated kernel %.2e (%.2f of the bar)"
          % (nfft, overlap, nchan, npair, direct, four, 5 * gap, err.max(), err.max() / (5 * gap)))
    assert 1e-7 < gap < 1e-6          # (the restatements' own sanity: a few ulp)
    assert (err <= 5 * gap).all(), (err.max(), 5 * gap)
    assert (got[:, zc, zb] == 0).all()


def test_delay_table_shifts_the_stream(driver):
    """T = exp(-2 pi i k d / NFFT) / NFFT delays by d samples: with d = M/2 output sample i is input sample i, with d = -M/2 input
    sample i + M, seamless across the blocks.  A wrong discard region or a wrong overlap shows as wrapped samples.  NFFT 2^14, the
    tolerance of tests/test_cdedisp_emul_cpu.py unchanged (3e-6 of the stream's rms; measured here: 7.4e-7 to 8.5e-7)."""
    nfft, overlap, nchan, npair, nblk = 1 << 14, 4560, 1, 1, 3
    L, k = nfft - overlap, np.arange(nfft)
    rng = np.random.default_rng(3)
    rows = gaussian_rows(rng, nchan, 2, nfft + (nblk - 1) * L, 1.0, 1.0)
    for d in (overlap // 2, 0, -overlap // 2):
        table = np.broadcast_to(np.exp(-2j * np.pi * ((k * d) % nfft) / nfft) / nfft, (npair, nchan, nfft)).astype(np.complex64)
        got = run(driver, rows, table, nfft, overlap, nblk).transpose(1, 2, 0, 3).reshape(nchan, 2, nblk * L)
        exp = rows[:, :, overlap // 2 - d:overlap // 2 - d + nblk * L]
        worst = np.max(np.abs(got - exp)) / np.sqrt(np.mean(np.abs(exp) ** 2))
        print("d %d: worst sample %.2e of the rms" % (d, worst))
        assert worst <= 3e-6, d
