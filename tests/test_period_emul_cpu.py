"""period_spectrum_kernel without a GPU: the kernel's own source (csrc/period_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/period_emul/) and run as 256 host threads per work-group, barriers and shuffles included.  What this
can show is the kernel's logic -- the swizzled addressing, the fused FFT stages for both parities of log2(NT/2), the untangle in the
bit-reversed domain, the block sums, the mask, the stack and the harmonic reduction -- not its arithmetic on the GPU (no fused
multiply-adds here): A against the float64 restatement at the GPU test's bar, the records bit for bit against the float32
harmonic restatement of that A, and the dead, the NaN and the zapped words exactly."""
import os
import subprocess

import numpy as np
import pytest

from tests.period_ref import harmonic_records, stacks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "period_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "period_kernels.h")
LDS_LINE = "extern __shared__ float2 pr_lds[];"
TOL = 1.45e-5                       # the bar of tests/test_period_gpu.py
RECORD = np.dtype([('H', '<f4'), ('k', '<i4')])

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("period_emul")
    src = open(KERNELS).read()
    assert src.count(LDS_LINE) == 1
    with open(os.path.join(d, "period_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float2* pr_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wno-unknown-pragmas", "-I", str(d), "-I", EMUL,
                           os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, z, keep, nt, nstack, nlevel, nwhite, kmin):
    exe, d = driver
    nser = z.shape[1]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.ascontiguousarray(keep, np.uint8).tobytes())
        f.write(np.ascontiguousarray(z, np.float32).tobytes())
    subprocess.check_call([exe] + [str(v) for v in (nt, nser, nstack, nlevel, nwhite, kmin)] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    n = nser * (nt // 2) * 4
    return raw[:n].view(np.float32).reshape(nser, nt // 2), raw[n:].view(RECORD).reshape(nser, nlevel)


@pytest.mark.parametrize("nt,nwhite,kmin", [(256, 8, 1), (512, 64, 3), (1024, 512, 31), (8192, 64, 2), (16384, 8192, 511)])
def test_kernel_source_on_host_threads(driver, nt, nwhite, kmin):
    """Four series (chi^2 powers with mean / sigma = 55, one dead, one with a NaN in the second segment), a stack of 2, 5 levels, a
    mask that zaps a run across a block edge and, where there is more than one, a whole block."""
    nser, nstack, nlevel, n = 4, 2, 5, nt // 2
    rng = np.random.default_rng(nt)
    z = (rng.chisquare(2 * 55 ** 2, (nstack * nt, nser)) * rng.uniform(0.5, 1.5, nser)).astype(np.float32)
    z[:, 1] = 0
    z[nt + 7, 2] = np.nan
    keep = np.ones(n, np.uint8)
    keep[3 * nwhite - 3:3 * nwhite + 2] = 0
    if nwhite < n:
        keep[nwhite:2 * nwhite] = 0
    A, rec = run(driver, z, keep, nt, nstack, nlevel, nwhite, kmin)
    A_ref, nseg = stacks(z.astype(np.float64), nt, nstack, nwhite, keep, np.float64)[-1]
    ok = [0, 1, 3]
    assert (np.abs(A[ok] - A_ref[ok]) <= TOL * np.maximum(1, A_ref[ok]) * nseg).all()
    assert (A[:, 0] == 0).all() and (A[1, 1:] == nseg).all() and np.isnan(A[2, 1:]).all() and (A[ok][:, keep == 0] == nseg).all()
    exp = harmonic_records(A, nlevel, kmin)
    assert np.array_equal(rec['k'], exp['k']) and np.array_equal(rec['H'].view(np.uint32), exp['H'].view(np.uint32))
    assert (rec['k'][2] == -1).all() and (rec['H'][2] == 0).all() and (rec['k'][ok] >= kmin << np.arange(nlevel)).all()


def test_integer_valued_stack_on_host_threads(driver):
    """The integer-valued stack of tests/test_period_gpu.py: every bin zapped but 40, 41, 104, 105, two tones of equal amplitude at 40
    and 104, a stack of 3: A is 3.0 everywhere, 6.0 at the tones, and the smallest k wins among equal maxima."""
    nt, nstack, nlevel, nser = 512, 3, 5, 10
    n = np.arange(nstack * nt)
    tone = np.cos(2 * np.pi * 40 * n / nt) + np.cos(2 * np.pi * 104 * n / nt)
    z = (100.0 + np.arange(1, nser + 1) * 8.0 * tone[:, None]).astype(np.float32)
    keep = np.zeros(nt // 2, np.uint8)
    keep[[40, 41, 104, 105]] = 1
    A, rec = run(driver, z, keep, nt, nstack, nlevel, 8, 1)
    assert (A[:, keep == 0][:, 1:] == 3.0).all() and (A[:, [40, 104]] == 6.0).all() and (A[:, [41, 105]] < 1e-6).all()
    exp = harmonic_records(A, nlevel, 1)
    assert np.array_equal(rec['k'], exp['k']) and np.array_equal(rec['H'], exp['H'])
    assert (rec['H'][:, 0] == 6.0).all() and (rec['k'][:, 0] == 40).all() and (rec['H'][:, 1] == 9.0).all() and (rec['k'][:, 1] == 40).all()
