"""The long-segment periodicity kernels without a GPU: the kernels' own source (csrc/plong_kernels.h) compiled as host C++ against a
stand-in for <hip/hip_runtime.h> (tests/plong_emul/) and run as 256 host threads per work-group, barriers and shuffles included,
in the order plong.hip launches them.  The driver is a program of its own, built with -fsanitize=address,undefined, and every
buffer has its exact size: a word read or written outside one ends the run.  What this can show is the kernels' logic -- the ingest
across uneven calls, the four-step split and the permutation it leaves, the mirror partner of the untangle, whole whitening
blocks per work-group, the batches, the bands across the sums' tiles, the tie rule -- not the GPU's arithmetic: A at the GPU
test's bar against the float64 restatement, and the records bit for bit against the float32 restatement (tests/plong_ref.py)
from the emulation's own A."""
import os
import subprocess

import numpy as np
import pytest

from tests import plong_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "plong_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "plong_kernels.h")
LDS_LINE = "extern __shared__ float2 pl_lds[];"
TOL = 3.1e-6                        # the bar of tests/test_plong_gpu.py
# worst |A - A_ref| / (max(1, A_ref) * nseg) the emulation shows (g++ -O1, no contraction): 4.2e-7 at 2^15, 9.1e-7 at 2^16 (B = 2^13)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("plong_emul")
    src = open(KERNELS).read()
    assert src.count(LDS_LINE) == 4                 # (the columns, the rows, the untangle and the whitening)
    with open(os.path.join(d, "plong_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float2* pl_lds = (float2*)g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtime inside the program: it starts whatever else the loader brings first)
                           "-Wno-unknown-pragmas", "-I", str(d), "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, x, calls, nt, nstack, nlevel, nwhite, kedge, sb, keep=None):
    """x [nwindows][nser][nprod]; (stacks completed, A [nser][nt/2], records [nser][nlevel][nband])."""
    exe, d = driver
    nser, nprod, nband = x.shape[1], x.shape[2], len(kedge) - 1
    assert sum(calls) == x.shape[0]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([nser, nprod, nt, nstack, nlevel, nwhite, nband, sb, len(calls), int(keep is not None)] + list(kedge) + list(calls), np.int32).tobytes())
        if keep is not None:
            f.write(np.ascontiguousarray(keep, np.uint8).tobytes())
        f.write(np.ascontiguousarray(x, np.float32).tobytes())
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    a = 4 + nser * (nt // 2) * 4
    return (int(raw[:4].view(np.int32)[0]), raw[4:a].view(np.float32).reshape(nser, nt // 2),
            raw[a:].view(plong_ref.RECORD).reshape(nser, nlevel, nband))


def case(seed, nwindows, nprod):
    """Four series: chi^2 powers with mean / sigma = 55, a dead one (S = 1.0 everywhere: every sum of a band is equal and the
    smallest k must win), one with a NaN, and an integer-valued one, white noise 0..49 with a pulse of 30 every 64 windows (a
    comb of strong lines would leave the blocks between its teeth to rounding noise, which no tolerance on S describes)."""
    rng = np.random.default_rng(seed)
    z = (rng.chisquare(2 * 55 ** 2, (nwindows, 4)) * rng.uniform(0.5, 1.5, 4)).astype(np.float32)
    z[:, 1] = 0
    z[nwindows // 3, 2] = np.nan
    z[:, 3] = rng.integers(0, 50, nwindows)
    z[5::64, 3] += 30
    if nprod == 1:
        return z[:, :, None]
    x = rng.standard_normal((nwindows, 4, 4)).astype(np.float32)
    x[..., 0] = np.floor(z / 2)
    x[..., 1] = z - x[..., 0]
    x[:, 2] = np.where(np.isnan(z[:, 2:3]), np.nan, x[:, 2])
    return x


def check(A, rec, nstacks, x, nt, nstack, nlevel, nwhite, kedge, keep=None):
    nseg_total = x.shape[0] // nt
    assert nstacks == nseg_total // nstack
    z64 = plong_ref.series(x, np.float64)
    A_ref, nseg = plong_ref.stacks(z64, nt, nstack, nwhite, keep, np.float64)[-1]
    ok = [0, 1, 3]
    err = np.abs(A[ok] - A_ref[ok]) / (np.maximum(1.0, A_ref[ok]) * nseg)
    print("plong emulation nt=%d: worst |A - A_ref| / (max(1, A_ref) nseg) = %.3g (TOL %.3g)" % (nt, err.max(), TOL))
    assert (err <= TOL).all(), err.max()
    assert (A[:, 0] == 0).all() and not np.signbit(A[:, 0]).any() and (A[1, 1:] == nseg).all() and np.isnan(A[2, 1:]).all()
    if keep is not None:
        assert (A[ok][:, np.asarray(keep) == 0][:, 1:] == nseg).all()
    if nseg == nstack:              # (the records are those of the last completed stack, which is the one A holds)
        exp = plong_ref.plane_of(plong_ref.harmonic_records(A, nlevel, kedge))
        assert rec.tobytes() == exp.tobytes(), np.argwhere((rec['k'] != exp['k']) | (rec['H'].view(np.uint32) != exp['H'].view(np.uint32)))[:5]
        N = nt // 2
        for lv in range(nlevel):
            for b in range(len(kedge) - 1):
                lo, hi = plong_ref.band_range(kedge, b, lv, N)
                assert tuple(rec[2, lv, b]) == (0.0, -1)
                if lo < hi:         # the dead series: every sum equal, the band's first bin
                    assert tuple(rec[1, lv, b]) == (float((1 << lv) * nseg), lo)
                    assert lo <= rec[0, lv, b]['k'] < hi and rec[0, lv, b]['H'] > 0
                else:
                    assert tuple(rec[0, lv, b]) == tuple(rec[1, lv, b]) == (0.0, -1)
    return A_ref


def test_smallest_segment_two_batches_uneven_calls(driver):
    """NT = 2^15 (N = 2^7 x 2^7, four rows per work-group of the rows pass), a stack of 2 and 9 windows past it, nprod = 4, B = 64,
    SB = 2 (two batches), a mask that zaps a run across a block edge, calls of 1, 4, 100, 7 ... windows; three bands whose edges
    fall inside tiles of the sums, the top one empty at level 4."""
    nt, nstack, nlevel, nwhite = 1 << 15, 2, 3, 64
    kedge = [3, 700, 5000, nt // 2]
    x = case(1, nstack * nt + 9, 4)
    calls = [1, 4, 100, 7, 20000, 2, 2, 1, 12000, 30000]
    calls.append(x.shape[0] - sum(calls))
    assert calls[-1] > 0 and sum(calls[:10]) < 2 * nt
    keep = np.ones(nt // 2, np.uint8)
    keep[3 * nwhite - 3:3 * nwhite + 2] = 0
    nstacks, A, rec = run(driver, x, calls, nt, nstack, nlevel, nwhite, kedge, 2, keep)
    check(A, rec, nstacks, x[:nstack * nt], nt, nstack, nlevel, nwhite, kedge, keep)
    assert plong_ref.band_range(kedge, 2, 2, nt // 2)[0] >= nt // 2          # (4 * 5000 > N: empty)


def test_odd_log_segment_and_the_largest_block(driver):
    """NT = 2^16 (N = 2^7 x 2^8: N1 != N2, two rows per work-group), one segment, nprod = 1, B = 2^13 (a work-group of the whitening
    owns one block of 8192 bins), SB = 3 (a batch of three and a batch of one), one call per quarter; one band, 5 levels."""
    nt, nstack, nlevel, nwhite = 1 << 16, 1, 5, 1 << 13
    kedge = [2, nt // 2]
    x = case(2, nt, 1)
    nstacks, A, rec = run(driver, x, [nt // 4] * 4, nt, nstack, nlevel, nwhite, kedge, 3)
    check(A, rec, nstacks, x, nt, nstack, nlevel, nwhite, kedge)
    from tests import period_ref
    old = period_ref.harmonic_records(A, nlevel, 2)
    assert rec['H'][..., 0].tobytes() == old['H'].tobytes() and rec['k'][..., 0].tobytes() == old['k'].tobytes()
