"""The acceleration-search kernels without a GPU: the kernels' own source (csrc/accel_kernels.h with csrc/plong_kernels.h) compiled
as host C++ against a stand-in for <hip/hip_runtime.h> (tests/accel_emul/) and run as 256 host threads per work-group in the order
accel.hip launches them.  The driver is a program of its own, built with -fsanitize=address,undefined, and every buffer has its
exact size: a word read or written outside one -- a gather index outside the segment, say -- ends the run.  Beside the engine's
sequence the driver runs plong.hip's on the segment resampled on the host with the contract's index rule, and ends with status 4
unless the two sets of trial records are equal byte for byte.  What this can show is the kernels' logic (the index map in the
gathered mean and columns pass, batch-local buffers, the record areas of (trial, batch), the best-over-trials rule), not the
GPU's arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from tests import accel_ref, plong_ref
from tests.test_plong_emul_cpu import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "accel_emul")
CSRC = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc")
LDS_LINE = "extern __shared__ float2 pl_lds[];"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("accel_emul")
    for name, count in (("plong_kernels", 4), ("accel_kernels", 1)):
        src = open(os.path.join(CSRC, name + ".h")).read()
        assert src.count(LDS_LINE) == count
        src = src.replace(LDS_LINE, "float2* pl_lds = (float2*)g_lds;")
        if name == "accel_kernels":
            assert src.count('#include "plong_kernels.h"') == 1
            src = src.replace('#include "plong_kernels.h"', '#include "plong_kernels_host.h"')
        with open(os.path.join(d, name + "_host.h"), "w") as f:
            f.write(src)
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtime inside the program: it starts whatever else the loader brings first)
                           "-Wno-unknown-pragmas", "-I", str(d), "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, x, calls, nt, nlevel, nwhite, kedge, sb, alphas, keep=None):
    """x [nwindows][nser][nprod]; (segments completed, trial records [ntrial][nser][nlevel][nband], the plane [nser][nlevel][nband])
    of the last completed segment.  The driver has compared the trial records with the plong sequence on the resampled series."""
    exe, d = driver
    nser, nprod, nband, ntrial = x.shape[1], x.shape[2], len(kedge) - 1, len(alphas)
    assert sum(calls) == x.shape[0]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([nser, nprod, nt, nlevel, nwhite, nband, sb, len(calls), int(keep is not None), ntrial] + list(kedge) + list(calls), np.int32).tobytes())
        f.write(np.asarray(alphas, np.float64).tobytes())
        if keep is not None:
            f.write(np.ascontiguousarray(keep, np.uint8).tobytes())
        f.write(np.ascontiguousarray(x, np.float32).tobytes())
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    n = ntrial * nser * nlevel * nband * 8
    trec = raw[4:4 + n].view(plong_ref.RECORD).reshape(ntrial, nser, nlevel, nband)
    ref = raw[4 + n:4 + 2 * n].view(plong_ref.RECORD).reshape(ntrial, nser, nlevel, nband)
    assert trec.tobytes() == ref.tobytes()
    return int(raw[:4].view(np.int32)[0]), trec, raw[4 + 2 * n:].view(accel_ref.ACCEL_RECORD).reshape(nser, nlevel, nband)


def nan_case(seed, nwindows, nprod):
    """test_plong_emul_cpu's four series (noise, a dead one, one with a NaN, an integer-valued one) with a second NaN in the window
    behind the first: a trial's map steps by 0, 1 or 2 windows, so it may skip one sample but never two neighbours, and the series
    is NaN in every trial."""
    x = case(seed, nwindows, nprod)
    x[nwindows // 3 + 1, 2] = np.nan
    return x


def check(trec, plane, alphas, nt, nlevel, kedge):
    """The plane is the best-over-trials rule on the trial records; the NaN series (2) is empty everywhere, the dead series (1) reads
    every band's first bin at trial 0, the noise series a bin of its band."""
    assert plane.tobytes() == accel_ref.best_over_trials(trec, alphas).tobytes()
    zero = [a for a, al in enumerate(alphas) if al == 0.0]
    for lv in range(nlevel):
        for b in range(len(kedge) - 1):
            lo, hi = plong_ref.band_range(kedge, b, lv, nt // 2)
            assert tuple(plane[2, lv, b]) == (0.0, -1, -1, 0.0) and not np.signbit(plane[2, lv, b]['H']) and not np.signbit(plane[2, lv, b]['H0'])
            if lo < hi:
                assert tuple(plane[1, lv, b]) == (float(1 << lv), lo, 0, float(1 << lv) if zero else 0.0)
                assert lo <= plane[0, lv, b]['k'] < hi and plane[0, lv, b]['H'] > 0 and 0 <= plane[0, lv, b]['ia'] < len(alphas)
                assert plane[0, lv, b]['H0'] == (trec[zero[0], 0, lv, b]['H'] if zero else 0.0)
            else:
                assert tuple(plane[0, lv, b]) == tuple(plane[1, lv, b]) == (0.0, -1, -1, 0.0)


def test_smallest_segment_three_trials_uneven_calls_and_three_batch_sizes(driver):
    """NT = 2^15, nprod = 4, B = 64, a mask across a block edge, three bands (the top one empty at level 4), 9 windows past the
    segment; trials 0, the extreme +0.5 / NT and the dyadic -2^-21 whose products are exact halves at n = 1024 * odd.  Batches of
    1 (four of them) with uneven calls, of 3 (a batch of three and one of one) and of all 4 series: the same records bit for bit."""
    nt, nlevel, nwhite = 1 << 15, 3, 64
    kedge = [3, 700, 5000, nt // 2]
    alphas = [0.0, 0.5 / nt, -2.0 ** -21]
    x = nan_case(1, nt + 9, 4)
    uneven = [1, 4, 100, 7, 20000, 2, 2, 1, 12000]
    uneven.append(x.shape[0] - sum(uneven))
    assert uneven[-1] > 0 and sum(uneven[:9]) < nt
    keep = np.ones(nt // 2, np.uint8)
    keep[3 * nwhite - 3:3 * nwhite + 2] = 0
    outs = []
    for sb, calls in ((1, uneven), (3, [nt // 2, nt // 2 + 9]), (4, [nt, 9])):
        nsegs, trec, plane = run(driver, x, calls, nt, nlevel, nwhite, kedge, sb, alphas, keep)
        assert nsegs == 1
        check(trec, plane, alphas, nt, nlevel, kedge)
        outs.append((trec.tobytes(), plane.tobytes()))
    assert outs[0] == outs[1] == outs[2]
    assert plong_ref.band_range(kedge, 2, 2, nt // 2)[0] >= nt // 2
    # the trials are different searches: the noise series' records differ between them somewhere
    assert trec[0, 0].tobytes() != trec[1, 0].tobytes() and trec[0, 0].tobytes() != trec[2, 0].tobytes()


def test_odd_log_segment_one_trial_without_a_zero_trial(driver):
    """NT = 2^16 (N1 != N2), nprod = 1, B = 2^13, one band, 5 levels, ntrial = 1 with alpha = -0.5 / NT, the other extreme: izero is
    -1 and H0 reads +0 everywhere."""
    nt, nlevel, nwhite = 1 << 16, 5, 1 << 13
    kedge = [2, nt // 2]
    alphas = [-0.5 / nt]
    x = nan_case(2, nt, 1)
    nsegs, trec, plane = run(driver, x, [nt // 4] * 4, nt, nlevel, nwhite, kedge, 4, alphas)
    assert nsegs == 1
    check(trec, plane, alphas, nt, nlevel, kedge)
    assert (plane['H0'] == 0).all() and not np.signbit(plane['H0']).any() and (plane['ia'][[0, 1, 3]] == 0).all()
