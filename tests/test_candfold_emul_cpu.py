"""The candidate folder's kernels without a GPU: the kernels' own source (csrc/candfold_kernels.h) compiled as host C++ against a
stand-in for <hip/hip_runtime.h> (tests/candfold_emul/) and run as 256 host threads per work-group in the order candfold.hip
launches them.  The driver is a program of its own, built with -fsanitize=address,undefined, and every buffer has its exact size: a
word read or written outside one -- a cell outside a candidate's cube, a window past the call, an LDS word past the launch's --
ends the run.  After every completed segment the driver compares cube, hits, records and best profiles with the bytes this side
wrote from the restatement (tests/candfold_ref.py) and ends with a status of 4 or more unless they are equal.  What this can show is
the kernels' logic (the tile walk, the cell owners, the groups of lanes per trial, the boxcar buffers, the tie rule, the two cubes
and candidate tables changing places), not the GPU's arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from caltech_bifrost_dsp_amd.blocks import candfold_gains, candfold_trials, fold_phase
from tests import candfold_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "candfold_emul")
CSRC = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc")
LDS_LINE = "extern __shared__ float cf_lds[];"
CAND = np.dtype([('phi0', '<u8'), ('dphi', '<u8'), ('ddphi', '<i8'), ('series', '<u4'), ('active', '<u4')])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("candfold_emul")
    src = open(os.path.join(CSRC, "candfold_kernels.h")).read()
    assert src.count(LDS_LINE) == 2
    with open(os.path.join(d, "candfold_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* cf_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtime inside the program: it starts whatever else the loader brings first)
                           "-Wno-unknown-pragmas", "-I", str(d), "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def osc(period, f1=0.0, phase=0.0):
    return fold_phase(1.0 / period, f1, -phase * period, 0.0, 1.0)


def run(driver, x, calls, sets, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains=None):
    """x [nwindows][nser][nprod]; sets: [(the call before which it is given, [(series, phi0, dphi, ddphi, active)])].  The restatement
    runs the same calls and writes the expectation; the driver compares.  Returns the restatement's (records, profiles) per
    completed segment."""
    exe, d = driver
    nser, nprod = x.shape[1], x.shape[2]
    gains = candfold_gains(nbin, nwidth) if gains is None else np.asarray(gains, np.float32)
    assert sum(calls) == x.shape[0]
    ref = candfold_ref.CandfoldRef(1, nser, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([nser, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, len(d1), len(calls), len(sets)], np.int32).tobytes())
        f.write(np.asarray(d1, np.int32).tobytes() + np.asarray(d2, np.int32).tobytes() + gains.tobytes() + np.asarray(calls, np.int32).tobytes())
        for at, cands in sets:
            tab = np.zeros(len(cands), CAND)
            for k, c in enumerate(cands):
                tab[k] = (c[1], c[2], c[3], c[0], c[4])
            f.write(np.array([at, len(cands)], np.int32).tobytes() + tab.tobytes())
        f.write(np.ascontiguousarray(x, np.float32).tobytes())
    outs, n = [], 0
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        for ic, nc in enumerate(calls):
            for at, cands in sets:
                if at == ic:
                    ref.set_candidates(*zip(*cands))
            out = ref.run(x[n:n + nc].reshape(nc, 1, nser, nprod))
            n += nc
            if out is not None:
                f.write(ref.cube.tobytes() + ref.hits.tobytes() + out[0].tobytes() + out[1].tobytes())
                outs.append(out)
    got = subprocess.check_output([exe, os.path.join(d, "in.bin"), os.path.join(d, "exp.bin")])
    assert int(got) == len(outs)
    return outs


def case(seed, nwindows, nser, nprod):
    """noise of mean 55 and sigma 1 (XX and YY half each with nprod = 4); series 1 dead, series 2 with a NaN window, series 3 with a
    pulse every 9.25 windows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nwindows, nser, nprod)) * 50
    if nprod == 1:
        x[..., 0] = 55 + rng.standard_normal((nwindows, nser))
    else:
        x[..., 0] = 27.5 + 0.7 * rng.standard_normal((nwindows, nser))
        x[..., 1] = 27.5 + 0.7 * rng.standard_normal((nwindows, nser))
    x[:, 1] = 0
    x[nwindows // 3, 2] = np.nan
    x[:, 3, 0] += 4.0 * ((np.arange(nwindows) / 9.25) % 1.0 < 0.1)
    return x.astype(np.float32)


def test_smallest_shape_uneven_calls_a_straddling_call_and_a_set_that_waits(driver):
    """nbin 16, nsub 2 x 37 windows, one width, nprod 4, 15 trials, three segments.  Calls of one window, calls that end on a
    sub-integration's and on the segment's last window, one that straddles the segment's end; a second set given exactly on a
    boundary (it holds at once) and a third one given mid-segment (it holds from the boundary the straddling call crosses).  Five slots: a period
    of 5.3 windows, one longer than the segment, one with a derivative, two on one series, an inactive one; a slot unset."""
    nbin, nsub, nsubwin = 16, 2, 37
    nt = nsub * nsubwin
    x = case(1, 3 * nt, 5, 4)
    calls = [1, 36, 37, 1, 20, 60, 30, 30, 7]
    assert sum(calls) == 3 * nt and sum(calls[:3]) == nt and sum(calls[:5]) < 2 * nt < sum(calls[:6])
    a = [(4,) + osc(5.3) + (1,), (0,) + osc(3000.0, phase=0.3) + (1,), (3,) + osc(9.25, f1=2e-5) + (1,), (4,) + osc(7.25, phase=0.5) + (1,), (2,) + osc(9.0) + (0,)]
    b = [(3,) + osc(9.25) + (1,), (1,) + osc(4.0) + (1,), (2,) + osc(11.0) + (1,)]
    d1, d2 = candfold_trials(2, 1)
    sets = [(0, a), (3, b), (5, a[:2])]
    outs = run(driver, x, calls, sets, 6, nbin, nsub, nsubwin, 1, d1, d2)
    assert len(outs) == 3
    assert (outs[0][0]['it'][:4] >= 0).all() and tuple(outs[0][0][4]) == tuple(outs[0][0][5]) == candfold_ref.EMPTY
    # the dead series: every score +0, the first trial, width and bin; the NaN series: no score
    assert tuple(outs[1][0][1]) == (0.0, 0.0, 0, 0, 0, 0) and tuple(outs[1][0][2]) == candfold_ref.EMPTY and outs[1][0]['it'][0] >= 0
    assert (outs[2][0]['it'][:2] >= 0).all() and tuple(outs[2][0][2]) == candfold_ref.EMPTY


@pytest.mark.parametrize("nbin,nsub,nsubwin,nwidth,ntrial", [(64, 7, 64, 5, 33), (256, 32, 8, 8, 99), (32, 3, 40, 4, 35), (128, 64, 3, 7, 9), (32, 2, 20, 2, 4096)])
def test_every_group_size_of_the_refinement(driver, nbin, nsub, nsubwin, nwidth, ntrial):
    """nbin 32, 64, 128 and 256 (8, 4, 2 and 1 groups of lanes a work-group), odd and largest nsub, every count of widths up to 8,
    trial counts that do not fill the last round of groups and the largest table of 4096, nprod 1: one segment and a few windows
    more, uneven calls."""
    nt = nsub * nsubwin
    x = case(nbin, nt + 5, 4, 1)
    if ntrial == 4096:
        i = np.arange(4096)
        d1, d2 = ((i % 64) - 32) * 24, ((i // 64) - 32) * 24
    else:
        d1, d2 = candfold_trials(*{33: (16, 0), 9: (4, 0), 35: (3, 2), 99: (4, 5)}[ntrial])
    assert len(d1) == ntrial
    rng = np.random.default_rng(nbin)
    calls = []
    while sum(calls) < nt + 5:
        calls.append(min(int(rng.integers(1, min(nt, 300) + 1)), nt + 5 - sum(calls)))
    cands = [(3,) + osc(9.25, phase=0.1) + (1,), (0,) + osc(2.0 * nbin / 3, f1=1e-6) + (1,), (2,) + osc(17.0) + (1,), (1,) + osc(5.0) + (1,)]
    (out,) = run(driver, x, calls, [(0, cands)], 4, nbin, nsub, nsubwin, nwidth, d1, d2)
    assert out[0]['it'][0] >= 0 and out[0]['S'][0] >= out[0]['S0'][0] > 0 and tuple(out[0][2]) == candfold_ref.EMPTY
    assert tuple(out[0][3]) == (0.0, 0.0, 0, 0, 0, 0)


def test_the_tie_rule_on_an_integer_cube(driver):
    """tests/test_candfold_gpu.py's integer case: equal maxima across trials, widths and bins; the record names the first trial of the
    equal ones, width 0, bin 3."""
    nbin, nsub, nsubwin = 16, 4, 64
    nt = nsub * nsubwin
    k = np.arange(nt)
    z = np.zeros(nt, np.float32)
    z[k % 16 == 3] = 8
    z[k % 16 == 9] = 8
    x = np.stack([z, 2 * z], axis=1).reshape(nt, 2, 1)
    o = (0, (1 << 64) // 16, 0)
    (out,) = run(driver, x, [100, 100, 56], [(0, [(0,) + o + (1,), (1,) + o + (1,)])], 3, nbin, nsub, nsubwin, 2, [64, 1, 0, -1], [0, 0, 0, 0], gains=[6.0, 7.0])
    assert tuple(out[0][0]) == (42.0, 42.0, 1, 0, 3, 0) and tuple(out[0][1]) == (84.0, 84.0, 1, 0, 3, 0)
