"""The rotation-measure synthesis kernels without a GPU: the kernels' own source (csrc/rmsynth_kernels.h) compiled as host C++
against a stand-in for <hip/hip_runtime.h> (tests/rmsynth_emul/) and run as 256 host threads per work-group with the grids, the LDS
bytes and the arguments rmsynth.hip launches them with.  The driver is a program of its own, built twice by tests/emul_build.py:
under the address and undefined-behaviour sanitizers, where every buffer has its exact size -- a bin past a row in a ragged tile, a
depth past the table's row, a channel past the list of used ones in a short chunk, a partial past the runs, an LDS word past the
launch's -- and under the thread sanitizer, which reports a word two threads of a work-group touch with no barrier between them
(the two chunk buffers taken in turn, the pw tile in their place, the reduction of the pick).  The thread sanitizer sees races
inside a work-group; it cannot see races between the work-groups of one launch, which run one after another here.  The state and
the LDS start as NaN, the output as 0xCD; the call runs twice over the same state.  The driver compares every byte of the output
with what this side wrote from the restatement (tests/rmsynth_ref.py) and ends with a status of 4 unless they are equal.  What this
shows is the kernels' logic, bounds and barriers, not the GPU's arithmetic (tests/test_rmsynth_gpu.py).  Nothing is loaded into
Python under a sanitizer."""
import os

import numpy as np
import pytest

from tests import emul_build, rmsynth_cases, rmsynth_ref

EMUL = os.path.join(emul_build.ROOT, "tests", "rmsynth_emul")
LDS_LINE = "extern __shared__ float rm_lds[];"


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("rmsynth_emul")
    src = open(os.path.join(emul_build.CSRC, "rmsynth_kernels.h")).read()
    assert src.count(LDS_LINE) == 3
    with open(os.path.join(d, "rmsynth_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* rm_lds = g_lds;"))
    return emul_build.build_both(d, EMUL, [d]), str(d)


def run(drivers, X, T, w, use, off, on, active, feeds, builds=("asan", "tsan")):
    """The restatement's (records, spec, profile) of a call the driver has reproduced byte for byte under both builds."""
    exes, d = drivers
    npair, _, nchg, nbin = X.shape
    nphi = T.shape[1]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([npair, nchg, nbin, nphi, feeds], np.int32).tobytes())
        for a, t in ((T, np.float32), (w, np.float32), (use, np.uint8), (off, np.uint8), (on, np.uint8), (active, np.uint8), (X, np.float32)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    rec, spec, prof = rmsynth_ref.rmsynth(X, T, w, use, off, on, active, feeds)
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        f.write(rmsynth_ref.out_bytes(rec, spec, prof).tobytes())
    for name in builds:
        assert int(emul_build.run(exes[name], os.path.join(d, "in.bin"), os.path.join(d, "exp.bin"))) == int(np.count_nonzero(use))
    return rec, spec, prof


def test_ragged_tiles_in_all_three_dimensions_with_channels_left_out(drivers):
    """2 pairs x 70 groups (nine chunks of 8, the last with 4 of the 68 used; NaN and Inf in the two left out) x 100 bins (two runs,
    the second of 36: 16-byte loads) x 130 depths (three tiles, the last with 2 depths); partial masks that differ per pair."""
    T, w, use = rmsynth_cases.table(70, 130)
    X = rmsynth_cases.poison_left_out(rmsynth_cases.float_scene(1, 2, 70, 100), use)
    off, on = rmsynth_cases.masks('partial', 2, 100)
    rec, spec, prof = run(drivers, X, T, w, use, off, on, np.ones(2, np.uint8), 0)
    assert np.isfinite(spec).all() and np.isfinite(prof).all() and (rec['k'] >= 0).all() and rec['n_on'].tolist() == [33, 33]


@pytest.mark.parametrize("nchg,nbin,nphi,feeds,kind,active", [
    (70, 5, 1, 1, 'full', [1, 0]),
    (70, 64, 65, 0, 'empty_off', [1, 1]),
    (70, 64, 65, 1, 'empty_on', [1, 1]),
    (9, 68, 6, 0, 'partial', [1, 1]),
    (13, 7, 3, 1, 'partial', [0, 1]),
], ids=["nbin5_nphi1_circular_pair1_inactive", "nbin64_nphi65_empty_off", "nbin64_nphi65_empty_on", "nchg9_nbin68_nphi6", "nchg13_nbin7_nphi3"])
def test_the_other_paths(drivers, nchg, nbin, nphi, feeds, kind, active):
    """5 bins and one depth (word-by-word loads of both, one tile), circular feeds, an inactive pair; one full tile of bins and a
    second tile of one depth (an odd nphi: word-by-word table loads) with a pair without off-pulse bins (baseline +0) or without
    on-pulse bins (k = -1, the profile's Q and U +0); 9 groups (a second chunk of one channel), 68 bins (a run of 4), 6 depths (an
    even nphi whose tile ends inside a 16-byte pair); 13 groups with odd sizes everywhere and pair 0 inactive."""
    T, w, use = rmsynth_cases.table(nchg, nphi)
    X = rmsynth_cases.poison_left_out(rmsynth_cases.float_scene(nbin + nphi, 2, nchg, nbin), use)
    off, on = rmsynth_cases.masks(kind, 2, nbin)
    active = np.array(active, np.uint8)
    rec, spec, prof = run(drivers, X, T, w, use, off, on, active, feeds)
    for p in range(2):
        if not active[p]:
            assert rec[p].tolist() == (-1, 0.0, 0, 0) and not spec[p].any() and not prof[p].any()
    if kind == 'empty_on':
        assert rec[0]['k'] == -1 and rec[0]['n_on'] == 0 and not spec[0].any() and not prof[0, 1:3].any() and prof[0, 0].any() and rec[1]['k'] >= 0
    if kind == 'empty_off':
        assert rec[0]['n_off'] == 0 and rec[0]['k'] >= 0


def test_no_used_channel_a_nan_in_a_used_channel_and_heavy_ties(drivers):
    """Every group left out (no chunk at all: spec is +0 everywhere and the tie goes to k = 0); one NaN in a used channel stays in
    its bin's words: an on-pulse bin makes every depth NaN (k = -1), an off-pulse one only the baseline's channel; constant data
    (y = 0: every word of spec equal, k = 0)."""
    T, w, use = rmsynth_cases.table(13, 10)
    X = rmsynth_cases.float_scene(3, 2, 13, 20)
    off, on = rmsynth_cases.masks('partial', 2, 20)
    rec, spec, _ = run(drivers, X, T, w, np.zeros(13, np.uint8), off, on, np.ones(2, np.uint8), 0)
    assert rec['k'].tolist() == [0, 0] and not spec.any()
    X[0, 0, 3, int(np.flatnonzero(on[0])[0])] = np.nan
    X[1] = 2.5
    rec, spec, prof = run(drivers, X, T, w, use, off, on, np.ones(2, np.uint8), 0)
    assert rec[0]['k'] == -1 and np.isnan(spec[0]).all() and np.isnan(prof[0, 0]).sum() == 1
    assert rec[1]['k'] == 0 and not spec[1].any()
