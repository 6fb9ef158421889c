"""The detrender's kernels without a GPU: the kernels' own source (csrc/detrend_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/detrend_emul/) and run as 256 host threads per work-group with the grids, the LDS bytes and the arguments
detrend.hip launches them with.  The driver is a program of its own, built twice by tests/emul_build.py: under the address and
undefined-behaviour sanitizers, where every buffer has its exact size -- a ring slot past a series' row, a series past the plane in
a ragged tile, a window past the call, a knot slot past the four, an LDS word past the launch's -- and under the thread sanitizer,
which reports a word two threads of a work-group touch with no barrier between them (the tile between its two sweeps, the keys
between the passes and their rewriting, the three count words).  The thread sanitizer sees races inside a work-group; it
cannot see races between the work-groups of one launch, which run one after another here.  The ring, the knot tables and the LDS
start as NaN and a Reset clears nothing, so a value used from before window 0 shows.  After every call the driver compares the
output, and after a call that decided a block M, A and the valid bytes, with what this side wrote from the restatement
(tests/detrend_ref.py) and ends with a status of 5 or more unless they are equal.  What this shows is the kernels' logic, bounds
and barriers, not the GPU's arithmetic (tests/test_detrend_gpu.py).  Nothing is loaded into Python under a sanitizer."""
import os

import numpy as np
import pytest

from tests import detrend_cases, detrend_ref, emul_build

EMUL = os.path.join(emul_build.ROOT, "tests", "detrend_emul")
LDS_LINE = "extern __shared__ float dt_lds[];"
K_MAD = detrend_cases.K_MAD


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("detrend_emul")
    src = open(os.path.join(emul_build.CSRC, "detrend_kernels.h")).read()
    assert src.count(LDS_LINE) == 3
    with open(os.path.join(d, "detrend_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* dt_lds = g_lds;"))
    return emul_build.build_both(d, EMUL, [d]), str(d)


def run(drivers, parts, nprod, nblk, nwin, normalise, builds=("asan", "tsan")):
    """parts: [(x [windows][npair][ndm][nprod], sizes)], a Reset between two parts.  Returns per part the restatement's (out, knots)."""
    exes, d = drivers
    nser = int(np.prod(parts[0][0].shape[1:3]))
    calls = [nc for _, sizes in parts for nc in sizes]
    resets = np.cumsum([len(sizes) for _, sizes in parts])[:-1]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([nser, nprod, nblk, nwin, int(normalise), len(calls), len(resets)], np.int32).tobytes() + np.array([K_MAD], np.float32).tobytes())
        f.write(np.asarray(calls, np.int32).tobytes() + np.asarray(resets, np.int32).tobytes())
        for x, sizes in parts:
            assert x.shape[0] == sum(sizes) and x.shape[3] == nprod and max(sizes) <= nwin
            f.write(np.ascontiguousarray(x, np.float32).tobytes())
    results, ndone = [], 0
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        for x, sizes in parts:
            ref = detrend_ref.DetrendRef(nser, nblk, normalise, K_MAD, nprod)
            outs, knots, a = [], [], 0
            for nc in sizes:
                before = ref.nblocks
                o = ref.run(x[a:a + nc])
                a += nc
                f.write(o.tobytes())
                if ref.nblocks > before:
                    f.write(b"".join(t.tobytes() for t in ref.newest))
                    knots.append(ref.newest)
                outs.append(o)
            results.append((np.concatenate(outs), knots))
            ndone += len(knots)
    for name in builds:
        assert int(emul_build.run(exes[name], os.path.join(d, "in.bin"), os.path.join(d, "exp.bin"))) == ndone
    return results


@pytest.mark.parametrize("normalise", [0, 1])
@pytest.mark.parametrize("nprod", [1, 4])
def test_the_smallest_block_calls_of_one_to_four_a_ring_that_wraps_and_a_reset(drivers, nprod, normalise):
    """nblk 4 (h 2, D 6), nwin 4: a ring of 10 slots that 44 windows wrap four times, the four knot slots taken eleven times; 7
    series (one ragged tile).  A prefix into block 2, a Reset, and the whole run on other data."""
    nblk, nwin = 4, 4
    sizes = [1, 2, 3, 4, 4, 1, 1, 2, 4, 3, 3, 4, 1, 2, 4, 4, 1]
    assert sum(sizes) == 44 and 44 // (6 + nwin) >= 3
    x0 = detrend_cases.float_scene(1, 10, 1, 7, nprod, nblk)
    x = detrend_cases.float_scene(2, 44, 1, 7, nprod, nblk)
    (_, _), (out, knots) = run(drivers, [(x0, [4, 4, 2]), (x, sizes)], nprod, nblk, nwin, normalise)
    assert len(knots) == 11 and not out[:6].any() and out[6:, 0].all()
    if normalise:
        assert not out[:, 1].any() and not any(k[2][1] for k in knots)       # the constant series has no scale: never valid


@pytest.mark.parametrize("nprod,normalise", [(1, 1), (4, 0)])
def test_ragged_tiles_a_block_that_is_no_power_of_two_and_calls_that_straddle_a_block_end(drivers, nprod, normalise):
    """nser 70 = 2 x 35 (three tiles of 32, the last with 6 live series), nblk 30 (u is no dyadic fraction), nwin 30: calls of 1 to
    30 windows, some with a block's last window inside, some of more than 32 windows' worth of tiles never (nwin < 32) -- the
    8192 case below has those.  The NaN of series 3 in block 2 and the infinities of series 4 are in."""
    nblk, nwin, total = 30, 30, 130
    sizes = detrend_cases.random_sizes(5, total, nwin)
    ends = np.cumsum(sizes)
    starts = ends - np.array(sizes)
    assert any(a < j * nblk < e for a, e in zip(starts, ends) for j in range(1, 5))
    x = detrend_cases.float_scene(3, total, 2, 35, nprod, nblk)
    (out, knots), = run(drivers, [(x, sizes)], nprod, nblk, nwin, normalise)
    assert len(knots) == 4 and not knots[2][2][3] and knots[1][2][3] and not knots[1][2][4] and not knots[3][2][4]
    assert out[45:, 0].all() and not out[45 + 70, 3]                           # (the NaN's own window, 2 nblk + nblk/3, reads +0)


def test_the_largest_block(drivers):
    """nblk 8192 with 2 series, nprod 4, normalised: 32 KiB of keys, 32 keys a thread and pass, calls of up to 8192 windows (256
    tiles along time).  Two blocks are decided; the outputs reach window 8211 > h, past the first knot."""
    nblk, nwin = 8192, 8192
    sizes = [8192, 5000, 3192, 4116]
    x = detrend_cases.float_scene(4, sum(sizes), 1, 2, 4, nblk, special=False)
    (out, knots), = run(drivers, [(x, sizes)], 4, nblk, nwin, 1)
    assert len(knots) == 2 and out[12288:].all() and not out[:12288].any()
