"""The cut-out kernels without a GPU: the kernels' own source (csrc/cutout_kernels.h, and csrc/dedisp_kernels.h for the ingest it
launches) compiled as host C++ against a stand-in for <hip/hip_runtime.h> (tests/cutout_emul/) and run as 256 host threads per
work-group with the grids, the LDS bytes and the arguments cutout.hip launches them with.  The driver is a program of its own, built
twice by tests/emul_build.py: under the address and undefined-behaviour sanitizers, where every buffer has its exact size -- a ring
slot past a channel's row, a channel past the plane in a ragged tile, a delay row past the table, an output column past nt, a slot's
area past the output, an LDS word past the launch's -- and under the thread sanitizer, which reports a word two threads of a
work-group touch with no barrier between them (the two halves and the third piece of the scrunch, the keys between the passes and
their rewriting, the boxcar rows, the reduction).  The thread sanitizer sees races inside a work-group; it cannot see races between
the work-groups of one launch, which run one after another here.  The ring, the row records and the LDS start as NaN, the output as
0xCD, and a Reset clears nothing.  After every call the driver compares the ids served and expired and every byte of a serving
call's output with what this side wrote from the restatement (tests/cutout_ref.py) and ends with a status of 5 or more unless they
are equal.  What this shows is the kernels' logic, bounds and barriers, not the GPU's arithmetic (tests/test_cutout_gpu.py).
Nothing is loaded into Python under a sanitizer."""
import os
import shutil

import numpy as np
import pytest

from tests import cutout_cases, cutout_ref, emul_build

EMUL = os.path.join(emul_build.ROOT, "tests", "cutout_emul")
LDS_LINE = "extern __shared__ float co_lds[];"
K_MAD = cutout_cases.K_MAD


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("cutout_emul")
    src = open(os.path.join(emul_build.CSRC, "cutout_kernels.h")).read()
    assert src.count(LDS_LINE) == 3
    with open(os.path.join(d, "cutout_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* co_lds = g_lds;"))
    shutil.copy(os.path.join(emul_build.CSRC, "dedisp_kernels.h"), str(d))      # (unchanged: its LDS is static)
    return emul_build.build_both(d, EMUL, [d]), str(d)


def run(drivers, sizes, x, delays, nhist, reqs, events=(), builds=("asan", "tsan"), **k):
    """reqs: [(at, (id, pair, n_c, ic, dstep))], given before call `at`; events: [(at, weights or None)], None a Reset.  Returns the
    restatement's cut-outs {id: (record, W, P)} and the ids expired."""
    exes, d = drivers
    nwin = k.pop('nwin')
    ref = cutout_ref.CutoutRef(nwin=nwin, delays=delays, nhist=nhist, k_mad=K_MAD, **k)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([k['npair'], k['nfine'], nwin, delays.shape[0], nhist, k['nband'], k['nt'], k['tscr'], k['ndmc'], k['nwidth'], k['nreq_max'],
                          len(sizes), len(reqs), len(events)], np.int32).tobytes() + np.array([K_MAD], np.float32).tobytes())
        f.write(np.asarray(sizes, np.int32).tobytes() + np.ascontiguousarray(delays, np.int32).tobytes())
        for at, row in reqs:
            f.write(np.array([at], np.int32).tobytes() + cutout_ref.requests([row]).tobytes())
        for at, w in events:
            f.write(np.array([at, 1 if w is None else 0], np.int32).tobytes() + np.asarray(np.zeros(k['nfine']) if w is None else w, np.float32).tobytes())
        assert x.shape[0] == sum(sizes) and max(sizes) <= nwin
        f.write(np.ascontiguousarray(x, np.float32).tobytes())
    cuts, gone, nserving, a = {}, [], 0, 0
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        for ic, nc in enumerate(sizes):
            for at, w in events:
                if at == ic:
                    ref.reset() if w is None else ref.set_weights(w)
            ref.request([row for at, row in reqs if at == ic])
            served, expired, out = ref.run(x[a:a + nc], fill=0xCD)
            a += nc
            f.write(np.array([len(served)] + served + [len(expired)] + expired, np.int32).tobytes())
            if out is not None:
                f.write(out.tobytes())
                nserving += 1
                for z, rid in enumerate(served):
                    cuts[rid] = ref.last[z]
            gone += expired
    for name in builds:
        assert int(emul_build.run(exes[name], os.path.join(d, "in.bin"), os.path.join(d, "exp.bin"))) == nserving
    return cuts, gone


SMALL = dict(npair=2, nfine=70, nwin=4, nband=7, nt=16, tscr=2, ndmc=5, nwidth=4, nreq_max=2)


def test_ragged_tiles_a_ring_that_wraps_absent_rows_two_in_a_call_one_too_many_one_expired_and_a_reset(drivers):
    """2 pairs x 70 channels (three ingest tiles of 32, the last with 6 live channels), bands of 10, nt 16 x tscr 2, nhist = ntu + S + 2 nwin - 1
    (what lets a request that is due wait one call more: a ring of 52 slots that 120 windows wrap twice), calls of 1..4 windows.  Request 100 begins before window 0; 101 and
    102 have rows absent below and above the grid, 106 (dstep 3) at both ends; 103, 104 and 105 fall due in one call at nreq_max 2;
    107 has lost its first window when it is asked for; a Reset before call 5 drops 108; channel 11 holds NaN under weight 0."""
    ndmf, S, total = 9, 9, 120
    delays = cutout_cases.table(ndmf, 70, S)
    x = cutout_cases.float_scene(2, total + 14, 2, 70)
    x[:, :, 11] = np.nan
    w = np.ones(70, np.float32)
    w[11] = 0
    sizes = [4, 3, 2, 4, 1] + cutout_cases.random_sizes(1, total, 4)
    starts = np.cumsum([0] + sizes)
    late = int(np.searchsorted(starts, 14 + 80))             # the first call that starts at window 80 of the run after the Reset, or later
    reqs = [(0, (108, 0, 500, 4, 1)), (5, (100, 0, 3, 4, 1)), (5, (101, 1, 40, 0, 1)), (5, (102, 0, 44, ndmf - 1, 1)), (5, (103, 1, 80, 4, 1)),
            (5, (104, 0, 80, 5, 1)), (5, (105, 1, 80, 3, 1)), (5, (106, 0, 95, 4, 3)), (late, (107, 0, 30, 4, 1))]
    cuts, gone = run(drivers, sizes, x, delays, 32 + S + 7, reqs, events=[(0, w), (5, None)], **SMALL)
    assert sorted(cuts) == [100, 101, 102, 103, 104, 105, 106] and gone == [107]
    assert all(c[0]['status'] == 0 and np.isfinite(c[2]).all() for c in cuts.values())
    assert not cuts[101][2][:2].any() and cuts[101][2][2:].all() and not cuts[102][2][3:].any() and cuts[102][2][:3].all()
    assert [bool(r.any()) for r in cuts[106][2]] == [False, True, True, True, False]


@pytest.mark.parametrize("k,ndmf,S,total,reqs", [
    (dict(SMALL, nband=70, tscr=1, ndmc=1, nwidth=1), 9, 9, 60, [(1, 0, 20, 8, 1), (2, 1, 30, 0, 2), (3, 1, 5, 3, 1)]),
    (dict(npair=1, nfine=3, nwin=40, nband=3, nt=16, tscr=64, ndmc=5, nwidth=4, nreq_max=1), 6, 50, 1800, [(7, 0, 600, 2, 1), (8, 0, 1100, 5, 2)]),
    (dict(npair=1, nfine=3, nwin=40, nband=1, nt=1024, tscr=1, ndmc=6, nwidth=10, nreq_max=1), 300, 60, 1400, [(9, 0, 700, 140, 1)]),
    (dict(npair=1, nfine=4, nwin=33, nband=2, nt=16, tscr=4, ndmc=256, nwidth=3, nreq_max=2), 200, 20, 260, [(10, 0, 100, 90, 1), (11, 0, 110, 100, 1)]),
], ids=["nband70_tscr1_ndmc1_nwidth1", "nfine3_tscr64", "nt1024", "ndmc256"])
def test_the_other_paths(drivers, k, ndmf, S, total, reqs):
    """One channel a band, no scrunch, one row and one width; tscr 64 (ntu 1024: four work-groups along m, four columns each, a sum
    of 64 LDS words); nt 1024 (4 KiB rows, four keys a thread and pass, ten widths); 256 rows to pick from around trials 90 and 100
    of 200, some of them absent at either end."""
    delays = cutout_cases.table(ndmf, k['nfine'], S)
    x = cutout_cases.float_scene(total, total, k['npair'], k['nfine'])
    cuts, gone = run(drivers, cutout_cases.whole(total, k['nwin']), x, delays, k['nt'] * k['tscr'] + S + k['nwin'] - 1, [(0, r) for r in reqs], **k)
    assert sorted(cuts) == [r[0] for r in reqs] and not gone and all(c[0]['status'] == 0 for c in cuts.values())


def test_rows_without_a_score_and_heavy_ties(drivers):
    """One NaN at the last window that only the highest trial's row needs (that row alone has no score); a constant pair (A = 0: no
    row is valid, status 1); data of two values (ties decided by the smallest i, iw, j)."""
    ndmf, S, total = 9, 9, 150
    k = dict(SMALL, nreq_max=1)
    delays = cutout_cases.table(ndmf, 70, S)
    x = cutout_cases.float_scene(33, total, 2, 70)
    x[:, 1] = 3.0
    x[96:, 0] = 0
    x[96:, 0, 5, 0] = (np.arange(total - 96) % 4 == 0)
    x[70 - 16 + 31 + int(delays[8, 0]), 0, 0, 1] = np.nan
    cuts, _ = run(drivers, cutout_cases.whole(total, 4), x, delays, 32 + S + 3, [(0, (3, 0, 70, 6, 1)), (0, (4, 1, 60, 4, 1)), (0, (5, 0, 125, 4, 1))], **k)
    assert cuts[3][0]['status'] == 0 and np.isnan(cuts[3][2][4]).any() and np.isfinite(cuts[3][2][:4]).all() and cuts[3][0]['i'] < 4
    assert cuts[4][0]['status'] == 1 and cuts[4][0]['i'] == -1 and cuts[5][0]['status'] == 0 and cuts[5][0]['S'] > 0
