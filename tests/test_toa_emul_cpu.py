"""The arrival-phase kernels without a GPU: the kernels' own source (csrc/toa_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/toa_emul/) and run as 256 host threads per work-group with the grids, the LDS bytes and the arguments
toa.hip launches them with.  The driver is a program of its own, built twice by tests/emul_build.py: under the address and
undefined-behaviour sanitizers, where every buffer has its exact size -- a bin past a row in the last four of a thread, a group past
a sub-band's list in a short batch, a row past the last in a tile of 8, a harmonic or a lag past the table's row, an LDS word past
the launch's -- and under the thread sanitizer, which reports a word two threads of a work-group touch with no barrier between them
(the staged chunks of the DFT and the correlation, the two sums of the base kernel, the reduction of the pick).  The thread
sanitizer sees races inside a work-group; it cannot see races between the work-groups of one launch, which run one after another
here.  base, var and the LDS start as NaN, the output as 0xCD; the call runs twice over the same state.  The driver compares every
byte of the output with what this side wrote from the restatement (tests/toa_ref.py) and ends with a status of 4 unless they are
equal.  What this shows is the kernels' logic, bounds and barriers, not the GPU's arithmetic (tests/test_toa_gpu.py).  Nothing is
loaded into Python under a sanitizer."""
import os

import numpy as np
import pytest

from tests import emul_build, toa_cases, toa_ref

EMUL = os.path.join(emul_build.ROOT, "tests", "toa_emul")
LDS_LINE = "extern __shared__ float toa_lds[];"


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("toa_emul")
    src = open(os.path.join(emul_build.CSRC, "toa_kernels.h")).read()
    assert src.count(LDS_LINE) == 4
    with open(os.path.join(d, "toa_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* toa_lds = g_lds;"))
    return emul_build.build_both(d, EMUL, [d]), str(d)


def run(drivers, c, active=None, builds=("asan", "tsan")):
    """The restatement's (records, P, PH, ccf) of a call the driver has reproduced byte for byte under both builds."""
    exes, d = drivers
    X, edges, w, D, L, S, off = (c[k] for k in ('X', 'edges', 'w', 'D', 'L', 'S', 'off'))
    npair, nprod, nchg, nbin = X.shape
    active = np.ones(npair, np.uint8) if active is None else np.array(active, np.uint8)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([npair, nprod, nchg, nbin, len(edges) - 1, D.shape[1], L.shape[1]], np.int32).tobytes())
        for a, t in ((edges, np.int32), (w, np.float32), (D, np.float32), (L, np.float32), (S, np.float32), (off, np.uint8), (active, np.uint8), (X, np.float32)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    out = toa_ref.toa(X, edges, w, D, L, S, off, active)
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        f.write(toa_ref.out_bytes(*out).tobytes())
    nused = sum(int(np.count_nonzero(w[edges[r]:edges[r + 1]])) for r in range(len(edges) - 1))
    for name in builds:
        assert int(emul_build.run(exes[name], os.path.join(d, "in.bin"), os.path.join(d, "exp.bin"))) == nused
    return out


@pytest.mark.parametrize("nprod", [1, 4])
def test_uneven_sub_bands_16_byte_loads_and_groups_left_out(drivers, nprod):
    """2 pairs x 70 groups (sub-bands of 9, 31 and 30 groups, of which 9, 30 and 29 used: batches of 8 with short last ones; NaN and
    Inf in the two of weight 0) x 100 bins (16-byte loads; base chains of 2 and 1 bins) x 33 harmonics x 257 lags (a second
    work-group of one lag); 8 rows: one full tile; partial masks that differ per pair."""
    c = toa_cases.case(1, 2, nprod, 70, 100, toa_cases.EDGES, 33, 257)
    rec, P, PH, ccf = run(drivers, c)
    assert np.isfinite(P).all() and np.isfinite(PH).all() and np.isfinite(ccf).all() and (rec['l'] >= 0).all() and (rec['var'] > 0).all()


@pytest.mark.parametrize("nprod,nchg,nbin,edges,nharm,nlag,kind,active", [
    (1, 70, 5, 3, 2, 1, 'full', [1, 0]),
    (4, 13, 64, 3, 31, 40, 'empty', [1, 1]),
    (1, 9, 68, 1, 6, 300, 'partial', [1, 1]),
    (4, 13, 7, 3, 3, 5, 'partial', [0, 1]),
    (1, 20, 1028, [2, 7, 7, 19], 5, 3, 'partial', [1, 1]),
], ids=["nbin5_nharm2_nlag1_pair1_inactive", "nprod4_nbin64_nharm31_empty_mask", "nsub1_nbin68_nlag300", "nchg13_nbin7_odd_sizes", "nbin1028_an_empty_sub_band"])
def test_the_other_paths(drivers, nprod, nchg, nbin, edges, nharm, nlag, kind, active):
    """5 bins, 2 harmonics and one lag (word loads, one thread with two bins), an inactive pair; 64 bins with 31 harmonics and a pair
    without off-pulse bins (base, var +0); one sub-band (2 rows a pair: a tile of 4 rows with 4 past the last), 68 bins (a base
    chain of 2 bins in four lanes), 300 lags (a second work-group of 44); 13 groups with odd sizes everywhere and pair 0 inactive;
    1028 bins (a second scrunch work-group of one thread, five DFT chunks, the last of 4 bins) with sub-bands that leave groups 0, 1
    and 19 outside and an empty one in the middle (row +0, l = -1)."""
    c = toa_cases.case(nbin + nlag, 2, nprod, nchg, nbin, edges, nharm, nlag, kind)
    rec, P, PH, ccf = run(drivers, c, active)
    for p in range(2):
        if not active[p]:
            assert all(r.tolist() == (-1, 0.0, 0.0, 0.0) for r in rec[p]) and not P[p].any() and not PH[p].any() and not ccf[p].any()
    if kind == 'empty':
        assert not rec[0]['base'].any() and not rec[0]['var'].any() and rec[1]['var'].all()
    if nbin == 1028:
        assert (rec[:, 1]['l'] == -1).all() and not P[:, 1].any() and not ccf[:, 1].any() and (rec[:, [0, 2, 3]]['l'] >= 0).all()


def test_a_sub_band_of_weight_0_a_nan_in_a_used_group_and_constant_data(drivers):
    """Sub-band 1 of 3 has only groups of weight 0 (row +0, l = -1, the band row the sum of the others); one NaN in a used group of
    sub-band 0 of pair 0 stays in that row and the band row (every PH and ccf word NaN, l = -1) and sub-band 2 is untouched;
    constant data in pair 1 (d = 0: every ccf word +0 and l = 0)."""
    c = toa_cases.case(3, 2, 1, 13, 20, [0, 4, 8, 13], 4, 10, left_out=(4, 5, 6, 7))
    c['w'] = (c['w'] != 0).astype(np.float32)          # (weights of 1: the profile of constant data is exact and equals its mean)
    rec, P, PH, ccf = run(drivers, c)
    assert (rec[:, 1]['l'] == -1).all() and not P[:, 1].any() and (rec[:, [0, 2, 3]]['l'] >= 0).all()
    clean = ccf.copy()
    c['X'][0, 0, 2, 5] = np.nan
    c['X'][1] = 2.5
    rec, P, PH, ccf = run(drivers, c)
    assert rec[0]['l'].tolist() == [-1, -1, clean[0, 2].argmax(), -1] and np.isnan(ccf[0, [0, 3]]).all() and np.isnan(P[0]).sum() == 2
    assert np.array_equal(ccf[0, 2], clean[0, 2]) and rec[1]['l'].tolist() == [0, -1, 0, 0] and not ccf[1].any()
