"""The phase folder's kernels without a GPU: the kernels' own source (csrc/fold_kernels.h, unchanged) compiled as host C++ against a
stand-in for <hip/hip_runtime.h> (tests/fold_emul/) and run as 256 host threads per work-group with the grids and the arguments
fold.hip launches them with.  The driver is a program of its own and every buffer has its exact size: a word read or written
outside one -- the repeated loads of a FOLD_BATCH batch's tail, the 8-byte load of fold_input<1> at the call's last channel, a
profile row past nbin, the rot and hits reads of the dump, a tile row past the chunk -- ends the run of the address-sanitizer
build; and a word two threads of a work-group touch with no barrier between them -- the dump's two phases over tile and wq, with
wq written again for every chunk -- is a report of the thread-sanitizer build.  The thread sanitizer sees races inside a
work-group between barriers; it cannot see races between the work-groups of one launch, which run one after another here.  The
device's copy of the hits holds a pattern until a normalising dump uploads them, so a dump that reads hits it should not shows.
After every Run the driver compares the profile, and after every Dump the output, the hits and the profile, word for word with
what this side wrote from the ordered float32 restatement (tests/fold_ref.FoldRef) and ends with a status of 5 or more unless they
are equal: on the host, with -ffp-contract=off, libm's fmaf and IEEE division, the contract is bit for bit on float data.  What
this shows is the kernels' logic, bounds and barriers, not the GPU's arithmetic (tests/test_fold_gpu.py).  Nothing is loaded into
Python under a sanitizer.

Every case has nfine 70 and three pairs, runs under both builds, and is the same list of operations:
  * nprod 4 gives W = 280 words a pair: two work-groups, the second with 24 live lanes; nprod 1 one work-group of 70 lanes, whose
    lane 69 loads XX, YY of the last channel of the call's last window as 8 bytes.
  * Pair 0 turns once in 3.3 windows: with nbin 5 bins repeat inside a batch of 8 and the period is shorter than a call; with
    nbin 64 and 100 most bins have 0 hits when the first normalising dump comes.  Pair 1 is inactive: never folded, its plane +0,
    cleared all the same.  Pair 2 turns once in 41 windows and has ddphi != 0: a word stays in its register over several windows.
  * Calls of 1, 8, 9, 30 and 7 windows: less than a batch, exactly one, one and a tail of 1, three and a tail of 6, a tail of 7.
  * nbin 5, 64 (one bin tile, full) and 100 (two bin tiles, the second with 36 bins).
  * Dumps: nfscr 1 (gpw = 32: three channel blocks, the last with 6 groups), normalising, not clearing, after 9 windows; nfscr 7
    (four groups and 28 channels a work-group, three blocks, the last with 2 groups), plain; nfscr 35 (two chunks of 32 + 3),
    normalising and clearing; nfscr 70 (three chunks, 32 + 32 + 6), plain; then the Reset, the same calls on other data, and
    nfscr 70 normalising and clearing followed by nfscr 7 normalising on the cleared profile (every bin has 0 hits: all +0).
  * Non-zero rotations in every channel of pairs 0 and 2; an eighth of the weights is 0 and those channels hold NaN and +Inf."""
import os

import numpy as np
import pytest

from tests import emul_build
from tests.fold_ref import FoldRef

EMUL = os.path.join(emul_build.ROOT, "tests", "fold_emul")
NPAIR, NFINE, NWIN = 3, 70, 30
CALLS = [1, 8, 9, 30, 7]
RUN, DUMP, RESET = 0, 1, 2


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("fold_emul")
    return emul_build.build_both(d, EMUL, [emul_build.CSRC]), str(d)


def operations():
    half = [(RUN, 1), (RUN, 8), (DUMP, 1, 1, 0), (RUN, 9), (DUMP, 7, 0, 0), (RUN, 30)]
    return half + [(DUMP, 35, 1, 1), (RUN, 7), (DUMP, 70, 0, 0), (RESET,)] + half + [(RUN, 7), (DUMP, 70, 1, 1), (DUMP, 7, 1, 0)]


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("nbin", [5, 64, 100])
def test_kernels_on_host_threads_equal_the_ordered_restatement(drivers, nbin, nprod):
    exes, d = drivers
    rng = np.random.default_rng(1000 * nbin + nprod)
    ops = operations()
    total = sum(o[1] for o in ops if o[0] == RUN)
    assert [o[1] for o in ops if o[0] == RUN] == CALLS * 2
    x = rng.chisquare(4, (total, NPAIR, NFINE, 4)).astype(np.float32)
    x[..., 2:] = rng.standard_normal((total, NPAIR, NFINE, 2)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, NFINE).astype(np.float32)
    off = rng.choice(NFINE, 9, replace=False)
    w[off] = 0
    x[::3, :, off[:5]] = np.nan
    x[1::4, :, off[5:], :2] = np.inf
    rot = rng.integers(1, nbin, (NPAIR, NFINE)).astype(np.int32)
    rot[1] = 0
    phi0 = [int(rng.integers(0, 1 << 63)) for _ in range(NPAIR)]
    dphi = [int(2 ** 64 / 3.3), int(2 ** 64 / 5.0), int(2 ** 64 / 41.0)]
    ddphi = [0, 0, -(1 << 51)]
    active = [1, 0, 1]
    osc = np.zeros(NPAIR, np.dtype([('phi0', '<u8'), ('dphi', '<u8'), ('ddphi', '<i8'), ('active', '<u4'), ('pad', '<u4')]))
    osc['phi0'], osc['dphi'], osc['ddphi'], osc['active'] = phi0, dphi, ddphi, active
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([NPAIR, NFINE, NWIN, nbin, nprod, len(ops)], np.int32).tobytes() + osc.tobytes() + rot.tobytes() + w.tobytes())
        f.write(np.array([list(o) + [0] * (4 - len(o)) for o in ops], np.int32).tobytes() + x.tobytes())
    ref = FoldRef(NPAIR, NFINE, nbin, nprod)
    ref.set_phase(phi0, dphi, ddphi, active, 0)
    ref.set_rotations(rot)
    ref.set_weights(w)
    n, dumps = 0, []
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        for o in ops:
            if o[0] == RUN:
                ref.run(x[n:n + o[1]])
                n += o[1]
                f.write(ref.prof.tobytes())
            elif o[0] == DUMP:
                out, hits = ref.dump(o[1], bool(o[2]), bool(o[3]))
                f.write(out.tobytes() + hits.astype(np.uint32).tobytes() + ref.prof.tobytes())
                dumps.append((o, out, hits))
            else:
                ref.reset()
    for name in sorted(exes):
        assert int(emul_build.run(exes[name], os.path.join(d, "in.bin"), os.path.join(d, "exp.bin"))) == len(dumps)
    # what the list of operations is there to reach
    (_, _, h0), (_, plain, _), (_, _, h35) = dumps[:3]
    assert h0[0].sum() == h0[2].sum() == 9 and not h0[1].any() and h35[0].sum() == 48
    if nbin > 9:
        assert (h0[[0, 2]] == 0).any(axis=1).all()                  # (a normalising dump over bins with 0 hits)
    else:
        assert h0[0].max() > 1                                      # (bins repeat inside the first batch)
    for _, out, _ in dumps:
        assert np.isfinite(out).all() and not out[1].any()          # (NaN and Inf stay in their zero-weight channels; the inactive pair)
    assert plain[0].any() and plain[2].any() and not dumps[-1][1].any() and dumps[-2][1][0].any()
    assert not ref.prof.any() and not dumps[-1][2].any()
