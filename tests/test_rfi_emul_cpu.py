"""The beam cleaner's kernels without a GPU: the kernels' own source (csrc/rfi_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/rfi_emul/) and run as 256 host threads per work-group in the order rfi.hip launches them.  The driver is
a program of its own, built with -fsanitize=address,undefined, and every buffer has its exact size: a word read or written outside
one -- a ring slot past the ring, a channel past the pair, a window past the call, an LDS word past the launch's -- ends the run.
After every call the driver compares out and stats, and after a call that decided a block flags, mu, V, R and gains, with the bytes
this side wrote from the restatement (tests/rfi_ref.py) and ends with a status of 4 or more unless they are equal.  What this can
show is the kernels' logic (the chains across calls, the ring, the two halves, the rank selection, the tree), not the GPU's
arithmetic.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from tests import rfi_cases, rfi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "rfi_emul")
CSRC = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc")
LDS_LINE = "extern __shared__ float rf_lds[];"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("rfi_emul")
    src = open(os.path.join(CSRC, "rfi_kernels.h")).read()
    assert src.count(LDS_LINE) == 2
    with open(os.path.join(d, "rfi_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* rf_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",      # (the runtime inside the program)
                           "-Wno-unknown-pragmas", "-I", str(d), "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, x, calls, events, nstat, nwin):
    """x [nwindows][npair][nfine][4]; events: [(the call before which they are given, (k_chan, t_clip, t_broad, min_count, zerodm),
    mask or None)].  The restatement runs the same calls and writes the expectation; the driver compares.  Returns the restatement's
    (out, stats) over the run and its block tables per decided block."""
    exe, d = driver
    _, npair, nfine, _ = x.shape
    assert sum(calls) == x.shape[0]
    ref = rfi_ref.RfiRef(npair, nfine, nstat)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([npair, nfine, nstat, nwin, len(calls), len(events)], np.int32).tobytes() + np.asarray(calls, np.int32).tobytes())
        for at, ctl, mask in events:
            m = np.zeros((nfine + 3) & ~3, np.uint8)
            if mask is not None:
                m[:nfine] = mask
            f.write(np.array([at], np.int32).tobytes() + np.array(ctl[:3], np.float32).tobytes() + np.array(ctl[3:], np.int32).tobytes() + m.tobytes())
        f.write(np.ascontiguousarray(x, np.float32).tobytes())
    outs, stats, blocks, n = [], [], [], 0
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        for ic, nc in enumerate(calls):
            for at, ctl, mask in events:
                if at == ic:
                    ref.set_control(*ctl)
                    ref.set_mask(mask)
            before = ref.nblocks
            o, s = ref.run(x[n:n + nc])
            n += nc
            f.write(o.tobytes() + s.tobytes())
            if ref.nblocks > before:
                f.write(b"".join(a.tobytes() for a in ref.block))
                blocks.append(ref.block)
            outs.append(o)
            stats.append(s)
    got = subprocess.check_output([exe, os.path.join(d, "in.bin"), os.path.join(d, "exp.bin")])
    assert int(got) == len(blocks)
    return np.concatenate(outs), np.concatenate(stats), blocks


def test_fewer_channels_than_chains_single_windows_and_a_call_that_straddles_two_blocks(driver):
    """nfine 7, one pair, blocks of 4 windows, calls of up to 3: single windows, calls ending on a block's last window, a straddling
    call; five blocks, so both halves are written three and two times and the ring of 7 slots wraps."""
    nstat, nwin = 4, 3
    x = rfi_cases.scene(1, 20, 1, 7, nstat)
    calls = [1, 3, 3, 3, 2, 3, 1, 1, 3]         # (the fourth call takes windows 7, 8, 9: block 1's last and block 2's first two)
    assert sum(calls) == 20 and sum(calls[:2]) == nstat and sum(calls[:3]) < 2 * nstat < sum(calls[:4])
    out, stats, blocks = run(driver, x, calls, [(0, rfi_cases.controls(7, min_fraction=0.3), None)], nstat, nwin)
    assert len(blocks) == 5 and (stats[:nstat, :, 2] == 4).all() and not out[:nstat].any() and (stats[nstat:, :, 2] != 4).all()
    assert blocks[0][0][0, 1] == 2 and blocks[0][0][0, 3] == 2 and blocks[1][0][0, 2] == 2         # the NaN, the constant channel, the +inf


def test_chains_of_one_and_two_channels_a_dead_pair_a_mask_and_controls_that_wait(driver):
    """nfine 300, three pairs, nwin = nstat = 16, four blocks.  Pair 2 is dead (count 0, code 1); a mask and other controls given
    mid-block before call 3 hold from the next block to be decided, block 2; the spike window carries code 2 and the
    window after it, with half the band clipped, code 1."""
    nstat = nwin = 16
    x = rfi_cases.scene(2, 64, 3, 300, nstat, dead_pair=2)
    mask = np.zeros(300, np.uint8)
    mask[[0, 17, 299]] = 1
    calls = [16, 7, 9, 5, 11, 16]
    events = [(0, rfi_cases.controls(300), None), (3, rfi_cases.controls(300, zerodm=False, min_fraction=0.2), mask)]
    out, stats, blocks = run(driver, x, calls, events, nstat, nwin)
    assert len(blocks) == 4
    assert (blocks[0][0][2] == 2).all() and (stats[nstat:, 2, 0] == 0).all() and (stats[nstat:, 2, 2] == 1).all()
    assert stats[nstat + 8, 0, 2] == 2 and stats[nstat + 9, 0, 2] == 1 and stats[nstat + 9, 0, 1] >= 140
    assert not (blocks[1][0][:, 17] & 1).any() and (blocks[2][0][:, [0, 17, 299]] & 1).all()       # the mask holds from block 2
    assert blocks[1][0][0, 5] == 4                                                                 # the noisy channel of block 1
    # zerodm: the mean over the kept channels is gone in blocks 0 and 1, not in block 2 (read 16 windows late)
    ok = stats[:, 0, 2] == 0
    z = np.abs(out[:, 0, :, 0].astype(np.float64).sum(axis=1))
    assert ok[16:48].sum() > 20 and z[16:48][ok[16:48]].max() < 1e-3 and z[48:][ok[48:]].max() > 0.5


def test_the_live_channel_count_and_the_tie_rule(driver):
    """nfine 3072 (twelve channels a chain), two pairs, blocks of 8 in calls of up to 6; then the integer scene: equal R in many
    channels, mad = 0, and every channel whose R is not the median an outlier."""
    nstat, nwin = 8, 6
    x = rfi_cases.scene(3, 18, 2, 3072, nstat)
    run(driver, x, [6, 2, 6, 4], [(0, rfi_cases.controls(3072), None)], nstat, nwin)
    xi = rfi_cases.integer_scene(12, 40)
    out, stats, blocks = run(driver, xi, [3, 3, 3, 3], [(0, rfi_cases.controls(40), None)], 4, 3)
    flags = blocks[0][0][0]
    assert (flags[np.arange(40) % 4 == 1] == 4).all() and (flags[np.arange(40) % 4 != 1] == 0).all() and (stats[4:, 0, 3] == 10).all()
