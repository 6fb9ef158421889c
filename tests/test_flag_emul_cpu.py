"""The flag kernels without a GPU: the kernels' own source (csrc/flag_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/flag_emul/) and run by a stand-alone driver, a work-group as that many host threads with its barriers,
under the address sanitizer.  What this can show is the kernels' logic -- the tile pairs and their decoding, the rows a lane takes,
the selects on the loads, ragged tiles, the mirrored half of a diagonal tile and the auto split off it, the partials and the order
they are added in, the selection of the medians for even and odd counts, the window of the channel test -- and that no access
leaves its buffer; not their arithmetic on the GPU, though every operation here is one IEEE float32 operation there and here.

The statistics are compared bit for bit with the restatement in the kernel's summation order (tests/flag_ref.py
statistics_kernel_order), the mask and chan bit for bit with the float32 restatement of steps 2 and 3 on the driver's own table."""
import os
import subprocess

import numpy as np
import pytest

from tests import flag_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "flag_emul")
CSRC = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc")
SHAPES = [(22, 3), (35, 2), (64, 2), (70, 5)]       # (nstand, nfine): one ragged tile, two, two full ones, three with the last ragged


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("flag_emul")
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", EMUL, "-I", CSRC,
                           os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, V, w, k=None, wchan=0):
    exe, d = driver
    nfine, nstand = V.shape[:2]
    k = fr.thresholds() if k is None else k
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.ascontiguousarray(V, np.complex64).tobytes())
        f.write(np.ascontiguousarray(w, np.float32).tobytes())
        f.write(np.asarray(k, np.float32).tobytes())
    subprocess.check_call([exe, str(nstand), str(nfine), str(wchan), os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    n = nfine * 2 * nstand
    return (raw[:n].reshape(nfine, 2, nstand), raw[n:9 * n].view(np.float32).reshape(nfine, 2, nstand, 2),
            raw[9 * n:].view(np.float32).reshape(nfine, 2, 4))


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("nstand,nfine", SHAPES)
def test_kernel_source_on_host_threads(driver, nstand, nfine):
    """Stand 3 of weight 0 and full of NaN, the upper triangle and the cross hands NaN, stand 7 eight times too loud in channel 1:
    R and A are the kernel-order restatement bit for bit (the ragged tiles, the diagonal tile's mirror, the partials in ascending
    tile order), +0 at stand 3; mask and chan are the restatement of steps 2 and 3 on that table; the last channel alone gives the
    same statistics and stand bits."""
    V = fr.case(nstand, nfine)
    fr.scale_stand(V, 1, 7, 8)
    w = np.ones(nstand, np.float32)
    w[3] = 0
    bad = fr.upper_and_cross_nan(V)
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    mask, stats, chan = run(driver, bad, w)
    R, A = fr.statistics_kernel_order(V, w)
    assert _same(stats[..., 0], R) and _same(stats[..., 1], A)
    assert (stats[:, :, 3].view(np.uint32) == 0).all()
    ref = fr.statistics(V, w)
    gap = fr.float_gap(V, w, ref)
    err = fr.stat_error(stats[..., 0], ref[0], w)
    print("%d stands: R's float32 gap %.2e, emulated kernel %.2e, worst error / bar %.2f" % (nstand, gap[0].max(), err.max(), (err / (5 * gap[0])).max()))
    assert (err <= 5 * gap[0]).all()
    emask, echan = fr.flags(stats, w, *fr.thresholds(), 0)
    assert _same(mask, emask) and _same(chan, echan)
    assert (mask[1, :, 7] & 3 == 3).all() and (mask[:, :, 3] & 16 == 16).all() and chan[0, 0, 3] == nstand - 1
    m1, s1, _ = run(driver, bad[-1:], w)
    assert _same(s1, stats[-1:]) and _same(m1 & 0x1b, mask[-1:] & 0x1b)


@pytest.mark.parametrize("live", [22, 21, 5, 4])
def test_medians_for_even_and_odd_counts(driver, live):
    """22 stands of which `live` have weight > 0 -- even and odd counts, down to the least for which the stand tests are taken --
    with ties in the table (two stands share every word): the medians, the MADs and the flags are the restatement's bit for bit."""
    V = fr.case(22, 2, seed=live)
    V[:, 11] = V[:, 10]
    V[:, :, :, 11] = V[:, :, :, 10]
    w = np.zeros(22, np.float32)
    w[np.random.default_rng(live).permutation(22)[:live]] = 1
    for k in (fr.thresholds(), fr.thresholds(1, 1, 1), fr.thresholds(0, 3, 0)):
        mask, stats, chan = run(driver, V, w, k)
        emask, echan = fr.flags(stats, w, *k, 0)
        assert _same(mask, emask) and _same(chan, echan)
        assert (chan[:, :, 3] == live).all()


def test_fewer_than_four_live_stands_flag_the_channel(driver):
    """NaN words leave 3 finite stands in (channel 1, pol 0): no stand test there, bit 2 on every stand of it, no y, and the channel
    test of pol 0 runs over the other channels."""
    V = fr.case(22, 4)
    w = np.zeros(22, np.float32)
    w[:5] = 1
    V[1, 1, 0, 0, 0] = np.nan                   # stands 1 and 0
    mask, stats, chan = run(driver, V, w)
    emask, echan = fr.flags(stats, w, *fr.thresholds(), 0)
    assert _same(mask, emask) and _same(chan, echan)
    assert chan[1, 0, 3] == 3 and (mask[1, 0] & 4 == 4).all() and (mask[1, 0, :2] & 8 == 8).all() and chan[1, 1, 3] == 5
    assert (chan[1, 0, :3].view(np.uint32) == 0).all()


@pytest.mark.parametrize("wchan", [0, 1, 3])
def test_channel_window(driver, wchan):
    """12 channels, channel 4 five times too loud, channel 9 without a y in pol 1: b, bit 2 and the window's clipping at both ends are
    the restatement's bit for bit."""
    V = fr.case(22, 12)
    fr.scale_channel(V, 4, 5)
    V[9, 5:, 1, 0, 1] = np.nan                  # every stand but 1 .. 4 meets a NaN word in (9, pol 1)
    V[9, 4, 1, 1:4, 1] = np.nan
    w = np.ones(22, np.float32)
    for k in (fr.thresholds(), fr.thresholds(6, 6, 0)):
        mask, stats, chan = run(driver, V, w, k, wchan)
        emask, echan = fr.flags(stats, w, *k, wchan)
        assert _same(mask, emask) and _same(chan, echan)
    assert chan[9, 1, 3] < 4 and (mask[9, 1] & 4 == 4).all()
