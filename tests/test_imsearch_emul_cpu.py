"""imsearch_ingest_kernel and imsearch_search_kernel without a GPU: the kernels' own source (csrc/imsearch_kernels.h) compiled as host
C++ against a stand-in for <hip/hip_runtime.h> (tests/imsearch_emul/) and run by a stand-alone driver, the search kernel's work-group
as 256 host threads with its barrier, under the address sanitizer.  What this can show is the kernels' logic -- which rows and
slots a lane reads, the ring wraps, what is left out by index, the chunked group loop, the boxcar tree in blocks, the keys and the
meeting of the four waves, ragged rows taken word by word -- and that no access leaves its buffer; not their arithmetic on the GPU.

The planes and the baseline are compared word for word with the float32 restatement (tests/imsearch_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests.imsearch_ref import RECORD, imsearch, integer_case, planted_case, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "imsearch_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "imsearch_kernels.h")
LDS_LINE = "__shared__ float4 is_red[(IS_WAVES - 1) * 2 * 64];"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("imsearch_emul")
    src = open(KERNELS).read()
    assert src.count(LDS_LINE) == 1
    with open(os.path.join(d, "imsearch_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float4* is_red = (float4*)g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", str(d),
                           "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, images, delays, w0, nwidth, nstat, w1=None, n_set=-1):
    exe, d = driver
    nint, ngroup, _, npix = images.shape
    ndm = delays.shape[0]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.ascontiguousarray(delays, np.int32).tobytes())
        f.write(np.ascontiguousarray(w0, np.float32).tobytes())
        f.write(np.ascontiguousarray(w0 if w1 is None else w1, np.float32).tobytes())
        f.write(np.ascontiguousarray(images, np.float32).tobytes())
    subprocess.check_call([exe] + [str(int(x)) for x in (npix, ngroup, ndm, nwidth, nstat, nint, n_set)] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = open(os.path.join(d, "out.bin"), "rb").read()
    planes = np.frombuffer(raw[:nint * npix * 8], RECORD).reshape(nint, npix)
    base = np.frombuffer(raw[nint * npix * 8:], np.float32).reshape(3, ngroup, npix)
    return planes, base


def check(planes, base, ref):
    for n in range(planes.shape[0]):
        assert planes[n].tobytes() == records(ref, n).tobytes(), n
    for got, name in zip(base, "cmv"):
        assert got.tobytes() == ref[name][-1].astype(np.float32).tobytes(), name


def test_planted_integer_case_word_for_word(driver):
    """The issue's integer case (npix 70: the last lane's row is ragged, the rows of the image are not 16-byte aligned): every plane
    and the last block's c, m, v are the float32 restatement's, and the planted pulse is the best record of its plane."""
    x, delays, w, (n, pix, idm, iw) = planted_case()
    planes, base = run(driver, x, delays, w, 3, 16)
    check(planes, base, imsearch(x, delays, w, 16, 3, np.float32))
    assert (planes[n]['idm'][pix], planes[n]['iw'][pix]) == (idm, iw) and planes[n]['snr'].argmax() == pix
    assert (planes[:16 + 12]['idm'] == -1).all() and (planes[16 + 12:]['idm'] >= 0).any()


def test_ragged_case_and_weights_set_mid_run(driver):
    """npix 37 (37 % 4 != 0), ndm 5 (a wave with two trials, three with one), 9 groups (more than one chunk of loads), weights set
    again after 40 integrations: word for word, and no boxcar reaches before the setting."""
    x, delays = integer_case(37, 9, 5, 64, seed=3)
    w0 = np.array([1, 2, 1, 0, 1, 1, 3, 1, 1], np.float32)
    w1 = np.array([1, 1, 0, 1, 2, 1, 1, 0, 1], np.float32)
    planes, base = run(driver, x, delays, w0, 3, 16, w1, 40)
    ref = imsearch(x, delays, [(0, w0), (40, w1)], 16, 3, np.float32)
    check(planes, base, ref)
    assert planes[40]['iw'].max() == 0 and planes[41]['iw'].max() <= 1 and planes[42]['iw'].max() <= 1 and (planes[40]['idm'] >= 0).all()


def test_aligned_rows_give_the_same_words(driver):
    """npix 72 takes the 16-byte path in the image and the state; its first 70 pixels are the planted case's: the same records."""
    x, delays, w, _ = planted_case()
    x72 = np.concatenate([x, x[..., :2]], axis=-1)
    p70, b70 = run(driver, x, delays, w, 3, 16)
    p72, b72 = run(driver, x72, delays, w, 3, 16)
    assert p72[:, :70].tobytes() == p70.tobytes() and b72[..., :70].tobytes() == b70.tobytes()
    assert p72[:, 70:].tobytes() == p70[:, :2].tobytes()


def test_two_tiles_and_seven_trials(driver):
    """npix 300 (two tiles, the second with idle lanes), ndm 7 (waves with two trials and with one), one width: word for word."""
    x, delays = integer_case(300, 5, 7, 40, seed=4)
    w = np.array([1, 1, 0, 2, 1], np.float32)
    planes, base = run(driver, x, delays, w, 1, 16)
    check(planes, base, imsearch(x, delays, w, 16, 1, np.float32))
    planes, base = run(driver, x[:, :, :, :37], delays[:1], w, 3, 16)
    check(planes, base, imsearch(x[:, :, :, :37], delays[:1], w, 16, 3, np.float32))


@pytest.mark.parametrize("nwidth,nstat", [(5, 16), (6, 32)])
def test_wide_boxcars_and_three_chunks_of_groups(driver, nwidth, nstat):
    """5 and 6 widths (the tree's blocks of 8 and 16 earlier sums) over 17 groups in use of 19 (three chunks of loads), npix 9, 3 trials,
    the weights set again mid-run: word for word."""
    x, delays = integer_case(9, 19, 3, 5 * nstat, seed=6)
    w0 = np.ones(19, np.float32)
    w0[[4, 11]] = 0
    w1 = w0.copy()
    w1[[0, 4]] = [2, 1]
    planes, base = run(driver, x, delays, w0, nwidth, nstat, w1, 3 * nstat + 5)
    check(planes, base, imsearch(x, delays, [(0, w0), (3 * nstat + 5, w1)], nstat, nwidth, np.float32))
    assert planes[-1]['iw'].max() == nwidth - 1 or planes['iw'].max() == nwidth - 1
