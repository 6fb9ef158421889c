"""image_kernel without a GPU: the kernel's own source (csrc/image_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/image_emul/) and run as 256 host threads per work-group, barriers, lane exchanges and the MFMA's operand
layout included, under the address sanitizer.  What this can show is the kernel's logic -- the steering tile and its pitch, the
operand layouts, the column tiles shared among the waves, the selects on the loads, partial tiles of stands and pixels, the
reduction -- and that no access leaves its buffer; not its arithmetic on the GPU (sincospif is double precision here).

The bar is the float bar of tests/test_image_gpu.py: five times the complex64-to-float64 gap of the restatement on the test's own
inputs.  Measured here: 0.07 of the bar (22 stands, 37 pixels), 0.02 (35 stands, 1 pixel), 0.03 (64 stands, 64 pixels)."""
import os
import subprocess

import numpy as np
import pytest

from caltech_bifrost_dsp_amd.blocks import image_norm, steering_delays
from tests.image_ref import float_gap, hermitian_uneven, random_array, word_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "image_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "image_kernels.h")
VEC_LINE = "typedef float img_f32x16 __attribute__((ext_vector_type(16)));"
LDS_LINE = "extern __shared__ __attribute__((aligned(16))) uint8_t img_lds[];"
FINE_BW = 23925.78125 / 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("image_emul")
    src = open(KERNELS).read()
    assert src.count(VEC_LINE) == 1 and src.count(LDS_LINE) == 1
    with open(os.path.join(d, "image_kernels_host.h"), "w") as f:
        f.write(src.replace(VEC_LINE, "typedef f16v img_f32x16;").replace(LDS_LINE, "uint8_t* img_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", str(d),
                           "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, V, freq, tau, w, autos, nfavg):
    exe, d = driver
    npix, nstand = tau.shape
    with open(os.path.join(d, "in.bin"), "wb") as f:
        for a, t in ((V, np.complex64), (freq, np.float64), (tau, np.float64), (w, np.float32)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    norm = repr(float(np.float32(image_norm(w, autos, nfavg))))
    subprocess.check_call([exe] + [str(v) for v in (nstand, len(freq), nfavg, npix, int(autos), norm)] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    return np.fromfile(os.path.join(d, "out.bin"), np.float32).reshape(len(freq) // nfavg, 4, npix)


def _setup(seed, nstand, npix, nfine):
    rng = np.random.default_rng(seed)
    lm = rng.uniform(-0.65, 0.65, (npix, 2))
    lmn = np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)
    tau = steering_delays(random_array(rng, nstand, 1200.0, 5.0), lmn)
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[3] = 0
    return rng, tau, 50e6 + FINE_BW * np.arange(nfine), w


@pytest.mark.parametrize("nstand,npix,nfine,nfavg,autos", [(22, 37, 4, 1, False), (35, 1, 4, 2, True), (64, 64, 2, 2, False)])
def test_kernel_source_on_host_threads(driver, nstand, npix, nfine, nfavg, autos):
    """The GPU parity test's shapes, stand 3 flagged and holding NaN and Inf: finite, every word within the bar of the float64
    restatement of the clean matrix; for 37 pixels, every third pixel and the last one alone give the same words bit for bit."""
    rng, tau, freq, w = _setup(100 + nstand, nstand, npix, nfine)
    V = hermitian_uneven(rng, nfine, nstand)
    bad = V.copy()
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    gap = float_gap(V, freq, tau, w, autos, nfavg)
    got = run(driver, bad, freq, tau, w, autos, nfavg)
    err = word_error(got, V, freq, tau, w, autos, nfavg)
    print("%d stands %d pixels: complex64 gap %.2e, bar %.2e, emulated kernel %.2e" % (nstand, npix, gap, 5 * gap, err.max()))
    assert np.isfinite(got).all() and (err <= 5 * gap).all(), err.max()
    if npix == 37:
        for sel in (slice(None, None, 3), slice(npix - 1, None)):
            sub = run(driver, bad, freq, np.ascontiguousarray(tau[sel]), w, autos, nfavg)
            assert sub.tobytes() == np.ascontiguousarray(got[:, :, sel]).tobytes()


@pytest.mark.parametrize("autos", [False, True])
def test_small_integers_with_unit_steering_are_exact(driver, autos):
    """tau = 0, small integers, w in {0, 1, 2}: float32(S) * float32(norm) with S the int64 sum, bit for bit (35 stands, 33 pixels)."""
    nstand, npix, nfine, nfavg = 35, 33, 4, 2
    rng = np.random.default_rng(211 + autos)
    w = rng.integers(0, 3, nstand)
    w[:3] = (1, 2, 0)
    re = rng.integers(-7, 8, (nfine, nstand, 2, nstand, 2))
    iv = rng.integers(-7, 8, (nfine, nstand, 2, nstand, 2))
    keep = (w != 0)[:, None] & (w != 0)[None, :] & (autos | ~np.eye(nstand, dtype=bool))
    S = np.zeros((nfine, 4), np.int64)
    for k, (part, p, q) in enumerate(((re, 0, 0), (re, 1, 1), (re, 0, 1), (iv, 0, 1))):
        S[:, k] = np.einsum('s,cst,t->c', w, np.where(keep[None], part[:, :, p, :, q], 0), w)
    S = S.reshape(nfine // nfavg, nfavg, 4).sum(axis=1)
    exp = S.astype(np.float32) * np.float32(image_norm(w, autos, nfavg))
    got = run(driver, re + 1j * iv, 50e6 + FINE_BW * np.arange(nfine), np.zeros((npix, nstand)), w.astype(np.float32), autos, nfavg)
    assert np.array_equal(got, np.broadcast_to(exp[:, :, None], got.shape))
