"""predict_kernel without a GPU: the kernel's own source (csrc/predict_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/predict_emul/) and run by a stand-alone driver as one wave of 64 host threads per work-group, barriers and
the MFMA's operand layout included, under the address sanitizer.  What this can show is the kernel's logic -- the tile pairs and
their decoding, which record and which stand a lane steers, the operand layout and signs of the four products, ragged tiles of
stands, odd and empty records, the loop's bound, the mirrored image and its masks on the diagonal tiles -- and that no access leaves
its buffer; not its arithmetic on the GPU (sincospif is double precision here).

The output is compared bit for bit with the float32 restatement in the kernel's order (tests/predict_ref.py, libm = True: the same
sine and cosine), and against the float64 restatement with the bar of tests/test_predict_gpu.py: five times the float32-to-float64
gap of the restatement on the test's own inputs, per word against max|V| + sum_k (|C_XX| + |C_YY| + 2 |C_XY|).  Measured here, worst
word / bar, subtract mode with cross = 1: 0.20 (22 stands, 1 record), 0.16 (35, 3), 0.22 (64, 32), 0.21 (70, 5), 0.20 (40, 17); over cross 0, 1 and both modes 0.09 to 0.22."""
import os
import subprocess

import numpy as np
import pytest

from tests.calapply_ref import hermitian_bits
from tests.predict_ref import MODEL, SUBTRACT, case, float_gap, integer_case, predict, records, scale, upper_nan, word_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "predict_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "predict_kernels.h")
VEC_LINE = "typedef float pr_f32x16 __attribute__((ext_vector_type(16)));"
LDS_LINE = "__shared__ __attribute__((aligned(16))) float2 pr_lds[2 * PR_T * PR_PITCH];"
SHAPES = [(22, 1, 2, 1), (35, 3, 4, 2), (64, 32, 2, 1), (70, 5, 3, 3), (40, 17, 2, 1)]      # (nstand, ncomp, nfine, nfavg), tests/test_predict_gpu.py's


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("predict_emul")
    src = open(KERNELS).read()
    assert src.count(VEC_LINE) == 1 and src.count(LDS_LINE) == 1
    with open(os.path.join(d, "predict_kernels_host.h"), "w") as f:
        f.write(src.replace(VEC_LINE, "typedef f16v pr_f32x16;").replace(LDS_LINE, "float2* pr_lds = (float2*)g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", str(d),
                           "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, V, freq, tau, comps, nfavg, cross, mode):
    exe, d = driver
    ndir, nstand = tau.shape
    nfine = len(freq)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.ascontiguousarray(freq, np.float64).tobytes())
        f.write(np.ascontiguousarray(tau, np.float64).tobytes())
        f.write(np.ascontiguousarray(comps).tobytes())
        if mode != MODEL:
            f.write(np.ascontiguousarray(V, np.complex64).tobytes())
    subprocess.check_call([exe] + [str(int(x)) for x in (nstand, nfine, nfavg, ndir, comps.shape[1], cross, mode)] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    return np.fromfile(os.path.join(d, "out.bin"), np.complex64).reshape(nfine, nstand, 2, nstand, 2)


@pytest.mark.parametrize("nstand,ncomp,nfine,nfavg", SHAPES)
def test_kernel_source_on_host_threads(driver, nstand, ncomp, nfine, nfavg):
    """Components of either sign on all four words, empty records holding NaN, a repeated pixel, the upper triangle NaN; cross 0 and
    1, both modes: every word is the kernel-order restatement's bit for bit, within the bar of the float64 one, written, and the
    output Hermitian bit for bit; the last group alone gives the same words bit for bit."""
    tau, freq, comps, V = case(nstand, ncomp, nfine, nfavg)
    bad = upper_nan(V)
    for cross in (1, 0):
        for mode in (SUBTRACT, MODEL):
            ref = predict(V, freq, tau, comps, nfavg, cross, mode)
            gap = float_gap(V, freq, tau, comps, nfavg, cross, mode, ref=ref)
            got = run(driver, bad, freq, tau, comps, nfavg, cross, mode)
            err = word_error(got, ref, scale(None if mode == MODEL else V, comps, nfavg))
            print("%d stands %d records cross %d mode %d: float32 gap %.2e, bar %.2e, emulated kernel %.2e = %.2f of the bar"
                  % (nstand, ncomp, cross, mode, gap, 5 * gap, err.max(), err.max() / (5 * gap)))
            assert np.isfinite(got.view(np.float32)).all() and (err <= 5 * gap).all(), err.max()
            assert got.tobytes() == predict(V, freq, tau, comps, nfavg, cross, mode, np.complex64, libm=True).tobytes()
            assert hermitian_bits(got)
            if cross and mode == SUBTRACT:
                sub = run(driver, bad[-nfavg:], freq[-nfavg:], tau, comps[-1:], nfavg, cross, mode)
                assert sub.tobytes() == got[-nfavg:].tobytes()


def test_no_filled_record_copies_the_lower_triangle(driver):
    """Every record empty, the input's upper triangle NaN: the lower triangle is the input bit for bit, the upper its conjugate, the
    diagonal's imaginary parts +0 -- 70 stands: three tiles a side, the last ragged."""
    tau, freq, comps, V = case(70, 2, 1, 1)
    n = 140
    got = run(driver, upper_nan(V), freq, tau, records(1, 3), 1, 1, SUBTRACT).reshape(1, n, n)
    A = V.reshape(1, n, n)
    low = np.tril(np.ones((n, n), bool), -1)
    assert got[:, low].tobytes() == A[:, low].tobytes()
    assert got.transpose(0, 2, 1)[:, low].tobytes() == np.conj(A[:, low]).tobytes()
    d = np.einsum('cii->ci', got)
    assert d.real.tobytes() == np.einsum('cii->ci', A).real.tobytes() and (np.ascontiguousarray(d.imag).view(np.uint32) == 0).all()


def test_small_integers_with_unit_steering_are_exact(driver):
    """Gaussian-integer V, tau = 0 (a = 1), integer components of either sign: every product reads V - sum C exactly; with cross =
    0 the cross-hand words are the input's bit for bit -- 35 stands and 5 records: two tiles, an odd record count, ncomp_max 7."""
    nstand, ncomp, nfine, nfavg = 35, 5, 2, 1
    V, comps, exp = integer_case(nstand, ncomp, nfine, nfavg, 7)
    freq = 50e6 + 12e3 * np.arange(nfine)
    tau = np.zeros((4, nstand))
    got = run(driver, upper_nan(V), freq, tau, comps, nfavg, 1, SUBTRACT)
    assert np.array_equal(got, exp) and hermitian_bits(got)
    got0 = run(driver, upper_nan(V), freq, tau, comps, nfavg, 0, SUBTRACT)
    for p in range(2):
        assert np.array_equal(got0[:, :, p, :, p], exp[:, :, p, :, p])
    n = 2 * nstand
    low = np.tril(np.ones((n, n), bool), -1)[None] & np.tile(np.array([[False, True], [True, False]]), (nstand, nstand))[None]
    assert got0.reshape(nfine, n, n)[np.broadcast_to(low, (nfine, n, n))].tobytes() == V.reshape(nfine, n, n)[np.broadcast_to(low, (nfine, n, n))].tobytes()
