"""calapply_kernel without a GPU: the kernels' own source (csrc/calapply_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/calapply_emul/) and run by a stand-alone driver as one wave of 64 host threads per work-group, barriers
and the MFMA's operand layout included, under the address sanitizer.  What this can show is the kernel's logic -- the tile pairs and
their decoding, the model's operand layout and signs, the rows a lane takes, the selects on the loads, ragged tiles of stands and
odd source counts, the mirrored image and its masks on the diagonal tiles -- and that no access leaves its buffer; not its arithmetic
on the GPU (sincospif is double precision here).

The shapes, the bar and the assertions are those of tests/test_calapply_gpu.py: five times the complex64-to-float64 gap of the
restatement on the test's own inputs, per word against |h_i||h_j| max|V| + sum_k F_k.  Measured here, worst word / bar: 0.10 (22
stands, 1 source), 0.19 (35, 3), 0.32 (64, 32), 0.20 (70, 5), 0.20 (35, no model)."""
import os
import subprocess

import numpy as np
import pytest

from tests.calapply_ref import apply, case, float_gap, hermitian_bits, scale, word_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "calapply_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "calapply_kernels.h")
VEC_LINE = "typedef float ca_f32x16 __attribute__((ext_vector_type(16)));"
LDS_LINE = "__shared__ __attribute__((aligned(16))) float2 ca_lds[2 * CA_T * CA_PITCH];"
SHAPES = [(22, 1, 3), (35, 3, 2), (64, 32, 2), (70, 5, 1), (35, 0, 2)]      # (nstand, nsrc, nfine), tests/test_calapply_gpu.py's


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("calapply_emul")
    src = open(KERNELS).read()
    assert src.count(VEC_LINE) == 1 and src.count(LDS_LINE) == 1
    with open(os.path.join(d, "calapply_kernels_host.h"), "w") as f:
        f.write(src.replace(VEC_LINE, "typedef f16v ca_f32x16;").replace(LDS_LINE, "float2* ca_lds = (float2*)g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", str(d),
                           "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, V, h, freq, tau=None, flux=None):
    exe, d = driver
    nfine, nstand = V.shape[:2]
    nsrc = 0 if tau is None else np.shape(tau)[0]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.ascontiguousarray(V, np.complex64).tobytes())
        f.write(np.ascontiguousarray(freq, np.float64).tobytes())
        if nsrc:
            f.write(np.ascontiguousarray(tau, np.float64).tobytes())
            f.write(np.ascontiguousarray(np.broadcast_to(flux, (nfine, nsrc)), np.float32).tobytes())
        f.write(np.ascontiguousarray(h, np.complex64).tobytes())
    subprocess.check_call([exe, str(nstand), str(nfine), str(nsrc), os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    return np.fromfile(os.path.join(d, "out.bin"), np.complex64).reshape(nfine, nstand, 2, nstand, 2)


def _upper_nan(V):
    """V with every word above the diagonal replaced by NaN: nothing may read them."""
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    up = np.triu(np.ones((n, n), bool), 1)
    return np.where(up[None], np.complex64(complex(np.nan, np.nan)), V.reshape(nfine, n, n)).reshape(V.shape).astype(np.complex64)


@pytest.mark.parametrize("nstand,nsrc,nfine", SHAPES)
def test_kernel_source_on_host_threads(driver, nstand, nsrc, nfine):
    """Random gains of modulus 0.5 to 2, stand 3 flagged and holding NaN and Inf, (stand 5, pol 1) flagged, the upper triangle NaN:
    every word within the bar of the float64 restatement, every word written, the flagged rows and columns +0, the output Hermitian
    bit for bit; the last channel alone gives the same words bit for bit."""
    tau, freq, flux, h, V = case(nstand, nsrc, nfine)
    ref = apply(V, h, freq, tau, flux)
    gap = float_gap(V, h, freq, tau, flux, ref=ref)
    bad = _upper_nan(V)
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    got = run(driver, bad, h, freq, tau, flux)
    err = word_error(got, ref, scale(V, h, flux))
    print("%d stands %d sources: complex64 gap %.2e, bar %.2e, emulated kernel %.2e = %.2f of the bar" % (nstand, nsrc, gap, 5 * gap, err.max(), err.max() / (5 * gap)))
    assert np.isfinite(got.view(np.float32)).all() and (err <= 5 * gap).all(), err.max()
    assert hermitian_bits(got)
    for x in (got[:, 3], got[:, :, :, 3], got[:, 5, 1], got[:, :, :, 5, 1]):
        assert (np.ascontiguousarray(x).view(np.uint32) == 0).all()
    sub = run(driver, bad[-1:], h[-1:], freq[-1:], tau, flux[-1:])
    assert sub.tobytes() == got[-1:].tobytes()


def test_unit_factors_without_a_model_copy_the_lower_triangle(driver):
    """Unit factors, nsrc = 0, the input's upper triangle NaN: the lower triangle is the input bit for bit, the upper its conjugate,
    the diagonal's imaginary parts +0 -- 70 stands: three tiles a side, the last ragged."""
    tau, freq, flux, h, V = case(70, 0, 1)
    n = 140
    got = run(driver, _upper_nan(V), np.ones_like(h), freq).reshape(1, n, n)
    A = V.reshape(1, n, n)
    low = np.tril(np.ones((n, n), bool), -1)
    assert got[:, low].tobytes() == A[:, low].tobytes()
    assert got.transpose(0, 2, 1)[:, low].tobytes() == np.conj(A[:, low]).tobytes()
    d = np.einsum('cii->ci', got)
    assert d.real.tobytes() == np.einsum('cii->ci', A).real.tobytes() and (np.ascontiguousarray(d.imag).view(np.uint32) == 0).all()


def test_factors_that_are_powers_of_two_scale_exactly(driver):
    """h from {+-2^n, +-i 2^n}: h_i conj(h_j) V is exact in float32, so the output equals the float64 restatement exactly."""
    tau, freq, flux, h, V = case(35, 0, 2)
    rng = np.random.default_rng(5)
    h = (np.exp2(rng.integers(-3, 4, h.shape)) * (1j ** rng.integers(0, 4, h.shape))).astype(np.complex64)
    got = run(driver, _upper_nan(V), h, freq)
    assert np.array_equal(got, apply(V, h)) and hermitian_bits(got)


def test_small_integers_with_unit_steering_are_exact(driver):
    """Gaussian-integer V, tau = 0 (a = 1), integer fluxes, unit factors: the pp blocks read V - sum F exactly, the pq blocks are
    untouched -- 35 stands and 5 sources: two tiles, an odd source count."""
    nstand, nsrc, nfine = 35, 5, 2
    rng = np.random.default_rng(7)
    n = 2 * nstand
    Z = rng.integers(-50, 51, (nfine, n, n)) + 1j * rng.integers(-50, 51, (nfine, n, n))
    L = np.where(np.tril(np.ones((n, n), bool), -1)[None], Z, 0)
    Z = L + np.conj(L.transpose(0, 2, 1)) + np.einsum('ci,ij->cij', rng.integers(1, 99, (nfine, n)), np.eye(n))
    V = Z.astype(np.complex64).reshape(nfine, nstand, 2, nstand, 2)
    flux = rng.integers(0, 9, (nfine, nsrc)).astype(np.float32)
    freq = 50e6 + 12e3 * np.arange(nfine)
    got = run(driver, _upper_nan(V), np.ones((nfine, 2, nstand), np.complex64), freq, np.zeros((nsrc, nstand)), flux)
    exp = V.astype(np.complex128)
    for p in range(2):
        exp[:, :, p, :, p] -= flux.sum(axis=1)[:, None, None]
    assert np.array_equal(got, exp) and hermitian_bits(got)
    assert np.array_equal(got[:, :, 0, :, 1], V[:, :, 0, :, 1]) and np.array_equal(got[:, :, 1, :, 0], V[:, :, 1, :, 0])
