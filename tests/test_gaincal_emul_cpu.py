"""gaincal_kernel without a GPU: the kernel's own source (csrc/gaincal_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/gaincal_emul/) and run by a stand-alone driver as 256 host threads per work-group, barriers, lane
exchanges and the MFMA's operand layout included, under the address sanitizer.  What this can show is the kernel's logic -- the
steering tile and its pitch, the operand layouts and the conjugation by operand signs, the column tiles shared among the waves, the
selects on the loads, partial tiles of stands and sources, the Gram route, the reductions, the uniform exit, the warm start -- and
that no access leaves its buffer; not its arithmetic on the GPU (sincospif is double precision here).

The bar is the float bar of tests/test_gaincal_gpu.py: five times the complex64-to-float64 gap of the restatement on the test's own
inputs, per (channel, pol) as max_s |g - g_ref| / rms_s |g_ref|.  Measured here: 0.23 of the bar (22 stands, 1 source), 0.14 (35
stands, 3 sources), 0.21 (64 stands, 32 sources)."""
import os
import subprocess

import numpy as np
import pytest

from tests.gaincal_ref import corrupt, float_gap, gain_error, model, noisy, setup, solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "gaincal_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "gaincal_kernels.h")
VEC_LINE = "typedef float gc_f32x16 __attribute__((ext_vector_type(16)));"
LDS_LINE = "extern __shared__ __attribute__((aligned(16))) uint8_t gc_lds[];"
NITER = 8       # (enough for every path of the loop: four averages; host threads are slow)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("gaincal_emul")
    src = open(KERNELS).read()
    assert src.count(VEC_LINE) == 1 and src.count(LDS_LINE) == 1
    with open(os.path.join(d, "gaincal_kernels_host.h"), "w") as f:
        f.write(src.replace(VEC_LINE, "typedef f16v gc_f32x16;").replace(LDS_LINE, "uint8_t* gc_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", str(d),
                           "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, V, freq, tau, flux, w, refant, niter, tol, passes=1):
    exe, d = driver
    nsrc, nstand = tau.shape
    nfine = len(freq)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        for a, t in ((V, np.complex64), (freq, np.float64), (tau, np.float64), (flux, np.float32), (w, np.float32)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    subprocess.check_call([exe] + [str(v) for v in (nstand, nfine, nsrc, niter, repr(float(tol)), refant, passes)] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    ng = nfine * 2 * nstand * 8
    return raw[:ng].view(np.complex64).reshape(nfine, 2, nstand), raw[ng:].view(np.float32).reshape(nfine, 2, 4)


@pytest.mark.parametrize("nstand,nsrc,nfine", [(22, 1, 3), (35, 3, 2), (64, 32, 2)])
def test_kernel_source_on_host_threads(driver, nstand, nsrc, nfine):
    """The GPU parity test's shapes on noisy inputs, stand 3 flagged and holding NaN and Inf: finite, every (channel, pol) within
    the bar of the float64 restatement of the clean matrix after NITER iterations, the flagged stand's gain 0, the stats those of
    the restatement; the last channel alone gives the same words bit for bit."""
    rng, tau, freq, flux, w, g = setup(100 + nstand, nstand, nsrc, nfine)
    V = noisy(rng, corrupt(model(freq, tau, flux), g), 0.02)
    bad = V.copy()
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    ref, rstats, _ = solve(V, freq, tau, flux, w, 0, NITER, 0.0)
    gap = float_gap(V, freq, tau, flux, w, 0, NITER, ref=ref)
    got, stats = run(driver, bad, freq, tau, flux, w, 0, NITER, 0.0)
    err = gain_error(got, ref)
    print("%d stands %d sources: complex64 gap %.2e, bar %.2e, emulated kernel %.2e = %.2f of the bar" % (nstand, nsrc, gap, 5 * gap, err.max(), err.max() / (5 * gap)))
    assert np.isfinite(got.view(np.float32)).all() and np.isfinite(stats).all() and (err <= 5 * gap).all(), err.max()
    # (the reference stand's imaginary part is the rounding of two products of about |g| / 2 each: four half-ulps of |g| at the most)
    assert (got[:, :, 3] == 0).all() and (np.abs(got[:, :, 0].imag) <= 2.0 ** -22 * got[:, :, 0].real).all() and (got[:, :, 0].real > 0).all()
    # (delta is a ratio of norms of gains that are each within the bar: by the triangle inequality it is within two bars)
    assert np.array_equal(stats[:, :, [0, 2, 3]], rstats[:, :, [0, 2, 3]]) and (np.abs(stats[:, :, 1] - rstats[:, :, 1]) <= 10 * gap).all()
    sub, sstats = run(driver, bad[-1:], freq[-1:], tau, flux[-1:], w, 0, NITER, 0.0)
    assert sub.tobytes() == got[-1:].tobytes() and sstats.tobytes() == stats[-1:].tobytes()


def test_early_exit_and_warm_start(driver):
    """22 stands, 3 sources, noise-free, tol 1e-4: the iteration counts and converged flags are the float64 restatement's (which the
    complex64 one shares, checked here); a second, warm pass over the same matrix stops at its first test, iteration 2."""
    nstand, nsrc, nfine, tol = 22, 3, 2, 1e-4
    rng, tau, freq, flux, w, g = setup(7, nstand, nsrc, nfine)
    V = corrupt(model(freq, tau, flux), g)
    ref, rstats, keep = solve(V, freq, tau, flux, w, 5, 60, tol)
    assert np.array_equal(rstats[:, :, [0, 3]], solve(V, freq, tau, flux, w, 5, 60, tol, np.complex64)[1][:, :, [0, 3]]) and (rstats[:, :, 3] == 1).all()
    got, stats = run(driver, V, freq, tau, flux, w, 5, 60, tol)
    assert np.array_equal(stats[:, :, [0, 2, 3]], rstats[:, :, [0, 2, 3]])
    assert (gain_error(got, ref) <= 5 * float_gap(V, freq, tau, flux, w, 5, 60, tol, ref=ref)).all()
    warm, wstats = run(driver, V, freq, tau, flux, w, 5, 60, tol, passes=2)
    assert (wstats[:, :, 0] == 2).all() and (wstats[:, :, 3] == 1).all() and (gain_error(warm, ref) <= 1e-3).all()


def test_one_source_on_small_integers_is_exact(driver):
    """tau = 0 and one source of flux 1: a = 1, so with g = 1 the first iteration is N_s = sum_{t != s} w_t X[s][t] and D_s = sum_t
    w_t - w_s, small integers for w in {0, 1, 2} and Gaussian-integer V: after one iteration and the phase reference (stand 0's N is
    made real, so the reference factor is exactly 1) the gains are float32(N) / float32(D) bit for bit -- 35 stands, two column tiles."""
    nstand, nfine = 35, 2
    rng = np.random.default_rng(211)
    w = rng.integers(0, 3, nstand)
    w[:4] = (1, 2, 0, 1)
    re = rng.integers(-7, 8, (nfine, nstand, 2, nstand, 2))
    iv = rng.integers(-7, 8, (nfine, nstand, 2, nstand, 2))
    re[:, :, :, 0, :] = np.abs(re[:, :, :, 0, :]) + 1       # X[0][t] = conj(V[t][0]): real and positive, so is N_0
    iv[:, :, :, 0, :] = 0
    V = (re + 1j * iv).astype(np.complex64)
    exp = np.zeros((nfine, 2, nstand), np.complex64)
    keep = (w != 0)[:, None] & (w != 0)[None, :] & ~np.eye(nstand, dtype=bool)
    for p in range(2):
        X = np.where(keep[None], np.conj(V[:, :, p, :, p]).transpose(0, 2, 1), 0)
        N = np.einsum('cst,t->cs', X, w)
        D = (w.sum() - w).astype(np.float32)
        exp[:, p] = np.where(w != 0, (N.real.astype(np.float32) / D) + 1j * (N.imag.astype(np.float32) / D), 0)
    got, stats = run(driver, V, 50e6 + np.arange(nfine), np.zeros((1, nstand)), np.ones((nfine, 1)), w.astype(np.float32), 0, 1, 0.0)
    assert got.tobytes() == exp.astype(np.complex64).tobytes() and (stats[:, :, 0] == 1).all() and (stats[:, :, 1] == -1).all()
