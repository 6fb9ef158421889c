"""peel_solve_kernel and peel_subtract_kernel without a GPU: the kernels' own source (csrc/peel_kernels.h) compiled as host C++
against a stand-in for <hip/hip_runtime.h> (tests/peel_emul/) and run by a stand-alone driver as host threads -- 256 per work-group
of the solve, 64 of the subtraction -- barriers, lane exchanges and the operand layouts of both MFMA shapes included, under the
address sanitizer.  What this can show is the kernels' logic -- the LDS tables and their pitch, the operand layouts and the
conjugation by operand signs, the column tiles shared among the waves, the selects on the loads, ragged tiles, the chain over the
directions and its reductions, the uniform exit, the warm start, the tile pairs, the mirrored image -- and that no access leaves its
buffer; not their arithmetic on the GPU (sincospif is double precision here).

The bars are those of tests/test_peel_gpu.py: five times the complex64-to-float64 gap of the restatement on the test's own inputs,
for the gains per (channel, pol, direction) as max_s |g - g_ref| / rms_s |g_ref|, for the output per (channel, pol) as max |out -
out_ref| / rms |V|.  Measured here, worst error / bar (gains, output): 0.15, 0.30 (22 stands, 1 direction), 0.42, 0.19 (35, 3), 0.12, 0.20 (64, 8)."""
import os
import subprocess

import numpy as np
import pytest

from tests.calapply_ref import hermitian_bits
from tests.peel_ref import case, dir_gain_error, float_gap, hermitian_nan, out_error, peel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "peel_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "peel_kernels.h")
SWAPS = (("typedef float pl_f32x4 __attribute__((ext_vector_type(4)));", "typedef f4v pl_f32x4;"),
         ("typedef float pl_f32x16 __attribute__((ext_vector_type(16)));", "typedef f16v pl_f32x16;"),
         ("extern __shared__ __attribute__((aligned(16))) uint8_t pl_lds[];", "uint8_t* pl_lds = g_lds;"),
         ("__shared__ __attribute__((aligned(16))) float2 ps_lds[2 * PS_T * PS_PITCH];", "float2* ps_lds = (float2*)g_lds2;"))
NITER = 8       # (enough for every path of the loop: four averages; host threads are slow)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("peel_emul")
    src = open(KERNELS).read()
    for old, new in SWAPS:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    with open(os.path.join(d, "peel_kernels_host.h"), "w") as f:
        f.write("#include <hip/hip_runtime.h>\nextern uint8_t* g_lds2;\n" + src)
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", str(d),
                           "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, V, freq, tau, flux, w, refant, niter, tol, passes=1):
    exe, d = driver
    ndir, nstand = tau.shape
    nfine = len(freq)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        for a, t in ((V, np.complex64), (freq, np.float64), (tau, np.float64), (flux, np.float32), (w, np.float32)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    subprocess.check_call([exe] + [str(v) for v in (nstand, nfine, ndir, niter, repr(float(tol)), refant, passes)] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    nv, ng = nfine * (2 * nstand) ** 2 * 8, nfine * 2 * ndir * nstand * 8
    return (raw[:nv].view(np.complex64).reshape(nfine, nstand, 2, nstand, 2), raw[nv:nv + ng].view(np.complex64).reshape(nfine, 2, ndir, nstand),
            raw[nv + ng:].view(np.float32).reshape(nfine, 2, 4))


@pytest.mark.parametrize("nstand,ndir,nfine", [(22, 1, 3), (35, 3, 2), (64, 8, 2)])
def test_kernel_source_on_host_threads(driver, nstand, ndir, nfine):
    """Noisy inputs, stand 3 flagged and holding NaN and Inf: finite gains within the bar of the float64 restatement of the clean
    matrix after NITER sweeps, the flagged stand's gains 0, the stats the restatement's; the output within its bar, every word
    written, Hermitian bit for bit, the flagged stand's rows and the cross hands bit-equal to the input; the last channel alone
    gives the same words bit for bit."""
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, noise=0.02)
    bad = hermitian_nan(V, 3)
    ref = peel(V, freq, tau, flux, w, 0, NITER, 0.0)
    ggap, ogap = float_gap(V, freq, tau, flux, w, 0, NITER, ref=ref)
    out, got, stats = run(driver, bad, freq, tau, flux, w, 0, NITER, 0.0)
    gerr = dir_gain_error(got, ref[1])
    keep = np.ones(nstand, bool)
    keep[3] = False
    oerr = out_error(out[:, keep][:, :, :, keep], ref[0][:, keep][:, :, :, keep], V[:, keep][:, :, :, keep])
    print("%d stands %d directions: gaps %.2e %.2e, emulated kernels %.2e = %.2f of the bar (gains), %.2e = %.2f of the bar (output)"
          % (nstand, ndir, ggap, ogap, gerr.max(), gerr.max() / (5 * ggap), oerr.max(), oerr.max() / (5 * ogap)))
    assert np.isfinite(got.view(np.float32)).all() and np.isfinite(stats).all() and (gerr <= 5 * ggap).all(), gerr.max()
    assert (got[:, :, :, 3] == 0).all() and (got[:, :, :, 0].real > 0).all() and (np.abs(got[:, :, :, 0].imag) <= 2.0 ** -22 * got[:, :, :, 0].real).all()
    assert np.array_equal(stats[:, :, [0, 2, 3]], ref[2][:, :, [0, 2, 3]]) and (np.abs(stats[:, :, 1] - ref[2][:, :, 1]) <= 10 * ggap).all()
    assert (oerr <= 5 * ogap).all(), oerr.max()
    assert hermitian_bits(out)
    assert out[:, 3].tobytes() == bad[:, 3].tobytes() and np.ascontiguousarray(out[:, :, :, 3]).tobytes() == np.ascontiguousarray(bad[:, :, :, 3]).tobytes()
    for p in range(2):
        assert np.ascontiguousarray(out[:, :, p, :, 1 - p]).tobytes() == np.ascontiguousarray(bad[:, :, p, :, 1 - p]).tobytes()
    sub = run(driver, bad[-1:], freq[-1:], tau, flux[-1:], w, 0, NITER, 0.0)
    assert sub[0].tobytes() == out[-1:].tobytes() and sub[1].tobytes() == got[-1:].tobytes() and sub[2].tobytes() == stats[-1:].tobytes()


def test_early_exit_warm_start_and_a_direction_that_is_off(driver):
    """22 stands, 3 directions of which the middle one has flux 0 in channel 1, tol 1e-4: the sweep counts and converged flags are
    the float64 restatement's (which the complex64 one shares, checked here); the direction that is off has gains of 0; a second,
    warm pass over the same matrix stops at its first test, sweep 2."""
    nstand, ndir, nfine, tol = 22, 3, 2, 1e-4
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, seed=17)
    flux = flux.copy()
    flux[1, 1] = 0
    ref = peel(V, freq, tau, flux, w, 5, 60, tol)
    r32 = peel(V, freq, tau, flux, w, 5, 60, tol, np.complex64)
    assert np.array_equal(ref[2][:, :, [0, 3]], r32[2][:, :, [0, 3]]) and (ref[2][:, :, 3] == 1).all()
    out, got, stats = run(driver, V, freq, tau, flux, w, 5, 60, tol)
    assert np.array_equal(stats[:, :, [0, 2, 3]], ref[2][:, :, [0, 2, 3]]) and (got[1, :, 1] == 0).all() and (got[0, :, 1, 0] != 0).all()
    ggap, ogap = float_gap(V, freq, tau, flux, w, 5, 60, tol, ref=ref)
    assert (dir_gain_error(got, ref[1]) <= 5 * ggap).all() and (out_error(out, ref[0], V) <= 5 * ogap).all()
    wout, warm, wstats = run(driver, V, freq, tau, flux, w, 5, 60, tol, passes=2)
    assert (wstats[:, :, 0] == 2).all() and (wstats[:, :, 3] == 1).all() and (dir_gain_error(warm, ref[1]) <= 1e-3).all()
