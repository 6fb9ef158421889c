"""UpchanGainCal on the MI355X: xengGaincal* against the restatement (tests/gaincal_ref.py).  Parity with the float64 restatement at
a fixed iteration count; the early exit's counts and flags; bit identity of a subset of the channels, after SetWeights back and
forth, in a fresh context, beside an X-engine contraction and xengBeamformRun, and of a warm start with niter = 0; a flagged stand
that holds NaN; a NaN in a stand that is read; warm and cold starts; the ABI with a context; Source -> UpchanCorr -> UpchanGainCal
on device rings.  The outputs sit between two poisoned 64 KiB guard bands that are checked after every call, the state's guards at
every close.  No wall-clock assertions.

The bar of the parity tests is not a constant: it is five times the worst gap between the complex64 and the float64 evaluation of
the restatement ON THE TEST'S OWN INPUTS (tests/gaincal_ref.py float_gap), per (channel, pol) as max_s |g - g_ref| / rms_s |g_ref|.
The iteration counts are those tests/test_gaincal_cpu.py measured (ITERATIONS).  Measured here on the CPU with numpy 2.2 (arrays of
1.2 km, so phases of hundreds of turns; gains of amplitude 0.5 to 2): gaps of 3.8e-7 to 9.2e-7, so bars of 1.9e-6 to 4.6e-6.
Measured on the MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import UpchanCorr, UpchanGainCal, steering_delays  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.gaincal_ref import corrupt, float_gap, gain_error, model, noisy, setup, sky, solve  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.image_ref import random_array  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_gaincal_cpu import ITERATIONS  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
# worst error / bar over test_parity_with_the_float64_restatement on the MI355X, per (nstand, nsrc, inputs)
MEASURED = {(22, 1, "clean"): 0.27, (22, 1, "noisy"): 0.20, (35, 3, "clean"): 0.26, (35, 3, "noisy"): 0.13, (64, 32, "clean"): 0.37, (64, 32, "noisy"): 0.21}
# (worst errors 5.1e-7, 4.8e-7, 5.9e-7, 3.4e-7, 1.5e-6, 9.9e-7 against gaps of 3.8e-7, 4.7e-7, 4.4e-7, 5.2e-7, 8.0e-7, 9.2e-7; the early exit's
# iteration counts are the restatement's in all 18 (channel, pol)s; a warm start takes 4 iterations where the cold start takes 10 to 20)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _info():
    l, n, t, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_int()
    ffi.call("xengGaincalGetInfo", ctypes.byref(l), ctypes.byref(n), ctypes.byref(t), ctypes.byref(r))
    return l.value, n.value, t.value, r.value


class GC:
    """The xengGaincal context (one per process), an input buffer and the outputs of one call, gains then stats, between two
    poisoned guard bands."""

    def __init__(self, tau, freq, flux, w=None, refant=0, niter=None, tol=0.0, model=True):
        self.nsrc, self.nstand = tau.shape
        self.nfine = len(freq)
        ffi.call("xengGaincalInitialize", 0, self.nstand, self.nfine, self.nsrc)
        if model:
            self.set_model(tau, freq, flux)
        if w is not None:
            self.set_weights(w, refant)
        if niter is not None:
            ffi.call("xengGaincalSetSolver", niter, tol)
        self.din = ffi.DeviceBuffer(self.nfine * (2 * self.nstand) ** 2 * 8)
        self.ngain, self.nstat = self.nfine * 2 * self.nstand * 8, self.nfine * 2 * 4 * 4
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.ngain + self.nstat)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def set_model(self, tau, freq, flux):
        ffi.call("xengGaincalSetModel", _dp(np.ascontiguousarray(tau, np.float64)), _dp(np.ascontiguousarray(freq, np.float64)),
                 _fp(np.ascontiguousarray(np.broadcast_to(flux, (self.nfine, self.nsrc)), np.float32)))

    def set_weights(self, w, refant):
        ffi.call("xengGaincalSetWeights", _fp(np.ascontiguousarray(w, np.float32)), int(refant))

    def upload(self, V):
        assert V.shape == (self.nfine, self.nstand, 2, self.nstand, 2) and V.dtype == np.complex64
        self.din.upload(np.ascontiguousarray(V))

    def enqueue(self, warm=0):
        ffi.call("xengGaincalRun", self.din.ptr, self.dout.ptr + GUARD, self.dout.ptr + GUARD + self.ngain, int(warm))

    def result(self):
        """After a sync: (gains, stats) (the poison is put back); every byte before them and past them must still be poison."""
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.ngain + self.nstat:] == POISON).all(), "bytes past the output were written"
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return (raw[GUARD:GUARD + self.ngain].copy().view(np.complex64).reshape(self.nfine, 2, self.nstand),
                raw[GUARD + self.ngain:GUARD + self.ngain + self.nstat].copy().view(np.float32).reshape(self.nfine, 2, 4))

    def run(self, V, warm=0):
        self.upload(V)
        self.enqueue(warm)
        ffi.call("xengGaincalSync")
        return self.result()

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengGaincalCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengGaincalDestroy")
        self.din.free()
        self.dout.free()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _case(nstand, nsrc, nfine, noise=0.0, seed=None):
    rng, tau, freq, flux, w, g = setup(100 + nstand if seed is None else seed, nstand, nsrc, nfine)
    V = corrupt(model(freq, tau, flux), g)
    if noise:
        V = noisy(rng, V, noise)
    return tau, freq, flux, w, g, V


# ---------------------------------------------------------------- 1. parity with float64
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["clean", "noisy"])
@pytest.mark.parametrize("nstand,nsrc,nfine", [(22, 1, 4), (35, 3, 3), (64, 32, 2)])
def test_parity_with_the_float64_restatement(nstand, nsrc, nfine, noise):
    """A partial column tile and one source; an odd stand count over two column tiles and three sources; an exact fit of two column
    tiles and all 32 sources.  Stand 3 flagged.  V = g g^H o M rounded to complex64, and the same plus Hermitian noise of uneven
    rows; tol = 0 and the iteration count test_gaincal_cpu.py measured, so every (channel, pol) runs exactly that many.  Every
    (channel, pol) within five float gaps of the float64 restatement."""
    tau, freq, flux, w, g, V = _case(nstand, nsrc, nfine, noise)
    niter = ITERATIONS[(nstand, nsrc, nfine)]
    ref, rstats, _ = solve(V, freq, tau, flux, w, 0, niter, 0.0)
    gap = float_gap(V, freq, tau, flux, w, 0, niter, ref=ref)
    gc = GC(tau, freq, flux, w, 0, niter, 0.0)
    got, stats = gc.run(V)
    assert _info()[1:] == (niter, 0.0, 0)
    gc.close()
    err = gain_error(got, ref)
    print("gaincal parity %d stands %d sources noise %g: float gap %.3g, bar %.3g, worst error %.3g = %.2f of the bar" % (nstand, nsrc, noise, gap, 5 * gap, err.max(),
                                                                                                                       err.max() / (5 * gap)))
    assert np.isfinite(got.view(np.float32)).all() and (err <= 5 * gap).all(), (err.max(), 5 * gap)
    assert (got[:, :, 3] == 0).all() and np.array_equal(stats[:, :, [0, 2, 3]], rstats[:, :, [0, 2, 3]])
    # (delta is a ratio of norms of gains that are each within the bar: by the triangle inequality it is within two bars)
    assert (np.abs(stats[:, :, 1] - rstats[:, :, 1]) <= 10 * gap).all()


# ---------------------------------------------------------------- 2. the early exit
@pytest.mark.parametrize("nstand,nsrc,nfine,tol", [(22, 1, 4, 3e-5), (35, 3, 3, 1e-4), (64, 32, 2, 3e-5)])
def test_early_exit_counts_and_flags_are_the_restatements(nstand, nsrc, nfine, tol):
    """Inputs and a tol at which the complex64 and the float64 restatement stop at the same iteration for every (channel, pol),
    every delta either of them forms being a factor 1.2 or more away from tol (checked here, on the CPU: a condition on the inputs;
    the device's delta is within a few 1e-6 of theirs).  The device's iteration counts and converged flags are then theirs, the
    counts differ among the (channel, pol)s of one launch, and the gains are within the bar."""
    tau, freq, flux, w, g, V = _case(nstand, nsrc, nfine)
    t64, t32 = [], []
    ref, rstats, _ = solve(V, freq, tau, flux, w, 0, 60, tol, trace=t64)
    s32 = solve(V, freq, tau, flux, w, 0, 60, tol, np.complex64, trace=t32)[1]
    assert np.array_equal(rstats[:, :, [0, 3]], s32[:, :, [0, 3]]) and (rstats[:, :, 3] == 1).all() and len(set(rstats[:, :, 0].ravel())) > 1
    assert all(max(d / tol, tol / d) >= 1.2 for _, _, _, d in t64 + t32)
    gap = float_gap(V, freq, tau, flux, w, 0, 60, tol, ref=ref)
    gc = GC(tau, freq, flux, w, 0, 60, tol)
    got, stats = gc.run(V)
    gc.close()
    print("gaincal early exit %d stands: iterations %s, restatement %s" % (nstand, stats[:, :, 0].ravel(), rstats[:, :, 0].ravel()))
    assert np.array_equal(stats[:, :, [0, 2, 3]], rstats[:, :, [0, 2, 3]])
    assert (stats[:, :, 1] <= tol).all() and (gain_error(got, ref) <= 5 * gap).all()


# ---------------------------------------------------------------- 3. bit identity
def test_channel_subsets_weights_back_and_forth_fresh_context_other_kernels_and_a_warm_start_change_no_bit():
    """35 stands, 3 sources, 3 channels, tol 1e-4 (every (channel, pol) converges, after counts of its own).  The last channel alone,
    and the first two, in contexts of their own: the corresponding words of the full run.  The same call after SetWeights to other
    weights (which changes the gains) and back; in a fresh context; in a fresh context while X-engine contractions run on their
    streams and xengBeamformRun on this one.  And a warm start with niter = 0 from the converged solution returns that solution,
    with 0 iterations in its stats."""
    nstand, nsrc, nfine, tol = 35, 3, 3, 1e-4
    tau, freq, flux, w, g, V = _case(nstand, nsrc, nfine, 0.05)
    w1 = np.roll(w, 5)
    gc = GC(tau, freq, flux, w, 0, 60, tol)
    full = gc.run(V)
    assert (full[1][:, :, 3] == 1).all() and np.isfinite(full[0].view(np.float32)).all()
    gc.set_weights(w1, 1)
    other = gc.run(V)
    gc.set_weights(w, 0)
    again = gc.run(V)
    assert _same(again, full) and not _same(other, full)
    ffi.call("xengGaincalSetSolver", 0, tol)
    kept, kstats = gc.run(V, warm=1)
    assert kept.tobytes() == full[0].tobytes() and (kstats[:, :, 0] == 0).all() and (kstats[:, :, 1] == -1).all() and (kstats[:, :, 3] == 0).all()
    cold, _ = gc.run(V, warm=0)                  # (niter = 0 without the warm start: the start itself, 1 at every live stand)
    assert np.array_equal(cold, np.broadcast_to(np.where(w != 0, 1, 0).astype(np.complex64), cold.shape))
    gc.close()
    for sel in (slice(nfine - 1, None), slice(0, 2)):
        gc = GC(tau, freq[sel], flux[sel], w, 0, 60, tol)
        sub = gc.run(np.ascontiguousarray(V[sel]))
        gc.close()
        assert _same(sub, (full[0][sel], full[1][sel]))
    bstand, bchan, btime, nbeam = 96, 8, 96, 4
    rng = np.random.default_rng(3)
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, bstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * bstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    gc = GC(tau, freq, flux, w, 0, 60, tol)
    gc.upload(V)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(3):
            for q in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + q * xg.gulp_bytes, xg.out.ptr, int(q == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            gc.enqueue()
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengGaincalSync")
            got.append(gc.result())
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    gc.close()
    ffi.call("xengBeamformDestroy")
    assert all(_same(x, full) for x in got)


# ---------------------------------------------------------------- 4. non-finite visibilities
def test_flagged_stands_holding_nan_are_the_stands_holding_zeros():
    """w_9 = 0 and w_33 = 0 (one in each column tile), NaN and Inf all over their rows and columns, in the cross hands too:
    bit-identical to the same matrix with zeros there, finite, and the two gains are 0."""
    nstand, nsrc, nfine = 35, 3, 2
    rng, tau, freq, flux, w, g = setup(51, nstand, nsrc, nfine, flagged=(9, 33))
    V = noisy(rng, corrupt(model(freq, tau, flux), g), 0.05)
    zeros, bad = V.copy(), V.copy()
    for s in (9, 33):
        zeros[:, s] = 0
        zeros[:, :, :, s] = 0
        bad[:, s] = np.nan
        bad[:, :, :, s] = np.inf
    gc = GC(tau, freq, flux, w, 0, 20, 1e-4)
    a, b = gc.run(zeros), gc.run(bad)
    gc.close()
    assert np.isfinite(a[0].view(np.float32)).all() and np.isfinite(a[1]).all() and _same(a, b) and (a[0][:, :, [9, 33]] == 0).all()
    assert (a[1][:, :, 2] == nstand - 2).all() and np.abs(a[0][:, :, 0]).min() > 0


def test_nan_in_a_read_stand_stays_within_its_channel_and_polarisation():
    """A NaN in V[c = 1][4 1][11 1] (channel 1 of three, polarisation 1): every other (channel, pol) is bit-identical to the clean
    run; (1, 1) is not converged after all 60 iterations and every gain of it is NaN or 0, none solved.  A NaN in a cross hand, V[1][4 0][11 1], is not read: no word changes."""
    nstand, nsrc, nfine = 22, 3, 3
    tau, freq, flux, w, g, V = _case(nstand, nsrc, nfine, 0.05, seed=61)
    bad, cross = V.copy(), V.copy()
    bad[1, 4, 1, 11, 1] = np.nan
    cross[1, 4, 0, 11, 1] = np.nan
    gc = GC(tau, freq, flux, w, 0, 60, 1e-4)
    clean, got, same = gc.run(V), gc.run(bad), gc.run(cross)
    gc.close()
    assert np.isfinite(clean[0].view(np.float32)).all() and (clean[1][:, :, 3] == 1).all() and _same(same, clean)
    others = np.ones((nfine, 2), bool)
    others[1, 1] = False
    assert got[0][others].tobytes() == clean[0][others].tobytes() and got[1][others].tobytes() == clean[1][others].tobytes()
    # (the NaN reaches every D of its (channel, pol) through the Gram matrix, and a D that is not > 0 gives the gain 0)
    x = got[0][1, 1]
    assert got[1][1, 1, 3] == 0 and got[1][1, 1, 0] == 60 and got[1][1, 1, 2] == 0 and (np.isnan(x) | (x == 0)).all()


# ---------------------------------------------------------------- 5. the warm start
def test_warm_start_takes_no_more_iterations_and_an_unconverged_solution_starts_cold():
    """Two integrations of one sky through one set of gains, each with noise of its own.  On the second the warm start needs no more
    iterations than the cold start in any (channel, pol) and fewer in all together -- a property of the restatement, checked on the
    CPU first; the device's counts are compared with each other only.  After a first run that no (channel, pol) converged in (4
    iterations) a warm start is the cold start bit for bit; SetModel and SetWeights forget a converged solution."""
    nstand, nsrc, nfine, tol = 35, 3, 3, 1e-4
    rng, tau, freq, flux, w, g = setup(71, nstand, nsrc, nfine)
    V0 = corrupt(model(freq, tau, flux), g)
    Va, Vb = noisy(rng, V0, 0.02), noisy(rng, V0, 0.02)
    keep = solve(Va, freq, tau, flux, w, 0, 60, tol, np.complex64)[2]
    rcold = solve(Vb, freq, tau, flux, w, 0, 60, tol, np.complex64)[1][:, :, 0]
    rwarm = solve(Vb, freq, tau, flux, w, 0, 60, tol, np.complex64, start=keep)[1][:, :, 0]
    assert keep[1].all() and (rwarm <= rcold).all() and rwarm.sum() < rcold.sum()
    gc = GC(tau, freq, flux, w, 0, 60, tol)
    cold = gc.run(Vb)
    gc.run(Va)
    warm = gc.run(Vb, warm=1)
    print("gaincal warm start: cold %s, warm %s iterations" % (cold[1][:, :, 0].ravel(), warm[1][:, :, 0].ravel()))
    assert (warm[1][:, :, 3] == 1).all() and (warm[1][:, :, 0] <= cold[1][:, :, 0]).all() and warm[1][:, :, 0].sum() < cold[1][:, :, 0].sum()
    assert (gain_error(warm[0], cold[0]) <= 10 * tol).all()
    gc.run(Va)
    gc.set_model(tau, freq, flux)
    assert _same(gc.run(Vb, warm=1), cold)
    gc.run(Va)
    gc.set_weights(w, 0)
    assert _same(gc.run(Vb, warm=1), cold)
    ffi.call("xengGaincalSetSolver", 4, tol)
    short = gc.run(Va)
    assert (short[1][:, :, 3] == 0).all() and (short[1][:, :, 0] == 4).all()
    ffi.call("xengGaincalSetSolver", 60, tol)
    assert _same(gc.run(Vb, warm=1), cold)
    gc.close()


# ---------------------------------------------------------------- 6. the ABI
def test_info_tickets_and_argument_checks_with_and_without_a_context():
    """GetInfo; Run before SetModel and before SetWeights is INVALID_STATE and launches nothing; SetModel refuses non-finite words
    and negative fluxes, SetWeights negative and non-finite weights and a reference stand out of range or of weight 0, SetSolver
    what is past its limits, and they change nothing; tickets count from 1 after Initialize and every one is done after Sync;
    every INVALID_ARGUMENT of Initialize leaves a live context alone; after Destroy every call that needs a context is
    INVALID_STATE."""
    nstand, nsrc, nfine = 6, 2, 2
    tau, freq, flux, w, g, V = _case(nstand, nsrc, nfine, seed=81)
    gc = GC(tau, freq, flux, model=False)
    assert _info() == (32 * 33 * 8 + 32 * 4 + 2 * 32 * 8 + 32 * 4 + 32 * 32 * 8 + 2 * 4 * 4, 60, 1e-5, 0)
    gc.upload(V)
    for step in (lambda: gc.set_model(tau, freq, flux), lambda: gc.set_weights(w, 1)):
        with pytest.raises(ffi.XengError) as ei:
            gc.enqueue()
        assert ei.value.status == INVALID_STATE
        step()
    ffi.call("xengGaincalSync")
    gc.result()                                 # (nothing was written)
    ffi.call("xengGaincalSetSolver", 20, 1e-4)
    first = gc.run(V)
    f32 = np.ascontiguousarray(flux, np.float32)
    for bt, bf, bx in ((np.where(np.arange(tau.size).reshape(tau.shape) == 7, np.nan, tau), freq, f32), (tau, np.where(np.arange(nfine) == 1, np.inf, freq), f32),
                       (tau, freq, np.where(np.arange(4).reshape(2, 2) == 3, -1, f32)), (tau, freq, np.where(np.arange(4).reshape(2, 2) == 0, np.nan, f32))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengGaincalSetModel", _dp(np.ascontiguousarray(bt, np.float64)), _dp(np.ascontiguousarray(bf, np.float64)), _fp(np.ascontiguousarray(bx, np.float32)))
        assert ei.value.status == INVALID_ARGUMENT
    for bad, ref in (([1, 1, 1, 1, 1, -1], 0), ([1, 1, 1, 1, 1, np.nan], 0), ([1, 1, 1, 1, 1, np.inf], 0), ([1, 1, 1, 1, 1, 1], 6), ([1, 1, 1, 1, 1, 1], -1),
                     ([1, 1, 0, 1, 1, 1], 2)):
        with pytest.raises(ffi.XengError) as ei:
            gc.set_weights(np.array(bad, np.float32), ref)
        assert ei.value.status == INVALID_ARGUMENT, (bad, ref)
    for bad in ((-1, 1e-4), (1025, 1e-4), (20, -1.0), (20, float('inf'))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengGaincalSetSolver", *bad)
        assert ei.value.status == INVALID_ARGUMENT, bad
    assert _info()[1:] == (20, 1e-4, 1) and _same(gc.run(V), first)
    ffi.call("xengGaincalSetSolver", 1024, 0.0)  # (the limits themselves are taken)
    ffi.call("xengGaincalSetSolver", 20, 1e-4)
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    ffi.call("xengGaincalMark", ctypes.byref(t))
    assert t.value == 1
    gc.enqueue()
    ffi.call("xengGaincalMark", ctypes.byref(t))
    assert t.value == 2
    ffi.call("xengGaincalWait", 2)
    ffi.call("xengGaincalSync")
    gc.result()
    for k in (1, 2):
        ffi.call("xengGaincalTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, 3):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengGaincalWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, nfine, nsrc), (0, 513, nfine, nsrc), (0, nstand, 0, nsrc), (0, nstand, nfine, 33), (0, nstand, nfine, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengGaincalInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info()[1:] == (20, 1e-4, 1)
    out = gc.dout.ptr + GUARD
    for args in ((None, out, out + gc.ngain, 0), (gc.din.ptr, None, out + gc.ngain, 0), (gc.din.ptr, out, None, 0), (gc.din.ptr + 8, out, out + gc.ngain, 0),
                 (gc.din.ptr, out + 4, out + gc.ngain, 0), (gc.din.ptr, out, out + gc.ngain + 2, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengGaincalRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengGaincalSync")
    gc.result()
    gc.close()
    s, n = ctypes.c_int(), ctypes.c_double()
    for name, args in (("xengGaincalRun", (4096, 4096, 4096, 0)), ("xengGaincalSetModel", (_dp(tau), _dp(freq), _fp(f32))), ("xengGaincalSetWeights", (_fp(w), 0)),
                       ("xengGaincalSetSolver", (10, 1e-5)), ("xengGaincalGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), ctypes.byref(s))),
                       ("xengGaincalMark", (ctypes.byref(t),)), ("xengGaincalWait", (1,)), ("xengGaincalTicketDone", (1, ctypes.byref(d))), ("xengGaincalSync", ()),
                       ("xengGaincalCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengGaincalDestroy")


# ---------------------------------------------------------------- 7. the chain on device rings
def test_source_to_upchan_corr_to_upchan_gaincal_on_device_rings():
    """Source -> UpchanCorr (44 inputs, 2 coarse channels, nupchan 2, one gulp of 64 samples per integration) -> UpchanGainCal (3
    sources, one stand flagged, 10 iterations) on device rings, three integrations: each span is, bit for bit, what the stand-alone
    calls give on UpchanCorr's own output spans -- the first from a cold start, the others warm; the header says what was solved."""
    nstand, nchan, g, N, nsrc, seq0, sfreq, niter, tol, nint = 22, 2, 64, 2, 3, 6400, 55e6, 10, 1e-3, 3
    ninput, nfine = 2 * nstand, nchan * N
    rng = np.random.default_rng(91)
    pos, lmn = random_array(rng, nstand, 1200.0, 5.0), sky(rng, nsrc)
    flux = [5.0, 2.0, 1.0]
    w = rng.uniform(0.5, 2.0, nstand).astype(np.float32)
    w[6] = 0
    vin = rng.integers(0, 256, (nint * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=sfreq)
    r0, r1, r2 = Ring("f-engine", space="cuda"), Ring("uc-output", space="cuda"), Ring("gaincal-output", space="cuda")
    uc = UpchanCorr(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=g // N, gpu=0)
    cal = UpchanGainCal(LOG, r1, r2, pos, lmn, flux, weights=w, refant=2, niter=niter, tol=tol, gpu=0)
    ngain = nfine * 2 * nstand * 8
    mid, sink = Sink(r1, nfine * ninput * ninput * 8), Sink(r2, ngain + nfine * 2 * 4 * 4)
    run_blocks([uc, cal], Source(r0, [(hdr, vin.reshape(-1), g * nchan * ninput)]), [mid, sink])
    ok = ctypes.c_int()
    ffi.call("xengGaincalCheckGuards", ctypes.byref(ok))
    ffi.call("xengGaincalDestroy")
    ffi.call("xengUpchanCorrDestroy")
    assert ok.value == 1
    (vh, _, vspans), = mid.sequences
    (gh, gtag, gspans), = sink.sequences
    assert len(vspans) == len(gspans) == nint and gtag == gh['seq0'] == seq0 and cal.stats['nsolve'] == nint
    assert (gh['nsrc'], gh['refant'], gh['niter'], gh['tol'], gh['stats_offset'], gh['nbit'], gh['complex'], gh['nfine']) == (nsrc, 2, niter, tol, ngain, 32, True, nfine)
    freq = vh['fine_sfreq'] + vh['fine_bw_hz'] * np.arange(nfine)
    gc = GC(steering_delays(pos, lmn), freq, np.asarray(flux, np.float32), w, 2, niter, tol)
    for k in range(nint):
        V = np.ascontiguousarray(vspans[k]).view(np.uint8).reshape(-1).view(np.complex64).reshape(nfine, nstand, 2, nstand, 2)
        gains, stats = gc.run(V, warm=int(k > 0))
        raw = np.ascontiguousarray(gspans[k]).view(np.uint8).reshape(-1)
        assert raw[:ngain].tobytes() == gains.tobytes() and raw[ngain:].tobytes() == stats.tobytes(), k
        assert (gains[:, :, 6] == 0).all() and (stats[:, :, 0] <= niter).all()
    gc.close()
