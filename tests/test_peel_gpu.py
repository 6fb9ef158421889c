"""UpchanPeel on the MI355X: xengPeel* against the restatement (tests/peel_ref.py).  Parity of the gains and of the output with the
float64 restatement at a fixed sweep count, with the output's structure; the early exit's counts and flags; bit identity of a subset
of the channels, after SetWeights back and forth, in a fresh context, beside an X-engine contraction and xengBeamformRun, and of a
warm start with niter = 0; a flagged stand that holds NaN; a NaN in a stand that is read; the residual against one shared gain; the
ABI with and without a context; Source -> UpchanCorr -> UpchanCalApply -> UpchanPeel -> UpchanImage on device rings.  The outputs sit
between two poisoned 64 KiB guard bands that are checked after every call, the state's guards at every close.  No wall-clock
assertions.

The bars of the parity tests are not constants: they are five times the worst gap between the complex64 and the float64 evaluation
of the restatement ON THE TEST'S OWN INPUTS (tests/peel_ref.py float_gap) -- for the gains per (channel, pol, direction) as max_s |g -
g_ref| / rms_s |g_ref|, for the output per (channel, pol) as max |out - out_ref| / rms |V|.  The sweep counts are those
tests/test_peel_cpu.py measured (ITERATIONS).  Measured on the MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import UpchanCalApply, UpchanCorr, UpchanImage, UpchanPeel, steering_delays  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import calapply_ref  # noqa: E402
from tests.calapply_ref import hermitian_bits  # noqa: E402
from tests.gaincal_ref import sky  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.image_ref import random_array  # noqa: E402
from tests.peel_ref import case, dir_gain_error, float_gap, hermitian_nan, out_error, peel, solve  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_image_gpu import IM  # noqa: E402
from tests.test_peel_cpu import ITERATIONS  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
# worst error / bar over test_parity_with_the_float64_restatement on the MI355X, per (nstand, ndir, inputs): (gains, output)
MEASURED = {(22, 1, "clean"): (0.12, 0.22), (22, 1, "noisy"): (0.12, 0.22), (35, 3, "clean"): (0.27, 0.28), (35, 3, "noisy"): (0.17, 0.24),
            (64, 8, "clean"): (0.47, 0.24), (64, 8, "noisy"): (0.68, 0.36), (70, 2, "clean"): (0.21, 0.30), (70, 2, "noisy"): (0.30, 0.28)}
# (worst gain errors 3.0e-7 (22, 1) to 2.0e-5 (the weakest of 8 directions at 64 stands) against gaps of 4.7e-7 to 8.5e-6; worst output errors
# 6.1e-7 to 1.6e-6 against gaps of 5.5e-7 to 1.0e-6; the early exit's sweep counts at tol 1e-5 are the complex64 and the float64 restatement's in
# all 20 (channel, pol)s; in the chain the image at a peeled source falls from 1300 .. 4100 to below 0.04)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _info():
    l, n, t, r, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_int(), ctypes.c_longlong()
    ffi.call("xengPeelGetInfo", ctypes.byref(l), ctypes.byref(n), ctypes.byref(t), ctypes.byref(r), ctypes.byref(b))
    return l.value, n.value, t.value, r.value, b.value


class PL:
    """The xengPeel context (one per process), an input buffer and the outputs of one call -- the span, the gains, the stats --
    between two poisoned guard bands."""

    def __init__(self, tau, freq, flux, w=None, refant=0, niter=None, tol=0.0, model=True):
        self.ndir, self.nstand = tau.shape
        self.nfine = len(freq)
        ffi.call("xengPeelInitialize", 0, self.nstand, self.nfine, self.ndir)
        if model:
            self.set_model(tau, freq, flux)
        if w is not None:
            self.set_weights(w, refant)
        if niter is not None:
            ffi.call("xengPeelSetSolver", niter, tol)
        self.nspan = self.nfine * (2 * self.nstand) ** 2 * 8
        self.din = ffi.DeviceBuffer(self.nspan)
        self.ngain, self.nstat = self.nfine * 2 * self.ndir * self.nstand * 8, self.nfine * 2 * 4 * 4
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nspan + self.ngain + self.nstat)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def set_model(self, tau, freq, flux):
        ffi.call("xengPeelSetModel", _dp(np.ascontiguousarray(tau, np.float64)), _dp(np.ascontiguousarray(freq, np.float64)),
                 _fp(np.ascontiguousarray(np.broadcast_to(flux, (self.nfine, self.ndir)), np.float32)))

    def set_weights(self, w, refant):
        ffi.call("xengPeelSetWeights", _fp(np.ascontiguousarray(w, np.float32)), int(refant))

    def upload(self, V):
        assert V.shape == (self.nfine, self.nstand, 2, self.nstand, 2) and V.dtype == np.complex64
        self.din.upload(np.ascontiguousarray(V))

    def pointers(self):
        o = self.dout.ptr + GUARD
        return self.din.ptr, o, o + self.nspan, o + self.nspan + self.ngain

    def enqueue(self, warm=0):
        ffi.call("xengPeelRun", *self.pointers(), int(warm))

    def result(self):
        """After a sync: (out, gains, stats) (the poison is put back); every byte before them and past them must still be poison."""
        raw = self.dout.download(np.uint8)
        end = GUARD + self.nspan + self.ngain + self.nstat
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[end:] == POISON).all(), "bytes past the output were written"
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        a, b = GUARD + self.nspan, GUARD + self.nspan + self.ngain
        return (raw[GUARD:a].copy().view(np.complex64).reshape(self.nfine, self.nstand, 2, self.nstand, 2),
                raw[a:b].copy().view(np.complex64).reshape(self.nfine, 2, self.ndir, self.nstand), raw[b:end].copy().view(np.float32).reshape(self.nfine, 2, 4))

    def run(self, V, warm=0):
        self.upload(V)
        self.enqueue(warm)
        ffi.call("xengPeelSync")
        return self.result()

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengPeelCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengPeelDestroy")
        self.din.free()
        self.dout.free()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _cross_hands_equal(out, V):
    return all(np.ascontiguousarray(out[:, :, p, :, 1 - p]).tobytes() == np.ascontiguousarray(V[:, :, p, :, 1 - p]).tobytes() for p in range(2))


# ---------------------------------------------------------------- 1. parity with float64, and the output's structure
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["clean", "noisy"])
@pytest.mark.parametrize("nstand,ndir,nfine", [(22, 1, 3), (35, 3, 3), (64, 8, 2), (70, 2, 2)])
def test_parity_with_the_float64_restatement(nstand, ndir, nfine, noise):
    """A single partial tile and one direction; an odd stand count over two tiles (a partial and a diagonal tile pair in the
    subtraction) and three directions; an exact fit of two tiles and all 8 directions; three tiles a side, the last ragged.  Stand 3
    flagged.  Bright sources through gains near 1 over a background the model does not know, and the same plus Hermitian noise; tol
    = 0 and the sweep count test_peel_cpu.py measured, so every (channel, pol) runs exactly that many.  Every (channel, pol,
    direction) of the gains and every (channel, pol) of the output within five float gaps of the float64 restatement; the output
    Hermitian bit for bit, its cross hands and the flagged stand's rows and columns the input's."""
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, noise=noise)
    niter = ITERATIONS[(nstand, ndir, nfine)]
    ref = peel(V, freq, tau, flux, w, 0, niter, 0.0)
    ggap, ogap = float_gap(V, freq, tau, flux, w, 0, niter, ref=ref)
    pl = PL(tau, freq, flux, w, 0, niter, 0.0)
    out, got, stats = pl.run(V)
    assert _info()[1:] == (niter, 0.0, 0, pl.nspan)
    pl.close()
    gerr, oerr = dir_gain_error(got, ref[1]), out_error(out, ref[0], V)
    print("peel parity %d stands %d directions noise %g: float gaps %.3g %.3g; worst gain error %.3g = %.2f of the bar, worst output error %.3g = %.2f of the bar"
          % (nstand, ndir, noise, ggap, ogap, gerr.max(), gerr.max() / (5 * ggap), oerr.max(), oerr.max() / (5 * ogap)))
    assert np.isfinite(got.view(np.float32)).all() and np.isfinite(out.view(np.float32)).all()
    assert (gerr <= 5 * ggap).all(), (gerr.max(), 5 * ggap)
    assert (oerr <= 5 * ogap).all(), (oerr.max(), 5 * ogap)
    assert (got[:, :, :, 3] == 0).all() and np.array_equal(stats[:, :, [0, 2, 3]], ref[2][:, :, [0, 2, 3]])
    # (delta is a ratio of norms of gains that are each within the bar: by the triangle inequality it is within two bars)
    assert (np.abs(stats[:, :, 1] - ref[2][:, :, 1]) <= 10 * ggap).all()
    assert hermitian_bits(out) and _cross_hands_equal(out, V)
    assert out[:, 3].tobytes() == V[:, 3].tobytes() and np.ascontiguousarray(out[:, :, :, 3]).tobytes() == np.ascontiguousarray(V[:, :, :, 3]).tobytes()


# ---------------------------------------------------------------- 2. the early exit
def test_early_exit_counts_and_flags_are_the_restatements():
    """tol = 1e-5 on the four shapes, noisy inputs: the device's converged flags and sweep counts are the complex64 restatement's.
    A (channel, pol) whose count differs is let pass only where its float64 delta at that exit sweep lies within a factor 2 of tol
    (the device's delta is within a few 1e-6 of the restatements'; such a one may fall on the other side), and at most 1 in 10 over
    all shapes may.  The gains are within the bar where the count is the float64 restatement's."""
    tol, total, left_out = 1e-5, 0, 0
    for nstand, ndir, nfine in [(22, 1, 3), (35, 3, 3), (64, 8, 2), (70, 2, 2)]:
        tau, freq, flux, w, g, V = case(nstand, ndir, nfine, noise=0.05)
        t64 = []
        r64 = solve(V, freq, tau, flux, w, 0, 60, tol, trace=t64)
        r32 = solve(V, freq, tau, flux, w, 0, 60, tol, np.complex64)
        ref = peel(V, freq, tau, flux, w, 0, 60, tol)
        ggap, _ = float_gap(V, freq, tau, flux, w, 0, 60, tol, ref=ref)
        pl = PL(tau, freq, flux, w, 0, 60, tol)
        out, got, stats = pl.run(V)
        pl.close()
        print("peel early exit %d stands %d directions: sweeps %s, complex64 restatement %s, float64 %s" % (nstand, ndir, stats[:, :, 0].ravel(), r32[1][:, :, 0].ravel(),
                                                                                                          r64[1][:, :, 0].ravel()))
        differ = np.argwhere((stats[:, :, 0] != r32[1][:, :, 0]) | (stats[:, :, 3] != r32[1][:, :, 3]))
        for c, p in differ:
            ds = [d for cc, pp, it, d in t64 if (cc, pp) == (c, p) and it <= r32[1][c, p, 0]]
            assert ds and tol / 2 <= ds[-1] <= 2 * tol, (nstand, ndir, c, p, stats[c, p], r32[1][c, p])
        total += stats[:, :, 0].size
        left_out += len(differ)
        assert (stats[:, :, 3] == 1).all() and (stats[:, :, 1] <= tol).all() and (stats[:, :, 2] == nstand - 1).all()
        same = stats[:, :, 0] == r64[1][:, :, 0]
        assert (dir_gain_error(got, ref[1])[same] <= 5 * ggap).all()
    assert 10 * left_out <= total, (left_out, total)


# ---------------------------------------------------------------- 3. bit identity
def test_channel_subsets_weights_back_and_forth_fresh_context_other_kernels_and_a_warm_start_change_no_bit():
    """35 stands, 3 directions, 3 channels, tol 1e-5 (every (channel, pol) converges).  The last channel alone, and the first two,
    in contexts of their own: the corresponding words of the full run.  The same call after SetWeights to other weights (which
    changes the result) and back; in a fresh context while X-engine contractions run on their streams and xengBeamformRun on this
    one.  And a warm start with niter = 0 from the converged solution returns that solution and the same output, with 0 sweeps in
    its stats; a cold one the unit gains."""
    nstand, ndir, nfine, tol = 35, 3, 3, 1e-5
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, noise=0.05)
    w1 = np.roll(w, 5)
    pl = PL(tau, freq, flux, w, 0, 60, tol)
    full = pl.run(V)
    assert (full[2][:, :, 3] == 1).all() and np.isfinite(full[1].view(np.float32)).all()
    pl.set_weights(w1, 1)
    other = pl.run(V)
    pl.set_weights(w, 0)
    again = pl.run(V)
    assert _same(again, full) and not _same(other, full)
    ffi.call("xengPeelSetSolver", 0, tol)
    kout, kept, kstats = pl.run(V, warm=1)
    assert kept.tobytes() == full[1].tobytes() and kout.tobytes() == full[0].tobytes()
    assert (kstats[:, :, 0] == 0).all() and (kstats[:, :, 1] == -1).all() and (kstats[:, :, 3] == 0).all()
    _, cold, _ = pl.run(V, warm=0)              # (niter = 0 without the warm start: the start itself, 1 at every live stand)
    assert np.array_equal(cold, np.broadcast_to(np.where(w != 0, 1, 0).astype(np.complex64), cold.shape))
    pl.close()
    for sel in (slice(nfine - 1, None), slice(0, 2)):
        pl = PL(tau, freq[sel], flux[sel], w, 0, 60, tol)
        sub = pl.run(np.ascontiguousarray(V[sel]))
        pl.close()
        assert _same(sub, tuple(x[sel] for x in full))
    bstand, bchan, btime, nbeam = 96, 8, 96, 4
    rng = np.random.default_rng(3)
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, bstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * bstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    pl = PL(tau, freq, flux, w, 0, 60, tol)
    pl.upload(V)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(3):
            for q in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + q * xg.gulp_bytes, xg.out.ptr, int(q == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            pl.enqueue()
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengPeelSync")
            got.append(pl.result())
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    pl.close()
    ffi.call("xengBeamformDestroy")
    assert all(_same(x, full) for x in got)


# ---------------------------------------------------------------- 4. non-finite visibilities
def test_flagged_stands_holding_nan_pass_through_and_touch_nothing_else():
    """w_9 = 0 and w_33 = 0 (one in each tile), NaN and Inf all over their rows and columns, the cross hands included (Hermitian bit
    for bit, as the ring's spans are): the gains and stats are bit-identical to those of the same matrix with zeros there, finite,
    and the two stands' gains are 0; their rows and columns of the output are the input's bit for bit, and every other word is the
    word of the run on the matrix with zeros."""
    nstand, ndir, nfine = 35, 3, 2
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, noise=0.05, flagged=(9, 33))
    zeros, bad = V.copy(), V
    for s in (9, 33):
        zeros[:, s] = 0
        zeros[:, :, :, s] = 0
        bad = hermitian_nan(bad, s)
    pl = PL(tau, freq, flux, w, 0, 20, 1e-5)
    a, b = pl.run(zeros), pl.run(bad)
    pl.close()
    assert np.isfinite(a[1].view(np.float32)).all() and np.isfinite(a[2]).all() and _same(a[1:], b[1:]) and (a[1][:, :, :, [9, 33]] == 0).all()
    assert (a[2][:, :, 2] == nstand - 2).all() and np.abs(a[1][:, :, :, 0]).min() > 0
    keep = np.ones(nstand, bool)
    keep[[9, 33]] = False
    assert np.ascontiguousarray(a[0][:, keep][:, :, :, keep]).tobytes() == np.ascontiguousarray(b[0][:, keep][:, :, :, keep]).tobytes()
    for s in (9, 33):
        assert b[0][:, s].tobytes() == bad[:, s].tobytes() and np.ascontiguousarray(b[0][:, :, :, s]).tobytes() == np.ascontiguousarray(bad[:, :, :, s]).tobytes()
    assert hermitian_bits(a[0])


def test_nan_in_a_read_stand_stays_within_its_channel_and_polarisation():
    """A NaN in V[c = 1][4 1][11 1] and its mirror (channel 1 of three, polarisation 1): the gains, the stats and the pp block of
    every other (channel, pol) are bit-identical to the clean run; (1, 1) is not converged after all 60 sweeps, none of its stands
    solved, every gain of it NaN or 0.  A NaN in a cross hand, V[1][11 1][4 0], is not read by the solve and is copied to the output:
    nothing else changes."""
    nstand, ndir, nfine = 22, 3, 3
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, noise=0.05, seed=61)
    bad, cross = V.copy(), V.copy()
    bad[1, 11, 1, 4, 1] = np.nan
    bad[1, 4, 1, 11, 1] = np.nan
    cross[1, 11, 1, 4, 0] = np.nan
    pl = PL(tau, freq, flux, w, 0, 60, 1e-5)
    clean, got, same = pl.run(V), pl.run(bad), pl.run(cross)
    pl.close()
    assert np.isfinite(clean[1].view(np.float32)).all() and (clean[2][:, :, 3] == 1).all() and _same(same[1:], clean[1:])
    diff = np.argwhere(same[0].view(np.uint64) != clean[0].view(np.uint64))
    assert sorted(map(tuple, diff)) == [(1, 4, 0, 11, 1), (1, 11, 1, 4, 0)]
    others = np.ones((nfine, 2), bool)
    others[1, 1] = False
    assert got[1][others].tobytes() == clean[1][others].tobytes() and got[2][others].tobytes() == clean[2][others].tobytes()
    for c in range(nfine):
        for p in range(2):
            if (c, p) != (1, 1):
                assert np.ascontiguousarray(got[0][c, :, p, :, p]).tobytes() == np.ascontiguousarray(clean[0][c, :, p, :, p]).tobytes()
    assert _cross_hands_equal(got[0], V)
    x = got[1][1, 1]
    assert got[2][1, 1, 3] == 0 and got[2][1, 1, 0] == 60 and got[2][1, 1, 2] == 0 and (np.isnan(x) | (x == 0)).all()


# ---------------------------------------------------------------- 5. against one shared gain
def test_residual_is_below_the_subtraction_with_one_shared_gain():
    """35 stands, 3 directions with gains of their own per direction (amplitude 1 +- 0.2, phase sigma 0.5 rad): the off-diagonal rms
    of the output's parallel hands over the live stands is below that of UpchanCalApply's subtraction of the same three sources with
    unit factors -- for the float64 restatements of both, and for the device's output against calapply's restatement.  Only the
    ordering is asserted."""
    nstand, ndir, nfine = 35, 3, 2
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, noise=0.05)
    live = w != 0
    off = live[:, None] & live[None, :] & ~np.eye(nstand, dtype=bool)

    def rms(x):
        return np.sqrt(np.mean([np.abs(np.asarray(x[:, :, p, :, p], np.complex128)[:, off]) ** 2 for p in range(2)]))

    shared = calapply_ref.apply(V, np.ones((nfine, 2, nstand), np.complex64), freq, tau, flux)
    ref = peel(V, freq, tau, flux, w, 0, 60, 1e-5)
    pl = PL(tau, freq, flux, w, 0, 60, 1e-5)
    out, got, stats = pl.run(V)
    pl.close()
    print("peel residual: input %.3g, one shared gain %.3g, per direction %.3g (float64 restatement %.3g)" % (rms(V), rms(shared), rms(out), rms(ref[0])))
    assert rms(ref[0]) < rms(shared) and rms(out) < rms(shared) and (stats[:, :, 3] == 1).all()


# ---------------------------------------------------------------- 6. the ABI
def test_info_tickets_and_argument_checks_with_and_without_a_context():
    """GetInfo; Run before SetModel and before SetWeights is INVALID_STATE and launches nothing; SetModel refuses non-finite words
    and negative fluxes, SetWeights negative and non-finite weights and a reference stand out of range or of weight 0, SetSolver
    what is past its limits, and they change nothing; tickets count from 1 after Initialize; ndir 0 and 9 and every other
    INVALID_ARGUMENT of Initialize leave a live context alone; a second Initialize replaces the context (no model, default solver);
    after Destroy every call that needs a context is INVALID_STATE."""
    nstand, ndir, nfine = 6, 2, 2
    tau, freq, flux, w, g, V = case(nstand, ndir, nfine, seed=81, flagged=(), nback=1)
    w = w.copy()
    w[2] = 0
    pl = PL(tau, freq, flux, model=False)
    nsp = 32
    lds = 4 * nsp * 9 * 8 + nsp * 4 + 8 * 4 + 8 * 32 * 8 + 8 * 8 + 2 * 4 * 4
    assert _info() == (lds, 60, 1e-5, 0, pl.nspan)
    pl.upload(V)
    for step in (lambda: pl.set_model(tau, freq, flux), lambda: pl.set_weights(w, 1)):
        with pytest.raises(ffi.XengError) as ei:
            pl.enqueue()
        assert ei.value.status == INVALID_STATE
        step()
    ffi.call("xengPeelSync")
    pl.result()                                 # (nothing was written)
    ffi.call("xengPeelSetSolver", 20, 1e-4)
    first = pl.run(V)
    f32 = np.ascontiguousarray(flux, np.float32)
    for bt, bf, bx in ((np.where(np.arange(tau.size).reshape(tau.shape) == 7, np.nan, tau), freq, f32), (tau, np.where(np.arange(nfine) == 1, np.inf, freq), f32),
                       (tau, freq, np.where(np.arange(4).reshape(2, 2) == 3, -1, f32)), (tau, freq, np.where(np.arange(4).reshape(2, 2) == 0, np.nan, f32))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeelSetModel", _dp(np.ascontiguousarray(bt, np.float64)), _dp(np.ascontiguousarray(bf, np.float64)), _fp(np.ascontiguousarray(bx, np.float32)))
        assert ei.value.status == INVALID_ARGUMENT
    for bad, ref in (([1, 1, 1, 1, 1, -1], 0), ([1, 1, 1, 1, 1, np.nan], 0), ([1, 1, 1, 1, 1, np.inf], 0), ([1, 1, 1, 1, 1, 1], 6), ([1, 1, 1, 1, 1, 1], -1),
                     ([1, 1, 0, 1, 1, 1], 2)):
        with pytest.raises(ffi.XengError) as ei:
            pl.set_weights(np.array(bad, np.float32), ref)
        assert ei.value.status == INVALID_ARGUMENT, (bad, ref)
    for bad in ((-1, 1e-4), (1025, 1e-4), (20, -1.0), (20, float('inf'))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeelSetSolver", *bad)
        assert ei.value.status == INVALID_ARGUMENT, bad
    assert _info()[1:4] == (20, 1e-4, 1) and _same(pl.run(V), first)
    ffi.call("xengPeelSetSolver", 1024, 0.0)    # (the limits themselves are taken)
    ffi.call("xengPeelSetSolver", 20, 1e-4)
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    ffi.call("xengPeelMark", ctypes.byref(t))
    t0 = t.value
    pl.enqueue()
    ffi.call("xengPeelMark", ctypes.byref(t))
    assert t.value == t0 + 1
    ffi.call("xengPeelWait", t.value)
    ffi.call("xengPeelSync")
    pl.result()
    for k in (t0, t0 + 1):
        ffi.call("xengPeelTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, t0 + 2):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeelWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, nfine, ndir), (0, 513, nfine, ndir), (0, nstand, 0, ndir), (0, nstand, nfine, 9), (0, nstand, nfine, 0), (0, nstand, 65536, ndir)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeelInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info()[1:4] == (20, 1e-4, 1)
    vin, out, gains, st = pl.pointers()
    for args in ((None, out, gains, st, 0), (vin, None, gains, st, 0), (vin, out, None, st, 0), (vin, out, gains, None, 0), (vin + 8, out, gains, st, 0),
                 (vin, out + 8, gains, st, 0), (vin, out, gains + 4, st, 0), (vin, out, gains, st + 2, 0), (vin, vin, gains, st, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPeelRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengPeelSync")
    pl.result()
    ok = ctypes.c_int()
    ffi.call("xengPeelCheckGuards", ctypes.byref(ok))
    assert ok.value == 1
    ffi.call("xengPeelInitialize", 0, nstand, nfine, ndir)      # a second Initialize: a new context
    assert _info()[1:4] == (60, 1e-5, 0)
    with pytest.raises(ffi.XengError) as ei:
        pl.enqueue()
    assert ei.value.status == INVALID_STATE
    pl.close()
    s, n, b = ctypes.c_int(), ctypes.c_double(), ctypes.c_longlong()
    for name, args in (("xengPeelRun", (4096, 8192, 4096, 4096, 0)), ("xengPeelSetModel", (_dp(tau), _dp(freq), _fp(f32))), ("xengPeelSetWeights", (_fp(w), 0)),
                       ("xengPeelSetSolver", (10, 1e-5)), ("xengPeelGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), ctypes.byref(s), ctypes.byref(b))),
                       ("xengPeelMark", (ctypes.byref(t),)), ("xengPeelWait", (1,)), ("xengPeelTicketDone", (1, ctypes.byref(d))), ("xengPeelSync", ()),
                       ("xengPeelCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengPeelDestroy")


# ---------------------------------------------------------------- 7. the chain on device rings
def _encode(x):
    """complex -> the F-engine's byte: 4-bit two's-complement real part in the high nibble, imaginary part in the low one"""
    re = np.clip(np.rint(x.real), -7, 7).astype(np.int16) & 0xF
    im = np.clip(np.rint(x.imag), -7, 7).astype(np.int16) & 0xF
    return ((re << 4) | im).astype(np.uint8)


def test_source_to_upchan_corr_to_upchan_calapply_to_upchan_peel_to_upchan_image_on_device_rings():
    """Source -> UpchanCorr (44 inputs, 2 coarse channels, nupchan 2, one gulp of 256 samples per integration) -> UpchanCalApply (unit
    gains, nothing subtracted) -> UpchanPeel (2 directions, one stand flagged, 30 sweeps) -> UpchanImage (the two directions and a
    third as pixels) on device rings, two integrations of voltages that hold two noise-like sources (amplitudes 4 and 2.5 on every
    input with their delays, an array of 100 m, plus receiver noise): each peeled span and solution() are, bit for bit, what the
    stand-alone calls give on UpchanCalApply's own output spans -- the first from a cold start, the second warm; the image at each
    peeled source's pixel drops to less than a fifth of what the imager reads on the unpeeled span; the headers say what was done."""
    nstand, nchan, g, N, ndir, seq0, sfreq, niter, tol, nint = 22, 2, 256, 2, 2, 6400, 55e6, 30, 0.0, 2
    ninput, nfine = 2 * nstand, nchan * N
    rng = np.random.default_rng(91)
    pos, lmn = random_array(rng, nstand, 100.0, 3.0), sky(rng, 3)
    w = np.ones(nstand, np.float32)
    w[6] = 0
    tau = steering_delays(pos, lmn)
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=sfreq)
    fc = sfreq + hdr['bw_hz'] / nchan * np.arange(nchan)                 # the coarse channels' centres
    x = 1.2 * (rng.standard_normal((nint * g, nchan, ninput)) + 1j * rng.standard_normal((nint * g, nchan, ninput)))
    for d, amp in zip(range(ndir), (4.0, 2.5)):
        s = amp * (rng.standard_normal((nint * g, nchan, 1)) + 1j * rng.standard_normal((nint * g, nchan, 1))) / np.sqrt(2)
        x = x + s * np.repeat(np.exp(-2j * np.pi * fc[:, None] * tau[d][None, :]), 2, axis=1)[None]
    vin = _encode(x)
    rings = [Ring(n, space="cuda") for n in ("f-engine", "uc-output", "calapply-output", "peel-output", "image-output")]
    uc = UpchanCorr(LOG, rings[0], rings[1], nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=g // N, gpu=0)
    cal = UpchanCalApply(LOG, rings[1], rings[2], pos, gpu=0)
    span = nfine * ninput * ninput * 8
    # the sources' fluxes in the correlator's units: the FFT is not normalised, so a source of variance a^2 per sample reads g a^2 per
    # integration (a little less after the 4-bit clipping).  The sweeps converge from gains within a factor of about 2 of 1 only.
    flux = [16.0 * g, 6.25 * g]
    pe = UpchanPeel(LOG, rings[2], rings[3], pos, lmn[:ndir], flux, weights=w, refant=2, niter=niter, tol=tol, gpu=0)
    img = UpchanImage(LOG, rings[3], rings[4], pos, lmn, weights=w, autos=False, gpu=0)
    mid, out, sink = Sink(rings[2], span), Sink(rings[3], span), Sink(rings[4], nfine * 4 * 3 * 4)
    run_blocks([uc, cal, pe, img], Source(rings[0], [(hdr, vin.reshape(-1), g * nchan * ninput)]), [mid, out, sink])
    sol = pe.solution()
    ok = ctypes.c_int()
    ffi.call("xengPeelCheckGuards", ctypes.byref(ok))
    for name in ("xengPeelDestroy", "xengCalapplyDestroy", "xengImageDestroy", "xengUpchanCorrDestroy"):
        ffi.call(name)
    assert ok.value == 1
    (vh, _, vspans), = mid.sequences
    (ph, ptag, pspans), = out.sequences
    (ih, itag, ispans), = sink.sequences
    assert len(vspans) == len(pspans) == len(ispans) == nint and ptag == ph['seq0'] == seq0 == itag and pe.stats['npeel'] == nint
    assert ph['npeeled'] == ndir and ph['nsubtracted'] == ndir and ph['calibrated'] is True and ph['nfine'] == nfine and ih['npix'] == 3
    freq = vh['fine_sfreq'] + vh['fine_bw_hz'] * np.arange(nfine)
    pl = PL(tau[:ndir], freq, np.asarray(flux, np.float32), w, 2, niter, tol)
    im = IM(tau, freq, 1)
    im.set_weights(w, False)
    for k in range(nint):
        V = np.ascontiguousarray(vspans[k]).view(np.uint8).reshape(-1).view(np.complex64).reshape(nfine, nstand, 2, nstand, 2)
        got = np.ascontiguousarray(pspans[k]).view(np.uint8).reshape(-1).view(np.complex64).reshape(nfine, nstand, 2, nstand, 2)
        exp, gains, stats = pl.run(V, warm=int(k > 0))
        assert got.tobytes() == exp.tobytes(), k
        assert hermitian_bits(got) and (gains[:, :, :, 6] == 0).all() and (stats[:, :, 0] == niter).all()
        before, after = im.run(V), im.run(got)
        assert np.ascontiguousarray(ispans[k]).view(np.uint8).tobytes() == after.tobytes(), k
        print("chain integration %d: image at the sources before %s, after %s" % (k, before[:, :2, :ndir].ravel(), after[:, :2, :ndir].ravel()))
        assert (np.abs(after[:, :2, :ndir]) < 0.2 * np.abs(before[:, :2, :ndir])).all()
    assert sol[0] == seq0 + (nint - 1) * g and sol[1].tobytes() == gains.tobytes() and sol[2].tobytes() == stats.tobytes()
    im.close()
    pl.close()
