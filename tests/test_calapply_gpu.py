"""UpchanCalApply on the MI355X: xengCalapply* against the restatement (tests/calapply_ref.py).  Parity with the float64 restatement;
the exact cases (a copy, scaling by powers of two, small integers); bit identity of the Hermitian pairs, of a channel run alone,
after SetFactors and SetModel back and forth, in a fresh context and beside an X-engine contraction and xengBeamformRun; flagged
stands that hold NaN; a NaN in a stand that is read; the ABI with a context; closure through xengImage* and xengGaincal*; Source ->
UpchanCorr -> UpchanCalApply -> UpchanImage on device rings.  The output sits between two poisoned 64 KiB guard bands that are
checked after every call, the state's guards at every close.  No wall-clock assertions.

The bar of the parity tests is not a constant: it is five times the worst gap between the complex64 and the float64 evaluation of
the restatement ON THE TEST'S OWN INPUTS (tests/calapply_ref.py float_gap), per word as |out - ref| / (|h_i||h_j| max|V| + sum_k
F_k).  Measured here on the CPU with numpy 2.2 (arrays of 1.2 km, so phases of hundreds of turns; gains of modulus 0.5 to 2): gaps of
7.8e-8 to 1.7e-7, so bars of 3.9e-7 to 8.4e-7; the kernel's source on host threads (tests/test_calapply_emul_cpu.py) reaches 0.10 to
0.32 of the bar.  Measured on the MI355X: see MEASURED below."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import UpchanCalApply, UpchanCorr, UpchanImage, steering_delays  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.imaging import image_norm  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import gaincal_ref, image_ref  # noqa: E402
from tests.calapply_ref import apply, case, factors, float_gap, hermitian_bits, scale, word_error  # noqa: E402
from tests.gaincal_ref import corrupt, model, sky  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.image_ref import random_array  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_gaincal_gpu import GC  # noqa: E402
from tests.test_image_gpu import IM  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
SHAPES = [(22, 1, 3), (35, 3, 2), (64, 32, 2), (70, 5, 1), (35, 0, 2)]      # (nstand, nsrc, nfine)
# worst word error / bar over test_parity_with_the_float64_restatement on the MI355X, per (nstand, nsrc)
MEASURED = {(22, 1): 0.10, (35, 3): 0.18, (64, 32): 0.32, (70, 5): 0.20, (35, 0): 0.20}
# (worst errors 8.4e-8, 8.5e-8, 2.0e-7, 1.2e-7, 7.8e-8 against gaps of 1.7e-7, 9.6e-8, 1.3e-7, 1.2e-7, 7.8e-8; the closure test: the imager's two readings
# differ by 0.005 of its bar and the solver returns |g - 1| <= 5.2e-7 = 0.35 of its bar; the chain on device rings 0.20 of the bar)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _info():
    t, g, l, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    ffi.call("xengCalapplyGetInfo", ctypes.byref(t), ctypes.byref(g), ctypes.byref(l), ctypes.byref(b))
    return t.value, g.value, l.value, b.value


class CA:
    """The xengCalapply context (one per process), an input buffer and the output of one call between two poisoned guard bands."""

    def __init__(self, nstand, freq, tau=None, flux=None, h=None, model=True):
        self.nstand, self.nfine = nstand, len(freq)
        self.nsrc = 0 if tau is None else np.shape(tau)[0]
        ffi.call("xengCalapplyInitialize", 0, self.nstand, self.nfine, self.nsrc)
        if model:
            self.set_model(tau, freq, flux)
        if h is not None:
            self.set_factors(h)
        self.nout = self.nfine * (2 * self.nstand) ** 2 * 8
        self.din = ffi.DeviceBuffer(self.nout)
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nout)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def set_model(self, tau, freq, flux):
        freq = np.ascontiguousarray(freq, np.float64)
        if self.nsrc:
            tau, flux = np.ascontiguousarray(tau, np.float64), np.ascontiguousarray(np.broadcast_to(flux, (self.nfine, self.nsrc)), np.float32)
            ffi.call("xengCalapplySetModel", _dp(tau), _dp(freq), _fp(flux))
        else:
            ffi.call("xengCalapplySetModel", None, _dp(freq), None)

    def set_factors(self, h):
        h = np.ascontiguousarray(h, np.complex64)
        assert h.shape == (self.nfine, 2, self.nstand)
        ffi.call("xengCalapplySetFactors", h.ctypes.data)

    def upload(self, V):
        assert V.shape == (self.nfine, self.nstand, 2, self.nstand, 2) and V.dtype == np.complex64
        self.din.upload(np.ascontiguousarray(V))

    def enqueue(self):
        ffi.call("xengCalapplyRun", self.din.ptr, self.dout.ptr + GUARD)

    def result(self):
        """After a sync: the output (the poison is put back); every byte before it and past it must still be poison."""
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.nout:] == POISON).all(), "bytes past the output were written"
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + self.nout].copy().view(np.complex64).reshape(self.nfine, self.nstand, 2, self.nstand, 2)

    def run(self, V):
        self.upload(V)
        self.enqueue()
        ffi.call("xengCalapplySync")
        return self.result()

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengCalapplyCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengCalapplyDestroy")
        self.din.free()
        self.dout.free()


def _upper_nan(V):
    """V with every word above the diagonal replaced by NaN: nothing may read them."""
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    up = np.triu(np.ones((n, n), bool), 1)
    return np.where(up[None], np.complex64(complex(np.nan, np.nan)), V.reshape(nfine, n, n)).reshape(V.shape).astype(np.complex64)


def _bits0(x):
    return bool((np.ascontiguousarray(x).view(np.uint32) == 0).all())


# ---------------------------------------------------------------- 1. parity with float64, Hermitian bits
@pytest.mark.parametrize("nstand,nsrc,nfine", SHAPES)
def test_parity_with_the_float64_restatement(nstand, nsrc, nfine):
    """A partial tile and one source; two tiles a side, the second ragged, and three sources (an odd k pair); two whole tiles and all
    32 sources; three tiles with a ragged last one and five sources; no model.  Random complex gains of modulus 0.5 to 2, stand 3
    flagged and holding NaN and Inf, (stand 5, pol 1) flagged, the input's upper triangle NaN.  Every word within five float gaps of
    the float64 restatement, the flagged rows and columns +0, the output Hermitian bit for bit."""
    tau, freq, flux, h, V = case(nstand, nsrc, nfine)
    ref = apply(V, h, freq, tau, flux)
    gap = float_gap(V, h, freq, tau, flux, ref=ref)
    bad = _upper_nan(V)
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    ca = CA(nstand, freq, tau, flux, h)
    got = ca.run(bad)
    ca.close()
    err = word_error(got, ref, scale(V, h, flux))
    print("calapply parity %d stands %d sources: float gap %.3g, bar %.3g, worst error %.3g = %.2f of the bar" % (nstand, nsrc, gap, 5 * gap, err.max(),
                                                                                                             err.max() / (5 * gap)))
    assert np.isfinite(got.view(np.float32)).all() and (err <= 5 * gap).all(), (err.max(), 5 * gap)
    assert hermitian_bits(got)
    assert all(_bits0(x) for x in (got[:, 3], got[:, :, :, 3], got[:, 5, 1], got[:, :, :, 5, 1]))


# ---------------------------------------------------------------- 2. exact cases
def test_unit_factors_without_a_model_copy_the_lower_triangle():
    """Unit factors (those of Initialize), nsrc = 0, no SetModel, the input's upper triangle NaN: the lower triangle is the input
    bit for bit, the upper its conjugate, the diagonal's imaginary parts +0 -- 70 stands: three tiles a side, the last ragged."""
    tau, freq, flux, h, V = case(70, 0, 1)
    n = 140
    ca = CA(70, freq, model=False)
    got = ca.run(_upper_nan(V)).reshape(1, n, n)
    ca.close()
    A = V.reshape(1, n, n)
    low = np.tril(np.ones((n, n), bool), -1)
    assert got[:, low].tobytes() == A[:, low].tobytes()
    assert got.transpose(0, 2, 1)[:, low].tobytes() == np.conj(A[:, low]).tobytes()
    d = np.einsum('cii->ci', got)
    assert d.real.tobytes() == np.einsum('cii->ci', A).real.tobytes() and _bits0(d.imag)


def test_factors_that_are_powers_of_two_scale_exactly():
    """h from {+-2^n, +-i 2^n}: h_i conj(h_j) V is exact in float32, so the output equals the float64 restatement exactly."""
    tau, freq, flux, h, V = case(35, 0, 2)
    rng = np.random.default_rng(5)
    h = (np.exp2(rng.integers(-3, 4, h.shape)) * (1j ** rng.integers(0, 4, h.shape))).astype(np.complex64)
    ca = CA(35, freq, h=h)
    got = ca.run(_upper_nan(V))
    ca.close()
    assert np.array_equal(got, apply(V, h)) and hermitian_bits(got)


def test_small_integers_with_unit_steering_are_exact():
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
    ca = CA(nstand, freq, np.zeros((nsrc, nstand)), flux)
    got = ca.run(_upper_nan(V))
    ca.close()
    exp = V.astype(np.complex128)
    for p in range(2):
        exp[:, :, p, :, p] -= flux.sum(axis=1)[:, None, None]
    assert np.array_equal(got, exp) and hermitian_bits(got)
    assert np.array_equal(got[:, :, 0, :, 1], V[:, :, 0, :, 1]) and np.array_equal(got[:, :, 1, :, 0], V[:, :, 1, :, 0])


# ---------------------------------------------------------------- 3. bit identity
def test_a_channel_alone_settings_back_and_forth_fresh_context_and_other_kernels_change_no_bit():
    """35 stands, 3 sources, 3 channels.  The middle channel alone in a context of its own: the corresponding words of the full run.
    The same call after SetFactors and SetModel to other values (which change the output) and back; in a fresh context; in a fresh
    context while X-engine contractions run on their streams and xengBeamformRun on this one."""
    nstand, nsrc, nfine = 35, 3, 3
    tau, freq, flux, h, V = case(nstand, nsrc, nfine, seed=41)
    h1, flux1 = np.roll(h, 5, axis=2), np.ascontiguousarray(flux[:, ::-1])
    ca = CA(nstand, freq, tau, flux, h)
    full = ca.run(V)
    assert np.isfinite(full.view(np.float32)).all()
    ca.set_factors(h1)
    other_h = ca.run(V)
    ca.set_factors(h)
    ca.set_model(tau, freq, flux1)
    other_m = ca.run(V)
    ca.set_model(tau, freq, flux)
    again = ca.run(V)
    ca.close()
    assert again.tobytes() == full.tobytes() and other_h.tobytes() != full.tobytes() and other_m.tobytes() != full.tobytes()
    ca = CA(nstand, freq[1:2], tau, flux[1:2], h[1:2])
    sub = ca.run(np.ascontiguousarray(V[1:2]))
    ca.close()
    assert sub.tobytes() == full[1:2].tobytes()
    bstand, bchan, btime, nbeam = 96, 8, 96, 4
    rng = np.random.default_rng(3)
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, bstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * bstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    ca = CA(nstand, freq, tau, flux, h)
    ca.upload(V)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(3):
            for q in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + q * xg.gulp_bytes, xg.out.ptr, int(q == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ca.enqueue()
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengCalapplySync")
            got.append(ca.result())
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    ca.close()
    ffi.call("xengBeamformDestroy")
    assert all(x.tobytes() == full.tobytes() for x in got)


# ---------------------------------------------------------------- 4. non-finite visibilities
def test_flagged_stands_holding_nan_are_the_stands_holding_zeros():
    """h = 0 in both polarisations of stands 9 and 33 (one in each tile), NaN and Inf all over their rows and columns, in the cross
    hands too: their rows and columns read +0, and the output is bit-identical to the run with zeros there."""
    nstand, nsrc, nfine = 35, 3, 2
    tau, freq, flux, h, V = case(nstand, nsrc, nfine, seed=51, flagged=(9, 33), half_flagged=())
    zeros, bad = V.copy(), V.copy()
    for s in (9, 33):
        zeros[:, s] = 0
        zeros[:, :, :, s] = 0
        bad[:, s] = np.nan
        bad[:, :, :, s] = np.inf
    ca = CA(nstand, freq, tau, flux, h)
    a, b = ca.run(zeros), ca.run(bad)
    ca.close()
    assert np.isfinite(a.view(np.float32)).all() and a.tobytes() == b.tobytes()
    assert all(_bits0(x) for s in (9, 33) for x in (a[:, s], a[:, :, :, s]))
    assert np.abs(a[:, 0, 0, 1, 0]).min() > 0


def test_nan_in_a_read_stand_stays_in_its_word_and_the_mirror():
    """A NaN in V[c = 1][11 1][4 1] (a word of the lower triangle): out[1][11 1][4 1] and its mirror out[1][4 1][11 1] are NaN, every
    other word is bit-identical to the clean run.  A NaN in the upper triangle, V[1][4 0][11 1], is not read: no word changes."""
    nstand, nsrc, nfine = 22, 3, 3
    tau, freq, flux, h, V = case(nstand, nsrc, nfine, seed=61)
    bad, upper = V.copy(), V.copy()
    bad[1, 11, 1, 4, 1] = np.nan
    upper[1, 4, 0, 11, 1] = np.nan
    ca = CA(nstand, freq, tau, flux, h)
    clean, got, same = ca.run(V), ca.run(bad), ca.run(upper)
    ca.close()
    assert np.isfinite(clean.view(np.float32)).all() and same.tobytes() == clean.tobytes()
    hit = np.zeros(V.shape, bool)
    hit[1, 11, 1, 4, 1] = hit[1, 4, 1, 11, 1] = True
    assert np.isnan(got[hit]).all() and got[~hit].tobytes() == clean[~hit].tobytes()


# ---------------------------------------------------------------- 5. the ABI
def test_info_tickets_and_argument_checks_with_and_without_a_context():
    """GetInfo; Run before SetModel is INVALID_STATE with sources and launches nothing; SetModel refuses non-finite words, negative
    fluxes and, with sources, null delays or fluxes; SetFactors non-finite words; they change nothing; tickets count from 1 after
    Initialize and every one is done after Sync; every INVALID_ARGUMENT of Initialize leaves a live context alone; after Destroy
    every call that needs a context is INVALID_STATE."""
    nstand, nsrc, nfine = 38, 2, 2
    tau, freq, flux, h, V = case(nstand, nsrc, nfine, seed=81)
    ca = CA(nstand, freq, tau, flux, model=False)
    assert _info() == (2, 3 * nfine, 2 * 32 * 17 * 8, nfine * (2 * nstand) ** 2 * 8)
    ca.upload(V)
    with pytest.raises(ffi.XengError) as ei:
        ca.enqueue()
    assert ei.value.status == INVALID_STATE
    ffi.call("xengCalapplySync")
    ca.result()                                 # (nothing was written)
    ca.set_model(tau, freq, flux)
    ca.set_factors(h)
    first = ca.run(V)
    f32 = np.ascontiguousarray(flux, np.float32)
    for bt, bf, bx in ((np.where(np.arange(tau.size).reshape(tau.shape) == 7, np.nan, tau), freq, f32), (tau, np.where(np.arange(nfine) == 1, np.inf, freq), f32),
                       (tau, freq, np.where(np.arange(4).reshape(2, 2) == 3, -1, f32)), (tau, freq, np.where(np.arange(4).reshape(2, 2) == 0, np.nan, f32))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCalapplySetModel", _dp(np.ascontiguousarray(bt, np.float64)), _dp(np.ascontiguousarray(bf, np.float64)), _fp(np.ascontiguousarray(bx, np.float32)))
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((None, _dp(freq), _fp(f32)), (_dp(tau), None, _fp(f32)), (_dp(tau), _dp(freq), None)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCalapplySetModel", *args)
        assert ei.value.status == INVALID_ARGUMENT
    for bad in (np.where(np.arange(nstand) == 2, np.nan, h), np.where(np.arange(nstand) == 7, complex(0, np.inf), h)):
        with pytest.raises(ffi.XengError) as ei:
            ca.set_factors(bad)
        assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengCalapplySetFactors", None)
    assert ei.value.status == INVALID_ARGUMENT
    assert ca.run(V).tobytes() == first.tobytes()
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    ffi.call("xengCalapplyMark", ctypes.byref(t))
    assert t.value == 1
    ca.enqueue()
    ffi.call("xengCalapplyMark", ctypes.byref(t))
    assert t.value == 2
    ffi.call("xengCalapplyWait", 2)
    ffi.call("xengCalapplySync")
    ca.result()
    for k in (1, 2):
        ffi.call("xengCalapplyTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, 3):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCalapplyWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, nfine, nsrc), (0, 513, nfine, nsrc), (0, nstand, 0, nsrc), (0, nstand, nfine, 33), (0, nstand, nfine, -1)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCalapplyInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info()[0] == 2
    out = ca.dout.ptr + GUARD
    for args in ((None, out), (ca.din.ptr, None), (ca.din.ptr + 8, out), (ca.din.ptr, out + 8)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCalapplyRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengCalapplySync")
    ca.result()
    ca.close()
    s, b = ctypes.c_int(), ctypes.c_longlong()
    for name, args in (("xengCalapplyRun", (4096, 4096)), ("xengCalapplySetModel", (_dp(tau), _dp(freq), _fp(f32))), ("xengCalapplySetFactors", (h.ctypes.data,)),
                       ("xengCalapplyGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(s), ctypes.byref(b))),
                       ("xengCalapplyMark", (ctypes.byref(t),)), ("xengCalapplyWait", (1,)), ("xengCalapplyTicketDone", (1, ctypes.byref(d))), ("xengCalapplySync", ()),
                       ("xengCalapplyCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCalapplyDestroy")


# ---------------------------------------------------------------- 6. closure through the existing engines
def test_closure_through_the_imager_and_the_solver():
    """35 stands, 2 channels: V = g g^H o (5 a_A a_A^H + 1 a_B a_B^H), the factors from the true g, source A subtracted -- what is
    left is the unit source B.  xengImageRun on the device's output reads, at B and at A, what it reads on the float64 restatement's
    matrix, within test_image_gpu.py's bar on that matrix (five float gaps of the imager's restatement) plus this kernel's own bar
    carried through norm * sum w_s w_t; xengGaincalRun on the output against B alone returns unit gains within test_gaincal_gpu.py's
    bar on that matrix (five float gaps of the solver's restatement)."""
    nstand, nfine, niter = 35, 2, 20
    rng, tau, freq, _, _, g = gaincal_ref.setup(301, nstand, 2, nfine, flagged=())
    flux = np.array([5.0, 1.0])
    V = corrupt(model(freq, tau, flux), g)
    h = factors(g)
    ref = apply(V, h, freq, tau[:1], flux[:1])
    gap = float_gap(V, h, freq, tau[:1], flux[:1], ref=ref)
    vbar = (5 * gap * scale(V, h, np.broadcast_to(flux[:1], (nfine, 1)))).reshape(V.shape)
    ref32 = np.ascontiguousarray(ref.astype(np.complex64))
    ca = CA(nstand, freq, tau[:1], flux[:1], h)
    got = ca.run(V)
    ca.close()
    print("closure: calapply float gap %.3g, worst word %.2f of the bar" % (gap, (word_error(got, ref, scale(V, h, np.broadcast_to(flux[:1], (nfine, 1)))) / (5 * gap)).max()))
    # the imager, pixels [B, A]
    w = np.ones(nstand, np.float32)
    tpix = np.ascontiguousarray(tau[::-1])
    im = IM(tpix, freq, 1)
    im.set_weights(w, False)
    a, b = im.run(got), im.run(ref32)
    im.close()
    sc = image_ref.scale(ref32, w, False, 1)
    A = image_ref.masked(vbar, w, False)
    carried = np.einsum('s,cspt,t->cp', w.astype(np.float64), A[:, :, [0, 1, 0, 0], :, [0, 1, 1, 1]].transpose(1, 2, 0, 3), w.astype(np.float64))[:, :, None] * image_norm(w, False, 1)
    igap = image_ref.float_gap(ref32, freq, tpix, w, False, 1)
    bar = 5 * igap * sc + carried
    d = np.abs(a.astype(np.float64) - b)
    print("closure: image at B %s, at A %s; worst difference %.3g of the bar (image float gap %.3g)" % (a[:, :2, 0].ravel(), a[:, :2, 1].ravel(), (d / bar).max(), igap))
    assert (d <= bar).all() and (np.abs(a[:, :2, 0] - 1) < 1e-4).all()
    # the solver, against B alone
    ggap = gaincal_ref.float_gap(ref32, freq, tau[1:], flux[1:], w, 0, niter)
    gc = GC(tau[1:], freq, flux[1:], w, 0, niter, 0.0)
    gains, stats = gc.run(got)
    gc.close()
    err = gaincal_ref.gain_error(gains, np.ones_like(gains))
    print("closure: gains |g - 1| worst %.3g, bar %.3g = %.2f of the bar" % (err.max(), 5 * ggap, err.max() / (5 * ggap)))
    assert (err <= 5 * ggap).all() and (stats[:, :, 2] == nstand).all()


# ---------------------------------------------------------------- 7. the chain on device rings
def test_source_to_upchan_corr_to_upchan_calapply_to_upchan_image_on_device_rings():
    """Source -> UpchanCorr (44 inputs, 2 coarse channels, nupchan 2, one gulp of 64 samples per integration) -> UpchanCalApply (2
    sources, one stand without a gain) -> UpchanImage (9 pixels) on device rings, two integrations: each calibrated span is within
    the bar of the float64 restatement of UpchanCorr's own output span and Hermitian bit for bit; each image is, bit for bit, what
    the stand-alone imager gives on the calibrated span; the headers say what was done."""
    nstand, nchan, g, N, nsrc, npix, seq0, sfreq, nint = 22, 2, 64, 2, 2, 9, 6400, 55e6, 2
    ninput, nfine = 2 * nstand, nchan * N
    rng = np.random.default_rng(91)
    pos, lmn, pix = random_array(rng, nstand, 1200.0, 5.0), sky(rng, nsrc), sky(rng, npix)
    flux = [50.0, 20.0]
    gains = rng.uniform(0.5, 2.0, (nfine, 2, nstand)) * np.exp(2j * np.pi * rng.uniform(size=(nfine, 2, nstand)))
    gains[:, :, 6] = 0
    vin = rng.integers(0, 256, (nint * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=sfreq)
    r0, r1, r2, r3 = Ring("f-engine", space="cuda"), Ring("uc-output", space="cuda"), Ring("calapply-output", space="cuda"), Ring("image-output", space="cuda")
    uc = UpchanCorr(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=g // N, gpu=0)
    cal = UpchanCalApply(LOG, r1, r2, pos, lmn, flux, gains=gains, gpu=0)
    img = UpchanImage(LOG, r2, r3, pos, pix, gpu=0)
    span = nfine * ninput * ninput * 8
    mid, out, sink = Sink(r1, span), Sink(r2, span), Sink(r3, nfine * 4 * npix * 4)
    run_blocks([uc, cal, img], Source(r0, [(hdr, vin.reshape(-1), g * nchan * ninput)]), [mid, out, sink])
    ok = ctypes.c_int()
    ffi.call("xengCalapplyCheckGuards", ctypes.byref(ok))
    ffi.call("xengCalapplyDestroy")
    ffi.call("xengImageDestroy")
    ffi.call("xengUpchanCorrDestroy")
    assert ok.value == 1
    (vh, _, vspans), = mid.sequences
    (ch, ctag, cspans), = out.sequences
    (ih, itag, ispans), = sink.sequences
    assert len(vspans) == len(cspans) == len(ispans) == nint and ctag == ch['seq0'] == seq0 == itag and cal.stats['napply'] == nint
    assert ch['calibrated'] is True and ch['nsubtracted'] == nsrc and 'nsrc' not in ch and ch['nfine'] == nfine and ih['npix'] == npix
    freq = vh['fine_sfreq'] + vh['fine_bw_hz'] * np.arange(nfine)
    tau, h = steering_delays(pos, lmn), factors(gains)
    F = np.broadcast_to(np.asarray(flux, np.float32), (nfine, nsrc))
    im = IM(steering_delays(pos, pix), freq, 1)
    for k in range(nint):
        V = np.ascontiguousarray(vspans[k]).view(np.uint8).reshape(-1).view(np.complex64).reshape(nfine, nstand, 2, nstand, 2)
        got = np.ascontiguousarray(cspans[k]).view(np.uint8).reshape(-1).view(np.complex64).reshape(nfine, nstand, 2, nstand, 2)
        ref = apply(V, h, freq, tau, F)
        gap = float_gap(V, h, freq, tau, F, ref=ref)
        err = word_error(got, ref, scale(V, h, F))
        print("chain integration %d: worst word %.2f of the bar" % (k, err.max() / (5 * gap)))
        assert (err <= 5 * gap).all() and hermitian_bits(got) and _bits0(got[:, 6]) and _bits0(got[:, :, :, 6])
        assert np.ascontiguousarray(ispans[k]).view(np.uint8).tobytes() == im.run(got).tobytes(), k
    im.close()
