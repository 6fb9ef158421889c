"""UpchanPredict on the MI355X: xengPredict* against the restatement (tests/predict_ref.py).  Parity with the float64 restatement for
cross 0 and 1 and both modes; the exact cases (small integers, no filled record, cross = 0 leaving the cross hands alone); bit identity
of the Hermitian pairs, of a channel group alone, under a larger ncomp_max, of an empty record against a C = 0 record, after
SetComponents and SetMode back and forth, in a fresh context and beside an X-engine contraction and xengBeamformRun; a NaN in a word
that is read; the ABI with and without a context; agreement with xengCalapplyRun; the major cycle closed on the device through
xengImageRun and xengCleanRun; TbfSource -> Copy -> UpchanCorr -> UpchanImage -> UpchanClean, then UpchanPredict -> UpchanImage on
device rings.  The output sits between two poisoned 64 KiB guard bands that are checked after every call, the state's guards at every
close.  No wall-clock assertions.

The bar of the parity tests is not a constant: it is five times the worst gap between the float32 (kernel-order) and the float64
evaluation of the restatement ON THE TEST'S OWN INPUTS (tests/predict_ref.py float_gap), per word as |out - ref| / (max|V| + sum_k
(|C_XX| + |C_YY| + 2 |C_Re + i C_Im|)) of the word's channel.  Measured here on the CPU with numpy 2.2 (an array of 1.2 km, so phases of
hundreds of turns): gaps of 2.7e-8 to 4.0e-8 in subtract mode and 2.1e-8 to 1.3e-7 in model mode; the kernel's source on host threads
(tests/test_predict_emul_cpu.py) reaches 0.09 to 0.22 of the bar.  Measured on the MI355X: see MEASURED below."""
import ctypes
import json
import os
import struct
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import (Copy, TbfSource, UpchanClean, UpchanCorr, UpchanImage, UpchanPredict, clean_components, clean_layout,  # noqa: E402
                                            component_visibilities, steering_delays)
from caltech_bifrost_dsp_amd.blocks.imaging import CLEAN_COMPONENT  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import calapply_ref, clean_ref, image_ref  # noqa: E402
from tests.calapply_ref import hermitian_bits  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.image_ref import random_array  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.predict_ref import MODEL, SUBTRACT, case, float_gap, integer_case, predict, records, scale, upper_nan, word_error  # noqa: E402
from tests.test_calapply_gpu import CA  # noqa: E402
from tests.test_clean_gpu import CL  # noqa: E402
from tests.test_image_gpu import IM  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
# (nstand, ncomp, nfine, nfavg): one ragged tile and an odd last record; two tiles and groups; full tiles and two trips of the loop
# (PR_PAIRS = 8 record pairs per trip); three tiles; one record more than a trip
SHAPES = [(22, 1, 2, 1), (35, 3, 4, 2), (64, 32, 2, 1), (70, 5, 3, 3), (40, 17, 2, 1)]
# worst word error / bar over test_parity_with_the_float64_restatement on the MI355X, per (nstand, ncomp), the worst of cross 0, 1 and both modes
MEASURED = {(22, 1): 0.20, (35, 3): 0.16, (64, 32): 0.22, (70, 5): 0.22, (40, 17): 0.20}
# (worst errors 3.2e-8 to 7.5e-8; agreement with CalApply: 0.17 and 0.19 of the two bars, all 9800 words equal; the major cycle on the device: 0.02 of the bar
# without autos, 0.03 with; the chain on device rings 0.20 of the bar, its closure 0.01)


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _info():
    t, g, l, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    b, s, n = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengPredictGetInfo", ctypes.byref(t), ctypes.byref(g), ctypes.byref(l), ctypes.byref(b), ctypes.byref(s), ctypes.byref(n), ctypes.byref(m))
    return t.value, g.value, l.value, b.value, s.value, n.value, m.value


class PR:
    """The xengPredict context (one per process), an input buffer and the output of one call between two poisoned guard bands."""

    def __init__(self, tau, freq, nfavg, ncomp_max, cross, comps=None, geometry=True):
        self.ndir, self.nstand = tau.shape
        self.nfine, self.nfavg, self.ncomp_max = len(freq), nfavg, ncomp_max
        ffi.call("xengPredictInitialize", 0, self.nstand, self.nfine, nfavg, self.ndir, ncomp_max, int(cross))
        if geometry:
            ffi.call("xengPredictSetGeometry", _dp(np.ascontiguousarray(tau, np.float64)), _dp(np.ascontiguousarray(freq, np.float64)))
        if comps is not None:
            self.set_components(comps)
        self.nout = self.nfine * (2 * self.nstand) ** 2 * 8
        self.din = ffi.DeviceBuffer(self.nout)
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nout)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        self.model = False

    def set_components(self, comps):
        comps = np.ascontiguousarray(comps)
        assert comps.shape == (self.nfine // self.nfavg, self.ncomp_max) and comps.dtype == CLEAN_COMPONENT
        ffi.call("xengPredictSetComponents", comps.ctypes.data)

    def set_mode(self, mode):
        ffi.call("xengPredictSetMode", mode)
        self.model = mode == MODEL

    def upload(self, V):
        assert V.shape == (self.nfine, self.nstand, 2, self.nstand, 2) and V.dtype == np.complex64
        self.din.upload(np.ascontiguousarray(V))

    def enqueue(self):
        ffi.call("xengPredictRun", None if self.model else self.din.ptr, self.dout.ptr + GUARD)

    def result(self):
        """After a sync: the output (the poison is put back); every byte before it and past it must still be poison."""
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.nout:] == POISON).all(), "bytes past the output were written"
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + self.nout].copy().view(np.complex64).reshape(self.nfine, self.nstand, 2, self.nstand, 2)

    def run(self, V=None):
        if V is not None:
            self.upload(V)
        self.enqueue()
        ffi.call("xengPredictSync")
        return self.result()

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengPredictCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengPredictDestroy")
        self.din.free()
        self.dout.free()


def _bits0(x):
    return bool((np.ascontiguousarray(x).view(np.uint32) == 0).all())


def _cross_low(nfine, nstand):
    """the cross-hand words of the lower triangle, bool [nfine][n][n]"""
    n = 2 * nstand
    m = np.tril(np.ones((n, n), bool), -1) & np.tile(np.array([[False, True], [True, False]]), (nstand, nstand))
    return np.broadcast_to(m[None], (nfine, n, n))


# ---------------------------------------------------------------- 1. parity with float64, Hermitian bits
@pytest.mark.parametrize("nstand,ncomp,nfine,nfavg", SHAPES)
def test_parity_with_the_float64_restatement(nstand, ncomp, nfine, nfavg):
    """Components of either sign on all four words, empty records that hold NaN in the middle, a repeated pixel, a list per group,
    the input's upper triangle NaN; cross 0 and 1, both modes (in model mode the input is NULL).  Every word within five float gaps
    of the float64 restatement, the output Hermitian bit for bit; with cross = 0 the cross-hand words of the lower triangle are the
    input's bit for bit (model mode: +0)."""
    tau, freq, comps, V = case(nstand, ncomp, nfine, nfavg)
    bad = upper_nan(V)
    n = 2 * nstand
    worst = 0.0
    for cross in (1, 0):
        pr = PR(tau, freq, nfavg, ncomp, cross, comps)
        pr.upload(bad)
        for mode in (SUBTRACT, MODEL):
            ref = predict(V, freq, tau, comps, nfavg, cross, mode)
            gap = float_gap(V, freq, tau, comps, nfavg, cross, mode, ref=ref)
            pr.set_mode(mode)
            got = pr.run()
            err = word_error(got, ref, scale(None if mode == MODEL else V, comps, nfavg))
            print("predict parity %d stands %d records cross %d mode %d: float gap %.3g, bar %.3g, worst error %.3g = %.2f of the bar"
                  % (nstand, ncomp, cross, mode, gap, 5 * gap, err.max(), err.max() / (5 * gap)))
            worst = max(worst, err.max() / (5 * gap))
            assert np.isfinite(got.view(np.float32)).all() and (err <= 5 * gap).all(), (err.max(), 5 * gap)
            assert hermitian_bits(got)
            if not cross:
                m = _cross_low(nfine, nstand)
                x = got.reshape(nfine, n, n)[m]
                assert _bits0(x) if mode == MODEL else x.tobytes() == V.reshape(nfine, n, n)[m].tobytes()
        pr.close()
    print("predict parity %d stands %d records: worst %.2f of the bar" % (nstand, ncomp, worst))


# ---------------------------------------------------------------- 2. exact cases
def test_small_integers_with_unit_steering_are_exact():
    """Gaussian-integer V, tau = 0 (a = 1), integer components of either sign and an empty record: every product reads V - sum C
    exactly; with cross = 0 the parallel hands do and the cross hands are the input's -- 35 stands and 5 records in 7: two tiles, an
    odd record count."""
    nstand, ncomp, nfine, nfavg = 35, 5, 2, 1
    V, comps, exp = integer_case(nstand, ncomp, nfine, nfavg, 7)
    freq, tau = 50e6 + 12e3 * np.arange(nfine), np.zeros((4, nstand))
    pr = PR(tau, freq, nfavg, 7, 1, comps)
    got = pr.run(upper_nan(V))
    pr.close()
    assert np.array_equal(got, exp) and hermitian_bits(got)
    pr = PR(tau, freq, nfavg, 7, 0, comps)
    got0 = pr.run(upper_nan(V))
    pr.close()
    assert all(np.array_equal(got0[:, :, p, :, p], exp[:, :, p, :, p]) for p in range(2)) and hermitian_bits(got0)
    m = _cross_low(nfine, nstand)
    assert got0.reshape(nfine, 70, 70)[m].tobytes() == V.reshape(nfine, 70, 70)[m].tobytes()


def test_no_filled_record_copies_the_lower_triangle():
    """The records of Initialize (all empty), the input's upper triangle NaN: the lower triangle is the input bit for bit, the upper
    its conjugate, the diagonal's imaginary parts +0 -- 70 stands: three tiles a side, the last ragged; then the same after
    SetComponents with empty records whose other words hold NaN."""
    tau, freq, comps, V = case(70, 2, 1, 1)
    n = 140
    pr = PR(tau, freq, 1, 3, 1)
    first = pr.run(upper_nan(V))
    empty = records(1, 3)
    empty['C'], empty['I'] = np.nan, np.nan
    pr.set_components(empty)
    again = pr.run()
    assert _info()[5] == 0
    pr.close()
    got = first.reshape(1, n, n)
    A = V.reshape(1, n, n)
    low = np.tril(np.ones((n, n), bool), -1)
    assert got[:, low].tobytes() == A[:, low].tobytes() and again.tobytes() == first.tobytes()
    assert got.transpose(0, 2, 1)[:, low].tobytes() == np.conj(A[:, low]).tobytes()
    d = np.einsum('cii->ci', got)
    assert d.real.tobytes() == np.einsum('cii->ci', A).real.tobytes() and _bits0(d.imag)


# ---------------------------------------------------------------- 3. bit identity
def _same_up_to_zero_signs(a, b):
    """bit for bit, up to the sign of a zero"""
    a, b = np.ascontiguousarray(a).view(np.float32), np.ascontiguousarray(b).view(np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())


def test_a_group_alone_trailing_empties_settings_back_and_forth_fresh_context_and_other_kernels_change_no_bit():
    """35 stands, 5 records, 6 channels in groups of 2.  The middle group alone in a context of its own: the corresponding words of the
    full run.  ncomp_max 21 (a second trip of the loop that is never entered) with trailing empties; an empty record in place of a
    record with C = 0: the same bits up to the sign of a zero.  The same call after SetComponents and SetMode to other values (which
    change the output) and back; in a fresh context; in a fresh context while X-engine contractions run on their streams and
    xengBeamformRun on this one."""
    nstand, ncomp, nfine, nfavg = 35, 5, 6, 2
    tau, freq, comps, V = case(nstand, ncomp, nfine, nfavg, seed=41)
    other = comps.copy()
    other['C'][:, 0] *= -0.5
    pr = PR(tau, freq, nfavg, ncomp, 1, comps)
    full = pr.run(V)
    assert np.isfinite(full.view(np.float32)).all()
    pr.set_components(other)
    other_c = pr.run()
    pr.set_components(comps)
    pr.set_mode(MODEL)
    other_m = pr.run()
    pr.set_mode(SUBTRACT)
    again = pr.run()
    pr.close()
    assert again.tobytes() == full.tobytes() and other_c.tobytes() != full.tobytes() and other_m.tobytes() != full.tobytes()
    pr = PR(tau, freq[2:4], nfavg, ncomp, 1, comps[1:2])
    sub = pr.run(np.ascontiguousarray(V[2:4]))
    pr.close()
    assert sub.tobytes() == full[2:4].tobytes()
    wide = records(nfine // nfavg, 21)
    wide[:, :ncomp] = comps
    pr = PR(tau, freq, nfavg, 21, 1, wide)
    padded = pr.run(V)
    zero = wide.copy()
    zero['C'][:, 3] = 0                         # record 3 filled, with C = 0 ...
    pr.set_components(zero)
    with_zero = pr.run()
    zero['pixel'][:, 3] = -1                    # ... and empty
    pr.set_components(zero)
    with_empty = pr.run()
    pr.close()
    assert _same_up_to_zero_signs(padded, full) and _same_up_to_zero_signs(with_zero, with_empty) and with_zero.tobytes() != full.tobytes()
    bstand, bchan, btime, nbeam = 96, 8, 96, 4
    rng = np.random.default_rng(3)
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, bstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * bstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    pr = PR(tau, freq, nfavg, ncomp, 1, comps)
    pr.upload(V)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(3):
            for q in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + q * xg.gulp_bytes, xg.out.ptr, int(q == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            pr.enqueue()
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengPredictSync")
            got.append(pr.result())
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    pr.close()
    ffi.call("xengBeamformDestroy")
    assert all(x.tobytes() == full.tobytes() for x in got)


# ---------------------------------------------------------------- 4. non-finite visibilities
def test_nan_in_an_input_word_stays_in_its_word_and_the_mirror():
    """A NaN in V[c = 1][11 1][4 0] (a cross-hand word of the lower triangle): out[1][11 1][4 0] and its mirror out[1][4 0][11 1] are
    NaN, every other word is bit-identical to the clean run.  A NaN in the upper triangle, V[1][4 0][11 1], is not read: no word
    changes."""
    nstand, ncomp, nfine, nfavg = 22, 3, 3, 1
    tau, freq, comps, V = case(nstand, ncomp, nfine, nfavg, seed=61)
    bad, upper = V.copy(), V.copy()
    bad[1, 11, 1, 4, 0] = np.nan
    upper[1, 4, 0, 11, 1] = np.nan
    pr = PR(tau, freq, nfavg, ncomp, 1, comps)
    clean, got, same = pr.run(V), pr.run(bad), pr.run(upper)
    pr.close()
    assert np.isfinite(clean.view(np.float32)).all() and same.tobytes() == clean.tobytes()
    hit = np.zeros(V.shape, bool)
    hit[1, 11, 1, 4, 0] = hit[1, 4, 0, 11, 1] = True
    assert np.isnan(got[hit]).all() and got[~hit].tobytes() == clean[~hit].tobytes()


# ---------------------------------------------------------------- 5. the ABI
def test_info_tickets_and_argument_checks_with_and_without_a_context():
    """GetInfo; Run before SetGeometry is INVALID_STATE and launches nothing; SetGeometry refuses NULL and non-finite words;
    SetComponents NULL, a pixel outside [-1, ndir) and a non-finite word of a filled record (not of an empty one); SetMode an unknown
    mode; they change nothing; tickets count from 1 after Initialize and every one is done after Sync; every INVALID_ARGUMENT of
    Initialize leaves a live context alone; after Destroy every call that needs a context is INVALID_STATE."""
    nstand, ncomp, nfine, nfavg = 38, 4, 4, 2
    tau, freq, comps, V = case(nstand, ncomp, nfine, nfavg, seed=81)
    ndir = tau.shape[0]
    pr = PR(tau, freq, nfavg, ncomp, 1, geometry=False)
    state = 2 * ncomp * 32 + (nfine + ndir * nstand) * 8 + 2 * 4
    assert _info() == (2, 3 * nfine, 2 * 32 * 17 * 8, nfine * (2 * nstand) ** 2 * 8, (state + 15) & ~15, 0, SUBTRACT)
    pr.upload(V)
    with pytest.raises(ffi.XengError) as ei:
        pr.enqueue()
    assert ei.value.status == INVALID_STATE
    ffi.call("xengPredictSync")
    pr.result()                                 # (nothing was written)
    ffi.call("xengPredictSetGeometry", _dp(tau), _dp(freq))
    pr.set_components(comps)
    assert _info()[5] == int((comps['pixel'] >= 0).sum())
    first = pr.run(V)
    for bt, bf in ((np.where(np.arange(tau.size).reshape(tau.shape) == 7, np.nan, tau), freq), (tau, np.where(np.arange(nfine) == 1, np.inf, freq))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPredictSetGeometry", _dp(np.ascontiguousarray(bt, np.float64)), _dp(np.ascontiguousarray(bf, np.float64)))
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((None, _dp(freq)), (_dp(tau), None)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPredictSetGeometry", *args)
        assert ei.value.status == INVALID_ARGUMENT
    for field, k, value in (('pixel', 0, ndir), ('pixel', 2, -2), ('C', 0, np.nan), ('C', 3, np.inf)):
        bad = comps.copy()
        assert bad['pixel'][1, k] >= 0
        if field == 'C':
            bad['C'][1, k, 2] = value
        else:
            bad['pixel'][1, k] = value
        with pytest.raises(ffi.XengError) as ei:
            pr.set_components(bad)
        assert ei.value.status == INVALID_ARGUMENT, (field, k)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengPredictSetComponents", None)
    assert ei.value.status == INVALID_ARGUMENT
    for mode in (-1, 2):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPredictSetMode", mode)
        assert ei.value.status == INVALID_ARGUMENT
    assert pr.run().tobytes() == first.tobytes() and _info()[6] == SUBTRACT
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    ffi.call("xengPredictMark", ctypes.byref(t))
    assert t.value == 1
    pr.enqueue()
    ffi.call("xengPredictMark", ctypes.byref(t))
    assert t.value == 2
    ffi.call("xengPredictWait", 2)
    ffi.call("xengPredictSync")
    pr.result()
    for k in (1, 2):
        ffi.call("xengPredictTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, 3):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPredictWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, nfine, nfavg, ndir, ncomp, 1), (0, 513, nfine, nfavg, ndir, ncomp, 1), (0, nstand, 0, nfavg, ndir, ncomp, 1), (0, nstand, nfine, 3, ndir, ncomp, 1),
                 (0, nstand, nfine, 0, ndir, ncomp, 1), (0, nstand, nfine, nfavg, 0, ncomp, 1), (0, nstand, nfine, nfavg, (1 << 24) + 1, ncomp, 1),
                 (0, 512, nfine, nfavg, 1 << 20, ncomp, 1), (0, nstand, nfine, nfavg, ndir, 0, 1), (0, nstand, nfine, nfavg, ndir, 4097, 1), (0, nstand, nfine, nfavg, ndir, ncomp, 2)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPredictInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info()[0] == 2
    out = pr.dout.ptr + GUARD
    for args in ((None, out), (pr.din.ptr, None), (pr.din.ptr + 8, out), (pr.din.ptr, out + 8)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPredictRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    ffi.call("xengPredictSync")
    pr.result()
    pr.close()
    s, b = ctypes.c_int(), ctypes.c_longlong()
    cc = np.ascontiguousarray(comps)
    for name, args in (("xengPredictRun", (4096, 4096)), ("xengPredictSetGeometry", (_dp(tau), _dp(freq))), ("xengPredictSetComponents", (cc.ctypes.data,)),
                       ("xengPredictSetMode", (MODEL,)),
                       ("xengPredictGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(s), ctypes.byref(b), ctypes.byref(b), ctypes.byref(b), ctypes.byref(s))),
                       ("xengPredictMark", (ctypes.byref(t),)), ("xengPredictWait", (1,)), ("xengPredictTicketDone", (1, ctypes.byref(d))), ("xengPredictSync", ()),
                       ("xengPredictCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengPredictDestroy")


# ---------------------------------------------------------------- 6. agreement with xengCalapplyRun
def test_agreement_with_calapply_on_a_model_it_can_express():
    """35 stands, 7 sources, 2 channels, C_XX = C_YY = F >= 0, cross = 0, unit factors in xengCalapplyRun: the two float64
    restatements are the same matrix, and each device output lies within its own bar of it.  (Bit equality is not required: CalApply
    multiplies F a from stored words.)"""
    nstand, nsrc, nfine = 35, 7, 2
    tau, freq, flux, h, V = calapply_ref.case(nstand, nsrc, nfine, flagged=(), half_flagged=())
    ones = np.ones_like(h)
    comps = records(nfine, nsrc)
    comps['pixel'] = np.arange(nsrc)[None]
    comps['C'][:, :, 0] = comps['C'][:, :, 1] = flux
    ref = predict(V, freq, tau, comps, 1, 0)
    cref = calapply_ref.apply(V, ones, freq, tau, flux)
    assert np.abs(ref - cref).max() <= 1e-12 * np.abs(ref).max()
    pr = PR(tau, freq, 1, nsrc, 0, comps)
    got = pr.run(V)
    pr.close()
    ca = CA(nstand, freq, tau, flux, ones)
    cgot = ca.run(V)
    ca.close()
    gap, cgap = float_gap(V, freq, tau, comps, 1, 0, ref=ref), calapply_ref.float_gap(V, ones, freq, tau, flux, ref=cref)
    err, cerr = word_error(got, ref, scale(V, comps, 1)), calapply_ref.word_error(cgot, ref, calapply_ref.scale(V, ones, flux))
    print("predict %.2f of its bar, calapply %.2f of its bar, words that differ between the two: %d of %d"
          % (err.max() / (5 * gap), cerr.max() / (5 * cgap), int((got != cgot).sum()), got.size))
    assert (err <= 5 * gap).all() and (cerr <= 5 * cgap).all()


# ---------------------------------------------------------------- 7. the major cycle closes on the device
def _closure(V, freq, tau, w, autos, nfavg, dirty, comps, stats, gain, second, residual):
    """|second image - Clean's residual| over (max|dirty| + sum|C|) per word, and the bar in the same unit: the image test's bar on V
    (five float gaps of the imager's restatement, against its scale), the clean test's bar on the device's dirty image and pixels
    (five float gaps of Clean's restatement), and this engine's bar (five float gaps of its restatement against its scale) carried
    through norm * sum w_s w_t = 1 / nfavg per channel.  Returns (difference, bar), both [ngroup][4][npix] in units of the scale."""
    ngroup = len(freq) // nfavg
    sc = clean_ref.scale(dirty, comps)
    ibar = 5 * image_ref.float_gap(V, freq, tau, w, autos, nfavg) * image_ref.scale(V, w, autos, nfavg)
    pixels = [list(comps['pixel'][g, :stats['ncomp'][g]]) for g in range(ngroup)]
    ref, rcomps, rstats, _ = clean_ref.clean(dirty, freq, tau, w, autos, nfavg, None, comps.shape[1], gain, pixels=pixels)
    cbar = 5 * clean_ref.float_gap(dirty, freq, tau, w, autos, nfavg, ref, rcomps, rstats, gain) * sc
    pbar = 5 * float_gap(V, freq, tau, comps, nfavg, 1) * scale(V, comps, nfavg).reshape(ngroup, nfavg).mean(axis=1)[:, None, None]
    d = np.abs(second.astype(np.float64) - residual.astype(np.float64))
    return d / sc, np.broadcast_to((ibar + cbar + pbar) / sc, d.shape)


@pytest.mark.parametrize("autos", [False, True])
def test_major_cycle_closes_on_the_device(autos):
    """35 stands, 300 pixels, 4 channels in groups of 2, two point sources in noise: xengImageRun -> xengCleanRun (niter 8, gain 0.5)
    -> xengPredictRun with the span's own component area -> xengImageRun.  The second image is Clean's residual, in all four words,
    within the sum of the three engines' bars."""
    nstand, npix, nfine, nfavg, niter, gain = 35, 300, 4, 2, 8, 0.5
    c = clean_ref.case(nstand, npix, nfine, nfavg, autos)
    V, freq, tau, w = c['V'], c['freq'], c['tau'], c['w']
    im = IM(tau, freq, nfavg)
    im.set_weights(w, autos)
    dirty = im.run(V)
    cl = CL(c, niter)
    residual, comps, stats = cl.run(dirty, niter, gain)
    cl.close()
    assert (stats['ncomp'] == niter).all()
    pr = PR(tau, freq, nfavg, niter, 1, comps)
    out = pr.run(V)
    pr.close()
    second = im.run(out)
    im.close()
    d, bar = _closure(V, freq, tau, w, autos, nfavg, dirty, comps, stats, gain, second, residual)
    print("major cycle autos %d: worst word %.3g of the scale = %.2f of the bar; the residual's peak %.3g of the dirty image's"
          % (autos, d.max(), (d / bar).max(), np.abs(residual).max() / np.abs(dirty).max()))
    assert np.isfinite(second).all() and (d <= bar).all(), (d / bar).max()
    # and the host helper says the same of the float64 matrix
    M = component_visibilities(freq, tau, comps, nfavg)
    host = image_ref.image(V - M, freq, tau, w, autos, nfavg)
    assert (np.abs(host - residual) / clean_ref.scale(dirty, comps) <= bar).all()


# ---------------------------------------------------------------- 8. the chain on device rings
def _vis(span, nfine, nstand):
    return np.ascontiguousarray(span).view(np.uint8).reshape(-1).view(np.complex64).reshape(nfine, nstand, 2, nstand, 2)


def test_tbf_file_to_upchan_clean_and_its_components_into_upchan_predict_on_device_rings(tmp_path):
    """TbfSource (host ring) -> Copy (device ring) -> UpchanCorr (44 inputs, 2 coarse channels, nupchan 2, one gulp of 64 samples per
    integration) -> UpchanImage (9 pixels, groups of two fine channels) -> UpchanClean (niter 4, gain 0.5) on device rings, two
    integrations; then UpchanCorr's spans -> UpchanPredict, fed the first Clean span's records by set_components -> UpchanImage.
    Every predicted span is within the bar of the float64 restatement and Hermitian bit for bit; every second image is, bit for bit,
    the stand-alone imager's on the predicted span; the second image of the first integration is its Clean residual within the sum
    of the three bars; the header says what was done."""
    nstand, nchan, g, N, npix, nfavg, seq0, nint, niter, gain = 22, 2, 64, 2, 9, 2, 6400, 2, 4, 0.5
    ninput, nfine = 2 * nstand, nchan * N
    ngroup = nfine // nfavg
    rng = np.random.default_rng(91)
    pos, lmn = random_array(rng, nstand, 1200.0, 5.0), clean_ref.sky(rng, npix)
    w = np.ones(nstand, np.float32)
    vin = rng.integers(0, 256, (nint * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=55e6)
    hdr['seq'] = seq0
    path = os.path.join(str(tmp_path), "lwa-dump-1.00.tbf.0")
    hjson = json.dumps(hdr).encode()
    with open(path, "wb") as fh:
        assert len(hjson) <= 1024 - 8
        fh.write(struct.pack('<II', len(hjson), 1024) + hjson)
        fh.write(b"\0" * (1024 - 8 - len(hjson)))
        fh.write(vin.tobytes())
    rh, rd, ru, ri, rc = (Ring("tbf", space="system"), Ring("tbf-gpu", space="cuda"), Ring("uc-output", space="cuda"), Ring("image-output", space="cuda"),
                          Ring("clean-output", space="cuda"))
    src = TbfSource(LOG, rh, [path], ntime_gulp=g)
    cp = Copy(LOG, rh, rd, ntime_gulp=g, nbyte_per_time=nchan * ninput)
    uc = UpchanCorr(LOG, rd, ru, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=g // N, gpu=0)
    img = UpchanImage(LOG, ru, ri, pos, lmn, nfavg=nfavg, weights=w, autos=False, gpu=0)
    cb = UpchanClean(LOG, ri, rc, pos, lmn, niter, gain=gain, weights=w, gpu=0)
    span, nimg, (co, so, nspan) = nfine * ninput * ninput * 8, ngroup * 4 * npix * 4, clean_layout(ngroup, niter, npix)
    mid, dirt, sink = Sink(ru, span), Sink(ri, nimg), Sink(rc, nspan)
    ths = [threading.Thread(target=b.main, daemon=True) for b in (src, cp, uc, img, cb)]
    for s in (mid, dirt, sink):
        s.start()
    for t in ths[::-1]:
        t.start()
    for t in ths + [mid, dirt, sink]:
        t.join(60)
        assert not t.is_alive()
    for name in ("xengCleanDestroy", "xengImageDestroy", "xengUpchanCorrDestroy"):
        ffi.call(name)
    (vh, _, vspans), = mid.sequences
    (_, _, dspans), = dirt.sequences
    (_, _, cspans), = sink.sequences
    assert len(vspans) == len(dspans) == len(cspans) == nint
    comps, stats, residual = clean_components(cspans[0], ngroup, niter, npix)
    assert (stats['ncomp'] == niter).all()
    # the second pass: the same visibilities, Clean's records taken out
    r1, r2, r3 = Ring("uc-again", space="cuda"), Ring("predict-output", space="cuda"), Ring("image-again", space="cuda")
    prd = UpchanPredict(LOG, r1, r2, pos, lmn, nfavg=nfavg, ncomp_max=niter + 2, gpu=0)
    prd.set_components(comps)
    img2 = UpchanImage(LOG, r2, r3, pos, lmn, nfavg=nfavg, weights=w, autos=False, gpu=0)
    out, sink2 = Sink(r2, span), Sink(r3, nimg)
    run_blocks([prd, img2], Source(r1, [(vh, np.concatenate([np.ascontiguousarray(s).view(np.uint8).reshape(-1) for s in vspans]), span)]), [out, sink2])
    ok = ctypes.c_int()
    ffi.call("xengPredictCheckGuards", ctypes.byref(ok))
    ffi.call("xengPredictDestroy")
    ffi.call("xengImageDestroy")
    assert ok.value == 1
    (ph, ptag, pspans), = out.sequences
    (ih, itag, ispans), = sink2.sequences
    assert len(pspans) == len(ispans) == nint and ptag == ph['seq0'] == seq0 == itag and prd.stats['npredict'] == nint and prd.stats['ngap'] == 0
    assert (ph['ncomponents'], ph['nsubtracted'], ph['predict_mode'], ph['nfine']) == (niter, niter, 'subtract', nfine) and ih['npix'] == npix
    freq = vh['fine_sfreq'] + vh['fine_bw_hz'] * np.arange(nfine)
    tau = steering_delays(pos, lmn)
    im = IM(tau, freq, nfavg)
    im.set_weights(w, False)
    for k in range(nint):
        V, got = _vis(vspans[k], nfine, nstand), _vis(pspans[k], nfine, nstand)
        ref = predict(V, freq, tau, comps, nfavg, 1)
        gap = float_gap(V, freq, tau, comps, nfavg, 1, ref=ref)
        err = word_error(got, ref, scale(V, comps, nfavg))
        print("chain integration %d: worst word %.2f of the bar" % (k, err.max() / (5 * gap)))
        assert (err <= 5 * gap).all() and hermitian_bits(got)
        assert np.ascontiguousarray(ispans[k]).view(np.uint8).tobytes() == im.run(got).tobytes(), k
    im.close()
    dirty, second = dspans[0].view(np.float32).reshape(ngroup, 4, npix), ispans[0].view(np.float32).reshape(ngroup, 4, npix)
    d, bar = _closure(_vis(vspans[0], nfine, nstand), freq, tau, w, False, nfavg, dirty, comps, stats, gain, second, residual)
    print("chain closure: worst word %.2f of the bar" % (d / bar).max())
    assert (d <= bar).all()
