"""BeamToa on the MI355X: xengToa* against the restatement (tests/toa_ref.py), byte for byte and with no tolerance -- the records,
the sub-band profiles, their harmonics, the correlation and the poison around them; which words are NaN is compared, a NaN's sign
and payload are not (the contract leaves them open).  The output sits between poisoned guard bands that are checked after every
call, the input is read back after every call and must be what was uploaded, the state's guards are checked at every close.  The
shapes are the smallest at which each mechanism can fail (the docstrings say which).  The harmonics and the correlation against the
float64 statement (blocks/toa.py toa_reference) within the a-priori bound; BeamFold -> BeamToa through rings on the device with a
planted pulsar.  No wall-clock assertions."""
import ctypes
import json
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamFold, BeamToa, subband_frequencies, toa_reference, toa_subbands, toa_tables, toa_template  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.dedisp import KDM  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import toa_cases, toa_ref  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, source_header, wait_for  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
EPS = 2.0 ** -24
_pf, _pb, _pi = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)


def _info(nsub):
    n, a, b, c, d = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    used = (ctypes.c_int * nsub)()
    ffi.call("xengToaGetInfo", ctypes.byref(n), used, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d))
    return n.value, list(used), a.value, b.value, c.value, d.value


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8).ctypes.data_as(_pb)


class TOA:
    """The xengToa context (one per process), an input buffer, the output between poisoned guard bands, and what the restatement
    needs beside it: every call goes to both and is compared byte for byte."""

    def __init__(self, c, nprod=None):
        self.c = c
        self.npair, self.nprod, self.nchg, self.nbin = c['X'].shape if nprod is None else (c['X'].shape[0], nprod) + c['X'].shape[2:]
        self.nsub, self.nharm, self.nlag = len(c['edges']) - 1, c['D'].shape[1], c['L'].shape[1]
        self.sizes = (self.npair, self.nsub, self.nbin, self.nharm, self.nlag)
        self.out_bytes = toa_ref.offsets(*self.sizes)[3]
        # the buffers come first, the context second: tests/test_accel_gpu.py says why
        self.din = ffi.DeviceBuffer(self.npair * self.nprod * self.nchg * self.nbin * 4)
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.out_bytes)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        ffi.call("xengToaInitialize", 0, self.npair, self.nprod, self.nchg, self.nbin, self.nsub, self.nharm, self.nlag)
        assert _info(self.nsub) == (0, [-1] * self.nsub) + toa_ref.offsets(*self.sizes)
        self.active = None
        self.set_all()

    def set_all(self):
        c = self.c
        self.edges, self.w = np.ascontiguousarray(c['edges'], np.int32), None if c['w'] is None else np.ascontiguousarray(c['w'], np.float32)
        ffi.call("xengToaSetBands", self.edges.ctypes.data_as(_pi), None if self.w is None else self.w.ctypes.data_as(_pf))
        w = np.ones(self.nchg) if self.w is None else self.w
        assert _info(self.nsub)[1] == [int(np.count_nonzero(w[self.edges[r]:self.edges[r + 1]])) for r in range(self.nsub)]
        self.D, self.L, self.S = (np.ascontiguousarray(c[k], np.float32) for k in 'DLS')
        ffi.call("xengToaSetTables", self.D.ctypes.data_as(_pf), self.L.ctypes.data_as(_pf))
        ffi.call("xengToaSetTemplate", self.S.ctypes.data_as(_pf))
        self.set_mask(c['off'])

    def set_mask(self, off):
        self.off = off
        ffi.call("xengToaSetMask", _u8(off))

    def set_active(self, active):
        self.active = active
        ffi.call("xengToaSetActive", _u8(active))

    def expected(self, X):
        return toa_ref.canonical(toa_ref.out_bytes(*toa_ref.toa(X, self.edges, self.w, self.D, self.L, self.S, self.off, self.active)), self.npair * (self.nsub + 1))

    def run(self, X, compare=True, enqueue_only=False):
        """The device's output bytes (NaNs canonical) after every check; compared with the restatement unless told not to."""
        sent = np.ascontiguousarray(X, np.float32)
        self.din.upload(sent)
        ffi.call("xengToaRun", self.din.ptr, self.dout.ptr + GUARD)
        if enqueue_only:
            return sent
        return self.result(sent, compare)

    def result(self, sent, compare=True):
        ffi.call("xengToaSync")
        assert self.din.download(np.uint8, sent.nbytes).tobytes() == sent.tobytes(), "the input was written"
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.out_bytes:] == POISON).all(), "bytes past the output were written"
        got = toa_ref.canonical(raw[GUARD:GUARD + self.out_bytes], self.npair * (self.nsub + 1))
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        if compare:
            exp = self.expected(sent)
            bad = np.flatnonzero(got != exp)
            a, b, c, _ = toa_ref.offsets(*self.sizes)
            assert bad.size == 0, "the output differs from byte %d on (%d bytes; P begins at %d, PH at %d, ccf at %d)" % (bad[0], bad.size, a, b, c)
        return got

    def split(self, got):
        return toa_ref.split_out(got, *self.sizes)

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengToaCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengToaDestroy")
        self.din.free()
        self.dout.free()


def first_case(nprod, seed=1):
    return toa_cases.case(seed, 2, nprod, 70, 100, toa_cases.EDGES, 33, 257)


@pytest.mark.parametrize("nprod", [1, 4])
def test_the_first_case_equals_the_restatement_byte_for_byte(nprod):
    """2 pairs x 70 groups in sub-bands [0, 9, 40, 70) (9, 30 and 29 used groups: batches of 8 with short last ones of 1, 6 and 5; NaN
    and Inf in groups 11 and 47, of weight 0) x 100 bins (16-byte loads, 25 threads of a scrunch work-group; base chains of 2 and 1
    bins, a run of 64 and one of 36) x 33 harmonics x 257 lags (a second correlation work-group of one lag); 8 rows: one full tile.
    Partial masks that differ per pair.  chi-squared data with a pulse, then integer data, then pair 1 inactive (nothing read, all
    +0, records {-1, 0, 0, 0})."""
    c = first_case(nprod)
    t = TOA(c)
    try:
        rec, P, PH, ccf = t.split(t.run(c['X']))
        assert np.isfinite(P).all() and np.isfinite(PH).all() and np.isfinite(ccf).all() and (rec['l'] >= 0).all() and (rec['var'] > 0).all()
        t.run(toa_cases.poison_unused(toa_cases.integer_scene(5, 2, nprod, 70, 100, top=20), c['edges'], c['w']))
        t.set_active(np.array([1, 0], np.uint8))
        rec, P, PH, ccf = t.split(t.run(c['X']))
        assert all(r.tolist() == (-1, 0.0, 0.0, 0.0) for r in rec[1]) and not P[1].any() and not PH[1].any() and not ccf[1].any() and (rec[0]['l'] >= 0).all()
        assert _info(3)[0] == 3
    finally:
        t.close()


@pytest.mark.parametrize("nprod,nchg,nbin,edges,nharm,nlag,kind,left_out", [
    (1, 70, 5, 3, 2, 1, 'full', toa_cases.LEFT_OUT),
    (4, 70, 64, 3, 31, 257, 'empty', toa_cases.LEFT_OUT),
    (1, 70, 68, 3, 33, 257, 'partial', toa_cases.LEFT_OUT),
    (4, 70, 100, 1, 33, 257, 'partial', toa_cases.LEFT_OUT),
    (1, 13, 100, 3, 33, 257, 'partial', toa_cases.LEFT_OUT),
    (4, 70, 100, 3, 33, 300, 'partial', toa_cases.LEFT_OUT),
    (1, 70, 100, [0, 9, 40, 70], 33, 257, 'partial', tuple(range(9, 40))),
], ids=["nbin5_nharm2_nlag1", "nbin64_nharm31_empty_mask", "nbin68", "nsub1", "nchg13_nsub3", "nlag300", "a_sub_band_of_weight_0"])
def test_the_other_paths(nprod, nchg, nbin, edges, nharm, nlag, kind, left_out):
    """nbin 5 with 2 harmonics and 1 lag: word loads, two threads (the second with one bin), one lag.  nbin 64 with 31 harmonics: one
    full run of the base chains, the most harmonics 64 bins allow; pair 0 has no off-pulse bin (base and var +0).  nbin 68: a base
    chain of 2 bins in four lanes only.  nsub 1: two rows a pair, a tile of 4 rows with 4 past the last.  nchg 13 with nsub 3:
    sub-bands of 4, 4 and 5 groups, a batch shorter than 8 everywhere (group 11 of weight 0).  nlag 300: a second work-group of 44
    lags.  A sub-band whose groups all have weight 0: its row is +0 with l = -1, and the band row is the sum of the other two."""
    c = toa_cases.case(nbin + nlag, 2, nprod, nchg, nbin, edges, nharm, nlag, kind, left_out)
    t = TOA(c)
    try:
        rec, P, PH, ccf = t.split(t.run(c['X']))
        assert np.isfinite(P).all() and np.isfinite(ccf).all()
        if kind == 'empty':
            assert not rec[0]['base'].any() and not rec[0]['var'].any() and rec[1]['var'].all() and (rec['l'] >= 0).all()
        if len(left_out) > 2:
            assert (rec[:, 1]['l'] == -1).all() and not P[:, 1].any() and not PH[:, 1].any() and not ccf[:, 1].any() and (rec[:, [0, 2, 3]]['l'] >= 0).all()
            assert np.array_equal(P[:, 3], (P[:, 0] + P[:, 2]).astype(np.float32))
        else:
            assert (rec['l'] >= 0).all()
    finally:
        t.close()


def test_a_nan_in_a_used_group_and_constant_data():
    """One NaN in a used group of sub-band 0 of pair 0, at an off-pulse bin: it stays in that row and the band row (base NaN, every
    PH and ccf word NaN, l = -1); sub-bands 1 and 2 equal the clean call's words.  The same NaN at a bin outside the mask: base and
    var stay finite, the harmonics are NaN all the same.  Constant data under weights of 1: every profile equals its mean exactly, d
    = 0, every ccf word is +0 and the tie goes to l = 0 with peak +0.  All equal the restatement (TOA.run compares)."""
    c = first_case(1, seed=9)
    t = TOA(c)
    try:
        clean = t.split(t.run(c['X']))
        b_off, b_on = int(np.flatnonzero(c['off'][0])[3]), int(np.flatnonzero(c['off'][0] == 0)[3])
        for b, base_nan in ((b_off, True), (b_on, False)):
            X = c['X'].copy()
            X[0, 0, 5, b] = np.nan
            rec, P, PH, ccf = t.split(t.run(X))
            assert rec[0]['l'].tolist() == [-1, clean[0][0, 1]['l'], clean[0][0, 2]['l'], -1] and np.isnan(PH[0, [0, 3]]).all() and np.isnan(ccf[0, [0, 3]]).all()
            assert np.flatnonzero(np.isnan(P[0, 0])).tolist() == [b] and np.isnan(rec[0, [0, 3]]['base']).all() == base_nan
            assert np.isnan(rec[0, [0, 3]]['base']).any() == base_nan and (rec[0, [0, 3]]['peak'] == 0).all()
            assert np.array_equal(ccf[0, 1:3], clean[3][0, 1:3]) and np.array_equal(ccf[1], clean[3][1]) and rec[1].tolist() == clean[0][1].tolist()
        c2 = dict(c, w=(c['w'] != 0).astype(np.float32))
        t.c = c2
        t.set_all()
        rec, P, PH, ccf = t.split(t.run(np.full((2, 1, 70, 100), 2.5, np.float32)))
        assert (rec['l'] == 0).all() and not rec['peak'].any() and not rec['var'].any() and not ccf.any() and not PH.any() and not np.signbit(ccf).any()
        assert P[0, :, 0].tolist() == [22.5, 75.0, 72.5, 170.0] and rec['base'][0].tolist() == [22.5, 75.0, 72.5, 170.0]
    finally:
        t.close()


def integer_case(nprod):
    """tests/test_toa_cpu.py's: integers 0..1, weights of 0 and 1, 16 off-pulse bins, D and S of -1, 0, 1 and the l = 0 column alone."""
    rng = np.random.default_rng(40 + nprod)
    edges = np.array([0, 4, 8, 13], np.int32)
    w = np.ones(13, np.float32)
    w[[5, 11]] = 0
    off = np.zeros((2, 20), np.uint8)
    off[0, :16], off[1, 2:18] = 1, 1
    X = toa_cases.poison_unused(toa_cases.integer_scene(7 + nprod, 2, nprod, 13, 20, top=2), edges, w)
    return dict(X=X, edges=edges, w=w, D=rng.integers(-1, 2, (20, 4, 2)).astype(np.float32), L=np.tile(np.array([1, 0], np.float32), (4, 1, 1)),
                S=rng.integers(-1, 2, (2, 4, 4, 2)).astype(np.float32), off=off)


@pytest.mark.parametrize("nprod", [1, 4])
def test_integer_data_with_the_l0_column_equals_the_float64_statement_exactly(nprod):
    """Integers 0..1 in 2 pairs x 13 groups x 20 bins, weights of 0 and 1, 16 off-pulse bins (the baseline is a multiple of 1/16),
    tables of -1, 0, 1 in D and S (the library takes any finite table) and the l = 0 column of the lag table alone, L = (1, 0):
    every float32 step is exact, so P, base, var, PH and ccf equal toa_reference's float64 values word for word."""
    c = integer_case(nprod)
    t = TOA(c)
    try:
        rec, P, PH, ccf = t.split(t.run(c['X']))
    finally:
        t.close()
    e = toa_reference(np.where(np.isfinite(c['X']), c['X'], 0), c['edges'], c['w'], c['D'], c['L'], c['S'], c['off'])
    for got, want in ((P, e['P']), (rec['base'], e['base']), (rec['var'], e['var']), (PH, e['PH']), (ccf, e['ccf'])):
        assert np.array_equal(got.astype(np.float64), want)
    assert rec['l'].tolist() == e['l'].tolist() and PH.any() and ccf.any()


def test_a_second_call_a_reset_a_fresh_context_and_other_kernels_beside_it_give_the_same_bytes():
    """The first case at nprod 4: a second call, a call after other data and a Reset, and a fresh context give the first call's
    bytes; so does a call enqueued between two xengBeamformRun on the same stream while X-engine contractions run on theirs
    (no packed fp32 in these kernels for MFMA traffic to disturb)."""
    c = first_case(4, seed=21)
    t = TOA(c)
    try:
        first = t.run(c['X'])
        assert t.run(c['X'], compare=False).tobytes() == first.tobytes()
        t.run(toa_cases.float_scene(22, 2, 4, 70, 100), compare=False)
        ffi.call("xengToaReset")
        assert _info(3)[0] == 0
        assert t.run(c['X'], compare=False).tobytes() == first.tobytes() and _info(3)[0] == 1
    finally:
        t.close()
    rng = np.random.default_rng(3)
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    t = TOA(c)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        assert t.run(c['X'], compare=False).tobytes() == first.tobytes()            # (a fresh context, alone)
        for g in range(4):
            ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
        ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
        sent = t.run(c['X'], enqueue_only=True)
        ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
        beside = t.result(sent, compare=False)
        ffi.call("xengXgpuSync")
        assert beside.tobytes() == first.tobytes()
    finally:
        xg.close()
        t.close()
        ffi.call("xengBeamformDestroy")
        for b in (bin_, bwt, bout):
            b.free()


def test_harmonics_and_correlation_are_within_the_a_priori_bound_of_the_float64_statement():
    """Every PH and ccf word of the first case (both nprod) against toa_reference in float64, within (n + c) 2^-24 sum |terms|.

    PH: n = nbin = 100 fmaf steps.  The terms are (A_b + mean_off A)|D[b][k]| with A_b = sum_g |w_g|(|X0| + |X1|) >= |P_b| and its
    off-pulse mean >= |base|, so that A_b + mean A >= |d_b|.  c counts the roundings behind d_b: a sub-band's chain of at most
    m = 30 fmaf, one add at nprod = 4 and the nsub = 3 adds of the band row (m + 1 + 3 = 34 on A_b); base adds to that its chains of
    ceil(100 / 64) = 2 adds, the 64 adds of the partials and the division (34 + 2 + 64 + 1 = 101 on mean A); d = fl(P - base) one
    more: c_d = 102, and 2 for the second-order terms of (1 + 2^-24)^202: c = 104.
    ccf: n = 2 nharm = 66 fmaf steps.  The terms are (E_re|sr| + E_im|si|)|L0| + (E_im|sr| + E_re|si|)|L1| with E the PH terms'
    sums (>= |re|, |im|).  c: the harmonics' own (100 + 104 = 204), the two roundings of a cross-spectrum word (2), and 2 for the
    second-order terms: c = 208."""
    worst = [0.0, 0.0]
    for nprod in (1, 4):
        c = first_case(nprod, seed=31)
        t = TOA(c)
        try:
            rec, P, PH, ccf = t.split(t.run(c['X']))
        finally:
            t.close()
        e = toa_reference(np.where(np.isfinite(c['X']), c['X'], 0.0), c['edges'], c['w'], c['D'], c['L'], c['S'], c['off'])
        bounds = ((100 + 104) * EPS * e['ph_scale'], (66 + 208) * EPS * e['ccf_scale'])
        for i, (got, want, bound) in enumerate(((PH, e['PH'], bounds[0]), (ccf, e['ccf'], bounds[1]))):
            err = np.abs(got.astype(np.float64) - want)
            worst[i] = max(worst[i], float((err / bound).max()))
            assert (bound > 0).all() and (err <= bound).all()
        assert rec['l'].tolist() == e['l'].tolist()
    print("toa: worst |PH - PH64| / bound = %.3g, worst |ccf - ccf64| / bound = %.3g" % tuple(worst))


def test_refusals():
    L = ffi.lib()
    L.xengToaDestroy()
    assert L.xengToaInitialize(0, 2, 1, 8, 16, 2, 4, 32) == 0
    try:
        buf = ffi.DeviceBuffer(1 << 16)
        e = np.array([0, 4, 8], np.int32)
        D, Lt, S = np.zeros((16, 4, 2), np.float32), np.zeros((4, 32, 2), np.float32), np.zeros((2, 3, 4, 2), np.float32)
        w = np.ones(8, np.float32)
        assert L.xengToaRun(buf.ptr, buf.ptr + 32768) == INVALID_STATE                      # (nothing set yet)
        assert L.xengToaSetBands(e.ctypes.data_as(_pi), w.ctypes.data_as(_pf)) == 0 and L.xengToaRun(buf.ptr, buf.ptr + 32768) == INVALID_STATE
        assert L.xengToaSetTables(D.ctypes.data_as(_pf), Lt.ctypes.data_as(_pf)) == 0 and L.xengToaRun(buf.ptr, buf.ptr + 32768) == INVALID_STATE
        for bad in ([0, 5, 4], [-1, 4, 8], [0, 4, 9]):
            assert L.xengToaSetBands(np.array(bad, np.int32).ctypes.data_as(_pi), None) == INVALID_ARGUMENT
        w[3] = np.inf
        assert L.xengToaSetBands(e.ctypes.data_as(_pi), w.ctypes.data_as(_pf)) == INVALID_ARGUMENT
        S[1, 2, 3, 1] = np.nan
        assert L.xengToaSetTemplate(S.ctypes.data_as(_pf)) == INVALID_ARGUMENT and L.xengToaRun(buf.ptr, buf.ptr + 32768) == INVALID_STATE
        S[1, 2, 3, 1] = 0
        D[3, 1, 0] = np.inf
        assert L.xengToaSetTables(D.ctypes.data_as(_pf), Lt.ctypes.data_as(_pf)) == INVALID_ARGUMENT
        assert L.xengToaSetTemplate(S.ctypes.data_as(_pf)) == 0 and _info(2)[1] == [4, 4]
        for a, b in ((None, buf.ptr), (buf.ptr, None), (buf.ptr + 4, buf.ptr + 32768), (buf.ptr, buf.ptr + 32768 + 8)):
            assert L.xengToaRun(a, b) == INVALID_ARGUMENT
        assert _info(2)[0] == 0
        ffi.call("xengMemset", buf.ptr, 0, buf.nbytes)
        assert L.xengToaRun(buf.ptr, buf.ptr + 32768) == 0
        t = ctypes.c_ulonglong()
        ffi.call("xengToaMark", ctypes.byref(t))
        ffi.call("xengToaWait", t.value)
        done = ctypes.c_int()
        ffi.call("xengToaTicketDone", t.value, ctypes.byref(done))
        assert done.value == 1 and _info(2)[0] == 1
        buf.free()
    finally:
        ffi.call("xengToaDestroy")


# ---------------------------------------------------------------- BeamFold -> BeamToa through rings
@pytest.mark.parametrize("space,stokes", [("cuda", "I"), ("cuda_host", "full")])
def test_fold_then_arrival_phases_through_rings_on_the_device(space, stokes):
    """2 pairs x 96 fine channels over 60 to 79.6 MHz, windows folded into 16 bins by a pulsar whose period is 16 windows (window n
    falls in bin n mod 16), pair 1 without a pulsar -- the shape of the BeamFold -> BeamRmSynth test.  The power beams carry the
    template (a wrapped Gaussian of sigma 1.5 bins) delayed by 0.2371 turns and dispersed by a DM error of 1e-5 pc cm^-3 (0.06 turns
    across the band; the pulsar list's DM is 0, so BeamFold rotates nothing), and normal noise of 0.3 per word.  BeamFold(nfscr=1)
    writes one cube per 4 spans of 16 windows at nprod 1 or 4; BeamToa (4 sub-bands, 5 harmonics, 64 lags) reads that ring in device
    space (directly) or in pinned host space (one staged copy per span).  The span equals the restatement fed the fold's own span
    byte for byte; the header's tau and dm_offset agree with what was planted within 5 Cramer-Rao errors -- each sub-band's
    sigma_F / (b sqrt(2 sum k^2 |S_k|^2)) / 2 pi from the planted noise (0.3 sqrt(2) / 2 per channel and bin after 4 hits, 24 channels),
    amplitude and template, carried through the straight-line fit -- and toa_s with the planted arrival time within the same error
    divided by f0."""
    npair, nchan, N, W, nwin, nbin, nsub, nspan = 2, 3, 32, 1, 16, 16, 4, 8
    tsub, nharm, nlag, tau, ddm, noise = 4, 5, 64, 0.2371, 1e-5, 0.3
    nfine = nchan * N
    chan_bw = 19.6e6 / nchan
    hdr = source_header(nchan, npair, 2, seq0=0, sfreq=60e6, chan_bw=chan_bw)
    hdr.update(nstand=npair, nbeam=npair, npol=2, complex=True, nbit=32, nupchan=N, nframe_sum=W, fine_bw_hz=chan_bw / N, fine_sfreq=60e6, pair0=0, acc_len=W * N)
    tsamp = W * N * nchan / hdr['bw_hz']
    f0 = 1.0 / (nbin * tsamp)
    pulsars = [dict(f0=f0, f1=0.0, pepoch=0.0, dm=0.0), None]
    freqs = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(nfine)
    x = toa_cases.planted_windows(77, nspan * nwin, npair, freqs, nbin, f0, (tau, 0.61), ddm, noise=noise)
    template = np.array([toa_cases.planted_template(nbin)] * npair)
    nprod = 1 if stokes == 'I' else 4
    r0, r1, r2 = Ring("toa-power", space="cuda"), Ring("toa-fold", space=space), Ring("toa-out", space="cuda_host")
    fold = BeamFold(LOG, r0, r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nbin=nbin, pulsars=pulsars, nsub=nsub, nfscr=1, stokes=stokes, gpu=0)
    toa = BeamToa(LOG, r1, r2, npair=npair, nchg=nfine, nbin=nbin, nsub=tsub, templates=template, nharm=nharm, nlag=nlag, gpu=0)
    cube_bytes = npair * nprod * nfine * nbin * 4
    sizes = (npair, tsub, nbin, nharm, nlag)
    sinks = [Sink(r1, cube_bytes), Sink(r2, toa_ref.offsets(*sizes)[3])]
    ths = [threading.Thread(target=blk.main, daemon=True) for blk in (fold, toa)]
    for t in sinks + ths:
        t.start()
    wait_for(lambda: len(r0._readers) >= 1 and len(r1._readers) >= 2 and len(r2._readers) >= 1, "the readers")
    src = Source(r0, [(hdr, x, nwin * npair * nfine * 16)])
    src.start()
    for t in [src] + ths + sinks:
        t.join(60)
        assert not t.is_alive(), "pipeline thread did not finish: %r" % (t,)
    cubes, outs = sinks[0].sequences, sinks[1].sequences
    assert len(cubes) == len(outs) == nspan // nsub
    edges = toa_subbands(nfine, tsub)
    D, L = toa_tables(nbin, nharm, nlag)
    S = toa_template(template, nharm, tsub)
    fr = subband_frequencies(freqs, edges)
    cr = [toa_cases.cramer_rao(S[0, r], 24.0, noise * np.sqrt(2.0) / 2 * np.sqrt(24.0), nbin) for r in range(tsub)]
    x_ref = KDM * f0 * (freqs.max() * 1e-6) ** -2
    dm_err, tau_err = toa_cases.line_errors(cr, KDM * f0 * (fr * 1e-6) ** -2, x_ref)
    a, b, cc, n = toa_ref.offsets(*sizes)
    for (ch, ctag, cspans), (oh, otag, ospans) in zip(cubes, outs):
        assert len(cspans) == len(ospans) == 1 and otag == ctag and ch['nprod'] == nprod and 'toa_nlag' not in ch
        assert (oh['toa_nsub'], oh['toa_nharm'], oh['toa_nlag'], oh['toa_edges']) == (tsub, nharm, nlag, edges.tolist()) and oh['nbin'] == nbin
        assert (oh['record_offset'], oh['profile_offset'], oh['harmonic_offset'], oh['ccf_offset'], oh['span_bytes']) == (0, a, b, cc, n)
        cube = cspans[0].view(np.float32).reshape(npair, nprod, nfine, nbin)
        exp = toa_ref.canonical(toa_ref.out_bytes(*toa_ref.toa(cube, edges, None, D, L, S, None, np.array([1, 0], np.uint8))), npair * (tsub + 1))
        got = toa_ref.canonical(ospans[0], npair * (tsub + 1))
        assert got.tobytes() == exp.tobytes()
        rec, P, PH, ccf = toa_ref.split_out(got, *sizes)
        assert (rec[0]['l'] >= 0).all() and all(r.tolist() == (-1, 0.0, 0.0, 0.0) for r in rec[1]) and not ccf[1].any()
        m = oh['toas'][0]
        t_mid = oh['subint_start'] * nchan / hdr['bw_hz'] + oh['subint_nwindow'] * tsamp / 2
        planted = (round(f0 * t_mid - tau - 0.5 / nbin) + tau + 0.5 / nbin) / f0
        dt = (m['tau'] - tau + 0.5) % 1 - 0.5
        print("BeamFold -> BeamToa (%s): tau error %.2f, dm_offset error %.2f, toa error %.2f Cramer-Rao errors (%.3g turns, %.3g pc cm^-3)"
              % (stokes, dt / tau_err, (m['dm_offset'] - ddm) / dm_err, (float(m['toa_s']) - planted) * f0 / tau_err, tau_err, dm_err))
        assert oh['toas'][1] is None and abs(dt) <= 5 * tau_err and abs(m['dm_offset'] - ddm) <= 5 * dm_err
        assert abs(float(m['toa_s']) - planted) <= 5 * tau_err / f0
    assert toa.stats['nsubint'] == nspan // nsub and toa.stats['ntoa'] == nspan // nsub
    assert json.dumps(outs[0][0])        # (the header is plain JSON)
