"""BeamCandFold on the MI355X: xengCandfold* against the restatement (tests/candfold_ref.py), byte for byte and with no tolerance:
the cube, the hits, the records and the best profiles of every completed segment, at the smallest shapes that can go wrong (bins a
period skips, periods longer than a segment, a period derivative, two candidates on one series, inactive and unset slots, a NaN
window, a dead series, odd nsub, one to eight widths, 4096 trials); bit identity across splits of a run over calls, after Reset
against a fresh context, and beside an X-engine contraction and xengBeamformRun; SetCandidates acting from the segment boundary; an
integer cube with equal maxima across trials, widths and bins; the ABI's refusals and tickets; and Source -> BeamDedisperse ->
BeamCandFold on device rings.  The output sits between two poisoned guard bands that are checked after every call, the input is
read back after every call and must be what was uploaded, the state's guards are checked at every close.  No wall-clock
assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import (BeamCandFold, BeamDedisperse, CANDFOLD_RECORD, as_records_candfold, candfold_gains, candfold_oscillators,  # noqa: E402
                                            candfold_trials, fold_phase)
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import candfold_ref  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
_pi, _pf = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
_pu64, _pi64, _pu8 = ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_ubyte)


def _info():
    n, k = ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengCandfoldGetInfo", ctypes.byref(n), ctypes.byref(k))
    return n.value, k.value


def _init(npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, g):
    d1, d2, g = np.ascontiguousarray(d1, np.int32), np.ascontiguousarray(d2, np.int32), np.ascontiguousarray(g, np.float32)
    ffi.call("xengCandfoldInitialize", 0, npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1.size, d1.ctypes.data_as(_pi), d2.ctypes.data_as(_pi),
             g.ctypes.data_as(_pf))


def _set(cands):
    """cands: (series, phi0, dphi, ddphi, active) each"""
    s = np.array([c[0] for c in cands], np.int32)
    a, b = np.array([c[1] for c in cands], np.uint64), np.array([c[2] for c in cands], np.uint64)
    d, on = np.array([c[3] for c in cands], np.int64), np.array([c[4] for c in cands], np.uint8)
    ffi.call("xengCandfoldSetCandidates", len(cands), s.ctypes.data_as(_pi), a.ctypes.data_as(_pu64), b.ctypes.data_as(_pu64), d.ctypes.data_as(_pi64),
             on.ctypes.data_as(_pu8))


def osc(period, f1=0.0, phase=0.0):
    """fold_phase for a period in windows (tsamp = 1), a derivative in turns per window^2 and a start phase in turns"""
    return fold_phase(1.0 / period, f1, -phase * period, 0.0, 1.0)


class CF:
    """The xengCandfold context (one per process), an input buffer, an output span between two poisoned guard bands, and the
    restatement beside it: every call goes to both, and every completed segment is compared byte for byte."""

    def __init__(self, npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains=None):
        self.shape = (npair, ndm, nprod)
        self.ncand_max, self.nbin, self.nsub, self.nt, self.nwin = ncand_max, nbin, nsub, nsub * nsubwin, nwin
        gains = candfold_gains(nbin, nwidth) if gains is None else np.asarray(gains, np.float32)
        # the buffers come first, the context second: tests/test_accel_gpu.py says why
        self.din = ffi.DeviceBuffer(nwin * npair * ndm * nprod * 4)
        self.nbytes = ncand_max * (16 + 4 * nbin)
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nbytes)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        _init(npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains)
        self.ref = candfold_ref.CandfoldRef(npair, ndm, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains)
        self.sent = None
        self.cubes = []                 # (cube bytes, hits bytes) of every segment completed

    def set(self, cands):
        _set(cands)
        self.ref.set_candidates(*zip(*cands))

    def reset(self):
        ffi.call("xengCandfoldReset")
        self.ref.reset()
        assert _info() == (0, 0)

    def enqueue(self, x, out=True):
        nc = x.shape[0]
        assert x.shape == (nc,) + self.shape
        self.sent = np.ascontiguousarray(x, np.float32)
        self.din.upload(self.sent)
        done = ctypes.c_int(-1)
        ffi.call("xengCandfoldRun", self.din.ptr, nc, self.dout.ptr + GUARD if out else None, ctypes.byref(done))
        assert done.value in (0, 1)
        return done.value

    def cube(self):
        cube, hits = np.empty((self.ncand_max, self.nsub, self.nbin), np.float32), np.empty((self.ncand_max, self.nsub, self.nbin), np.uint32)
        ffi.call("xengCandfoldGetCube", cube.ctypes.data_as(_pf), hits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
        return cube, hits

    def result(self, completed):
        """After a sync: the input is byte for byte what was uploaded; the span of a completing call (the poison is put back behind
        it), or None after having checked that a call which completed nothing left the poison in the output too; every byte before
        and after it must still be poison."""
        if self.sent is not None:
            assert self.din.download(np.uint8, self.sent.nbytes).tobytes() == self.sent.tobytes(), "the input was written"
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.nbytes:] == POISON).all(), "bytes past the best profiles were written"
        if not completed:
            assert (raw[GUARD:GUARD + self.nbytes] == POISON).all(), "a call that completed no segment wrote its output"
            return None
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + self.nbytes].copy()

    def run(self, x, sync=True):
        """One call, on the device and in the restatement; the span's bytes when it completed a segment."""
        done = self.enqueue(x)
        ffi.call("xengCandfoldSync")
        span = self.result(done)
        exp = self.ref.run(self.sent)
        assert (span is None) == (exp is None)
        if span is not None:
            cube, hits = self.cube()
            assert hits.tobytes() == self.ref.hits.tobytes(), "hits differ: %r" % (np.argwhere(hits != self.ref.hits)[:5],)
            assert cube.tobytes() == self.ref.cube.tobytes(), "the cube differs: %r" % (np.argwhere(cube.view(np.uint32) != self.ref.cube.view(np.uint32))[:5],)
            rec, prof = as_records_candfold(span, self.ncand_max, self.nbin)
            assert rec.tobytes() == exp[0].tobytes(), "records differ: %r / %r" % (rec, exp[0])
            assert prof.tobytes() == exp[1].tobytes(), "best profiles differ"
            self.cubes.append((cube.tobytes(), hits.tobytes()))
        return span

    def stream(self, x, sizes):
        spans, n = [], 0
        for nc in sizes:
            s = self.run(x[n:n + nc])
            if s is not None:
                spans.append(s.tobytes())
            n += nc
        assert n == x.shape[0]
        return spans

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengCandfoldCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengCandfoldDestroy")
        self.din.free()
        self.dout.free()


def _sizes(rng, total, nwin, fixed=None):
    out = []
    while total:
        nc = fixed if fixed else int(rng.integers(1, nwin + 1))
        out.append(min(total, nc))
        total -= out[-1]
    return out


def noise(rng, nwindows, npair, ndm, nprod):
    """powers of mean 55 and sigma 1 times a gain per series; with nprod = 4, XX and YY take half each and the cross terms are noise"""
    gain = rng.uniform(0.5, 1.5, (npair, ndm))
    if nprod == 1:
        return ((55 + rng.standard_normal((nwindows, npair, ndm))) * gain).astype(np.float32)[..., None]
    x = rng.standard_normal((nwindows, npair, ndm, 4)) * 100
    x[..., 0] = (27.5 + rng.standard_normal((nwindows, npair, ndm)) * 0.7) * gain
    x[..., 1] = (27.5 + rng.standard_normal((nwindows, npair, ndm)) * 0.7) * gain
    return x.astype(np.float32)


# ---------------------------------------------------------------- 1. the three shapes, word for word
def test_shape_a_skipped_bins_long_periods_a_derivative_shared_series_and_empty_slots():
    """nbin 16, nsub 2 x 37 windows, one width, nprod 4, 15 trials.  Candidates: a period of 5.3 windows (three bins a window:
    bins are skipped), one of 3000 windows (a segment stays in one bin), one with a period derivative, a second on the first one's series, an
    inactive one; slot 5 of 6 is unset.  Two and a half segments in calls of random sizes."""
    npair, ndm, nbin, nsub, nsubwin = 2, 3, 16, 2, 37
    nt = nsub * nsubwin
    rng = np.random.default_rng(1)
    x = noise(rng, 2 * nt + nt // 2, npair, ndm, 4)
    d1, d2 = candfold_trials(2, 1)
    cf = CF(npair, ndm, 50, 4, 6, nbin, nsub, nsubwin, 1, d1, d2)
    cf.set([(4,) + osc(5.3) + (1,), (1,) + osc(3000.0, phase=0.3) + (1,), (2,) + osc(11.7, f1=2e-5) + (1,), (4,) + osc(7.25, phase=0.5) + (1,),
            (0,) + osc(9.0) + (0,)])
    spans = cf.stream(x, _sizes(rng, x.shape[0], 50))
    assert len(spans) == 2 and _info() == (x.shape[0], 2)
    cube, hits = cf.cube()
    cf.close()
    rec, prof = as_records_candfold(np.frombuffer(spans[1], np.uint8), 6, nbin)
    assert (hits[1] > 0).sum() <= 2 * nsub and hits[:4].sum(axis=(1, 2)).tolist() == [nt] * 4
    assert (rec['it'][:4] >= 0).all() and (rec['iw'][:4] == 0).all()
    empty = np.array([candfold_ref.EMPTY] * 2, CANDFOLD_RECORD).tobytes()
    assert rec[4:].tobytes() == empty and not prof[4:].any() and not cube[4:].any() and not hits[4:].any()


def test_shape_b_odd_nsub_five_widths_a_nan_window_and_a_dead_series():
    """nbin 64, nsub 7 x 512 windows, five widths, 33 trials, nprod 1.  Series 2 has a NaN window: the NaN stays in its one cell of the cube; it
    is in the sum total_c of every trial's base, so the candidate has no score that is not NaN and its record is empty.  Series 3 is all zero: every score is +0, and the
    record names trial 0, width 0, bin 0."""
    npair, ndm, nbin, nsub, nsubwin = 1, 4, 64, 7, 512
    nt = nsub * nsubwin
    rng = np.random.default_rng(2)
    x = noise(rng, nt + 9, npair, ndm, 1)
    x[1234, 0, 2, 0] = np.nan
    x[:, 0, 3, 0] = 0.0
    n = np.arange(x.shape[0])
    x[:, 0, 1, 0] += 3.0 * (np.abs(((n / 100.37) % 1.0) - 0.5) < 0.02)
    d1, d2 = candfold_trials(5, 1)
    assert d1.size == 33
    cf = CF(npair, ndm, 1000, 1, 4, nbin, nsub, nsubwin, 5, d1, d2)
    cf.set([(0,) + osc(64.0) + (1,), (1,) + osc(100.37) + (1,), (2,) + osc(100.37) + (1,), (3,) + osc(33.3) + (1,)])
    (span,) = cf.stream(x, _sizes(rng, x.shape[0], 1000))
    cube, hits = cf.cube()
    cf.close()
    rec, prof = as_records_candfold(np.frombuffer(span, np.uint8), 4, nbin)
    assert np.isnan(cube[2]).sum() == 1 and tuple(rec[2]) == candfold_ref.EMPTY and not prof[2].any() and not np.isnan(np.delete(cube, 2, 0)).any()
    assert tuple(rec[3]) == (0.0, 0.0, 0, 0, 0, 0) and not np.signbit(rec['S'][3]) and not prof[3].any()
    assert rec['S'][1] > 2 * rec['S'][0] and (rec['S'] >= rec['S0']).all() and (rec['it'][:2] >= 0).all()


def test_shape_c_256_bins_4096_trials_and_a_full_table_of_candidates():
    """nbin 256, nsub 32 x 64 windows, eight widths, a 64 x 64 table of 4096 trials, ncand = ncand_max = 9."""
    npair, ndm, nbin, nsub, nsubwin = 3, 3, 256, 32, 64
    nt = nsub * nsubwin
    rng = np.random.default_rng(3)
    x = noise(rng, nt, npair, ndm, 1)
    i = np.arange(4096)
    d1, d2 = ((i % 64) - 32) * 24, ((i // 64) - 32) * 24
    cf = CF(npair, ndm, nt, 1, 9, nbin, nsub, nsubwin, 8, d1, d2)
    cf.set([(s,) + osc(20.0 + 37.77 * s, f1=1e-7 * (s - 4)) + (1,) for s in range(9)])
    (span,) = cf.stream(x, [nt])
    cf.close()
    rec, _ = as_records_candfold(np.frombuffer(span, np.uint8), 9, nbin)
    assert (rec['it'] >= 0).all() and (rec['S'] >= rec['S0']).all() and len(set(rec['it'].tolist())) > 1


# ---------------------------------------------------------------- 2. bit identity
SPLIT = dict(npair=2, ndm=5, nwin=50, nbin=32, nsub=3, nsubwin=40, nwidth=3)


def _split_cands():
    return [(7,) + osc(13.1) + (1,), (2,) + osc(400.0, phase=0.9) + (1,), (7,) + osc(2.5, f1=1e-4) + (1,), (9,) + osc(31.0) + (0,)]


def _split_cf(nprod):
    c = SPLIT
    d1, d2 = candfold_trials(3, 2)
    return CF(c['npair'], c['ndm'], c['nwin'], nprod, 5, c['nbin'], c['nsub'], c['nsubwin'], c['nwidth'], d1, d2)


@pytest.mark.parametrize("nprod", [1, 4])
def test_bit_identical_across_splits_reset_and_concurrent_kernels(nprod):
    """Two segments of 3 x 40 windows and 17 windows more: calls of one window, of 40 (every call ends on a sub-integration's last
    window, every third on the segment's), of 50 (the third straddles the segment's end), of 7 and a random split.  Each run
    follows a Reset -- the second one after 50 windows of another run's partial segment, which must leave no trace -- and gives the
    same spans, cubes and hits bit for bit, the following segment's included; so does a fresh context run while X-engine
    contractions and xengBeamformRun are in flight."""
    c = SPLIT
    nt = c['nsub'] * c['nsubwin']
    total = 2 * nt + 17
    rng = np.random.default_rng(7 + nprod)
    x = noise(rng, total, c['npair'], c['ndm'], nprod)
    splits = [[1] * total, [40] * (total // 40) + [total % 40], [50] * (total // 50) + [total % 50], [7] * (total // 7) + [total % 7], _sizes(rng, total, c['nwin'])]
    cf = _split_cf(nprod)
    cf.set(_split_cands())
    outs = []
    for i, sizes in enumerate(splits):
        if i == 1:
            assert cf.stream(100 + x[:50][::-1], [30, 20]) == []
        cf.reset()
        cf.cubes = []
        spans = cf.stream(x, sizes)
        assert len(spans) == 2 and _info() == (total, 2)
        outs.append((spans, cf.cubes))
    cf.close()
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    cf = _split_cf(nprod)
    cf.set(_split_cands())
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        spans, n = [], 0
        for nc in splits[2]:
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            done = cf.enqueue(x[n:n + nc])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengCandfoldSync")
            s = cf.result(done)
            if s is not None:
                spans.append(s.tobytes())
                cube, hits = cf.cube()
                cf.cubes.append((cube.tobytes(), hits.tobytes()))
            n += nc
        ffi.call("xengXgpuSync")
        outs.append((spans, cf.cubes))
    finally:
        xg.close()
    cf.close()
    ffi.call("xengBeamformDestroy")
    for o in outs[1:]:
        assert o == outs[0]
    assert outs[0][0][0] != outs[0][0][1]


def test_set_candidates_mid_segment_acts_from_the_boundary():
    """A set given 30 windows into segment 0 leaves that segment as it would have been, and folds segment 1 with m = 0 at its first
    window: segment 1 equals segment 0 of a fresh run of the same windows with the new set.  A set given exactly between two
    segments acts at once."""
    c = SPLIT
    nt = c['nsub'] * c['nsubwin']
    rng = np.random.default_rng(21)
    x = noise(rng, 3 * nt, c['npair'], c['ndm'], 1)
    new = [(3,) + osc(17.3, phase=0.25) + (1,), (7,) + osc(13.1) + (1,)]
    newer = [(1,) + osc(6.1) + (1,)]
    cf = _split_cf(1)
    cf.set(_split_cands())
    assert cf.stream(x[:30], [30]) == []
    cf.set(new)
    a, b = cf.stream(x[30:2 * nt], [50, 50, 50, 50, 10])
    cf.set(newer)                       # (the count stands on the boundary)
    (c2,) = cf.stream(x[2 * nt:], [50, 50, 20])
    cf.reset()
    cf.set(_split_cands())
    (a0,) = cf.stream(x[:nt], [50, 50, 20])
    cf.reset()
    cf.set(new)
    (b0,) = cf.stream(x[nt:2 * nt], [40, 40, 40])
    cf.reset()
    cf.set(newer)
    (c0,) = cf.stream(x[2 * nt:], [40, 40, 40])
    cf.close()
    assert a == a0 and b == b0 and c2 == c0 and a != b


# ---------------------------------------------------------------- 3. the tie rule, in integers
def test_integer_cube_with_equal_maxima_across_trials_widths_and_bins():
    """nbin 16, nsub 4 x 64 windows, a period of exactly 16 windows: every cell takes 4 windows, every sum is a small integer and every
    division is by 16.  Two equal pulses of 8 per window at bins 3 and 9 (twice that in the second series); the gains (6, 7) make
    the scores of width 1 at bins 3 and 9 and of width 2 at bins 2, 3, 8 and 9 equal.  Trials (64, 0), (1, 0), (0, 0), (-1, 0): the
    first smears the pulse over four bins, the second and fourth shift nothing and equal the third.  The record must name trial 1 (the first of the equal ones), width 0, bin 3, and S0 = S."""
    nbin, nsub, nsubwin = 16, 4, 64
    nt = nsub * nsubwin
    k = np.arange(nt)
    z = np.zeros(nt, np.float32)
    z[k % 16 == 3] = 8
    z[k % 16 == 9] = 8
    x = np.stack([z, 2 * z], axis=1).reshape(nt, 1, 2, 1)
    d1, d2 = [64, 1, 0, -1], [0, 0, 0, 0]
    cf = CF(1, 2, 100, 1, 3, nbin, nsub, nsubwin, 2, d1, d2, gains=[6.0, 7.0])
    o = (0, (1 << 64) // 16, 0)
    cf.set([(0,) + o + (1,), (1,) + o + (1,)])
    (span,) = cf.stream(x, [100, 100, 56])
    cf.close()
    rec, prof = as_records_candfold(np.frombuffer(span, np.uint8), 3, nbin)
    # p = 8 at bins 3 and 9, total 16; width 1: (8 - 1) * 6 = 42; width 2: (8 - 2) * 7 = 42 at bins 2, 3, 8 and 9
    assert tuple(rec[0]) == (42.0, 42.0, 1, 0, 3, 0) and tuple(rec[1]) == (84.0, 84.0, 1, 0, 3, 0)
    assert prof[0].tolist() == [8.0 if b in (3, 9) else 0.0 for b in range(16)]
    assert tuple(rec[2]) == candfold_ref.EMPTY


# ---------------------------------------------------------------- 4. the ABI
def test_refusals_completed_flag_and_calls_without_a_context():
    """Every INVALID_ARGUMENT of Initialize leaves a live context alone; Run before SetCandidates is INVALID_STATE; SetCandidates
    refuses a count outside 1..ncand_max, a series outside the table and null arrays; Run refuses nwin_call outside 1..nwin,
    misaligned or null pointers and a completing call without an output, with nothing launched and the count unchanged; GetCube
    before a segment has completed is INVALID_STATE; after Destroy every call that needs a context is."""
    d1, d2 = candfold_trials(1, 1)
    g = candfold_gains(16, 2)
    cf = CF(2, 4, 64, 1, 3, 16, 2, 40, 2, d1, d2)
    # (npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth)
    good = [2, 4, 64, 1, 3, 16, 2, 40, 2]
    for i, v in ((0, 0), (1, 0), (2, 0), (2, 81), (3, 2), (4, 0), (4, 4097), (5, 8), (5, 24), (5, 512), (6, 1), (6, 65), (7, 0), (7, 1 << 30), (8, 0), (8, 5)):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            _init(*args, d1, d2, np.resize(g, max(1, args[8])))
        assert ei.value.status == INVALID_ARGUMENT, args
    for bad in (dict(nbin=256, nsub=33), ):
        with pytest.raises(ffi.XengError) as ei:
            _init(2, 4, 64, 1, 3, bad['nbin'], bad['nsub'], 40, 2, d1, d2, g)       # nsub * nbin > 8192
        assert ei.value.status == INVALID_ARGUMENT
    for t1, t2, gg in (([(1 << 20) + 1], [0], g), ([0], [-(1 << 20) - 1], g), (d1, d2, [1.0, np.inf]), (d1, d2, [1.0, 0.0]), (d1, d2, [np.nan, 1.0]),
                       (np.zeros(4097), np.zeros(4097), g)):
        with pytest.raises(ffi.XengError) as ei:
            _init(*good, t1, t2, gg)
        assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengCandfoldInitialize", 0, *good, 1, None, None, None)
    assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        _init(1, 1, 64, 1, 4096, 256, 32, 64, 2, d1, d2, g)                     # two cubes and their hits, 512 MiB: above the state limit
    assert ei.value.status == INVALID_ARGUMENT
    assert _info() == (0, 0)                    # (the context is still there)
    comp = ctypes.c_int(-1)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengCandfoldRun", cf.din.ptr, 1, cf.dout.ptr, ctypes.byref(comp))
    assert ei.value.status == INVALID_STATE     # (no candidates yet)
    for cands in ([(8,) + osc(9.0) + (1,)], [(-1,) + osc(9.0) + (1,)], [(0,) + osc(9.0) + (1,)] * 4):
        with pytest.raises(ffi.XengError) as ei:
            _set(cands)
        assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengCandfoldSetCandidates", 1, None, None, None, None, None)
    assert ei.value.status == INVALID_ARGUMENT
    cf.set([(0,) + osc(9.0) + (1,)])
    for args in ((cf.din.ptr, 0, cf.dout.ptr), (cf.din.ptr, 65, cf.dout.ptr), (cf.din.ptr + 4, 1, cf.dout.ptr), (cf.din.ptr, 1, cf.dout.ptr + 8),
                 (None, 1, cf.dout.ptr)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCandfoldRun", *args, ctypes.byref(comp))
        assert ei.value.status == INVALID_ARGUMENT and _info() == (0, 0)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengCandfoldRun", cf.din.ptr, 1, cf.dout.ptr, None)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (0, 0)
    with pytest.raises(ffi.XengError) as ei:
        cf.cube()
    assert ei.value.status == INVALID_STATE
    rng = np.random.default_rng(5)
    x = noise(rng, 80, 2, 4, 1)
    assert cf.enqueue(x[:60], out=False) == 0
    ffi.call("xengCandfoldSync")
    assert cf.result(0) is None
    cf.ref.run(x[:60])
    with pytest.raises(ffi.XengError) as ei:
        cf.enqueue(x[60:], out=False)           # completes the segment: needs an output
    assert ei.value.status == INVALID_ARGUMENT and _info() == (60, 0)
    ffi.call("xengCandfoldSync")
    assert cf.result(0) is None
    assert cf.run(x[60:]) is not None and _info() == (80, 1)
    din, dout = cf.din.ptr, cf.dout.ptr
    f, u, s, n, t = np.zeros(96, np.float32), np.zeros(96, np.uint32), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_ulonglong()
    cf.close()
    one = (ctypes.c_int * 1)(0)
    for name, args in (("xengCandfoldRun", (din, 1, dout, ctypes.byref(s))), ("xengCandfoldReset", ()), ("xengCandfoldGetInfo", (ctypes.byref(n), ctypes.byref(n))),
                       ("xengCandfoldGetCube", (f.ctypes.data_as(_pf), u.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))),
                       ("xengCandfoldSetCandidates", (1, one, (ctypes.c_ulonglong * 1)(0), (ctypes.c_ulonglong * 1)(0), (ctypes.c_longlong * 1)(0),
                                                      (ctypes.c_ubyte * 1)(1))),
                       ("xengCandfoldMark", (ctypes.byref(t),)), ("xengCandfoldWait", (1,)), ("xengCandfoldTicketDone", (1, ctypes.byref(s))),
                       ("xengCandfoldSync", ()), ("xengCandfoldCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name


def test_completion_tickets_and_the_backend_methods():
    """xengCandfoldMark / Wait / TicketDone as the other engines'; the backend's candfold_* calls give the restatement's span."""
    from caltech_bifrost_dsp_amd.backend import HipBackend
    npair, ndm, nbin, nsub, nsubwin = 1, 3, 16, 2, 64
    nt = nsub * nsubwin
    rng = np.random.default_rng(11)
    x = noise(rng, nt, npair, ndm, 1)
    d1, d2 = candfold_trials(2, 0)
    g = candfold_gains(nbin, 3)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    outs = [ffi.DeviceBuffer(2 * (16 + 4 * nbin)) for _ in range(4)]
    be = HipBackend()
    assert be.candfold_initialize(0, npair, ndm, nt, 1, 2, nbin, nsub, nsubwin, 3, d1, d2, g) == 0
    cands = [(2,) + osc(10.7) + (1,), (0,) + osc(23.0) + (1,)]
    assert be.candfold_set_candidates(*zip(*cands)) == 0
    ref = candfold_ref.CandfoldRef(npair, ndm, 1, 2, nbin, nsub, nsubwin, 3, d1, d2, g)
    ref.set_candidates(*zip(*cands))
    tickets, done = [], ctypes.c_int(-1)
    for o in outs:
        rv, comp = be.candfold_run(din, nt, o)
        assert (rv, comp) == (0, 1)
        tickets.append(be.candfold_mark())
    assert tickets == [1, 2, 3, 4]
    be.candfold_wait(tickets[1])
    assert be.candfold_ticket_done(tickets[0]) and be.candfold_ticket_done(tickets[1])
    be.candfold_sync()
    assert be.candfold_ticket_done(tickets[-1]) and be.candfold_info() == (4 * nt, 4) and be.candfold_guards_intact()
    for bad in (0, tickets[-1] + 1):
        with pytest.raises(ffi.XengError):
            ffi.call("xengCandfoldTicketDone", bad, ctypes.byref(done))
        with pytest.raises(ffi.XengError):
            ffi.call("xengCandfoldWait", bad)
    with pytest.raises(ffi.XengError):
        ffi.call("xengCandfoldMark", None)
    for k, o in enumerate(outs):        # (m keeps running across the segments: every one folds at its own phase)
        assert o.download(np.uint8).tobytes() == ref.span(ref.run(x)), k
    cube, hits = be.candfold_cube(2, nsub, nbin)
    assert cube.tobytes() == ref.cube.tobytes() and hits.tobytes() == ref.hits.tobytes()
    be.candfold_reset()
    assert be.candfold_info() == (0, 0)
    ffi.call("xengCandfoldDestroy")
    din.free()
    for o in outs:
        o.free()


# ---------------------------------------------------------------- 5. the chain on device rings
def chain_case():
    """Dual-pol power beams [nwindows][2 pairs][4 x 8 fine channels][4] of values 0..49 with a pulse of 8 per channel in XX of pair
    1 every 16 windows, dispersed at trial 5 of 8; the header UpchanSumBeams writes.  The dedisperser's latency S = 10 windows
    makes the folder skip span 0 of 16 windows; a segment is 4 x 64 windows."""
    from tests.test_dedisp_cpu import header_table, power_header
    nchan, npair, N, W, nwin, nt, d0 = 4, 2, 8, 4, 16, 256, 5
    nfine = nchan * N
    dms = [float(d) for d in np.linspace(0.0, 0.14, 8)]
    hdr = power_header(nchan, npair, N, W, seq0=4096)
    table, tsamp = header_table(hdr, nfine, dms)
    S = int(table.max())
    nspan = -(-S // nwin) + nt // nwin + 1
    rng = np.random.default_rng(99)
    x = rng.integers(0, 50, (nspan * nwin, npair, nfine, 4)).astype(np.float32)
    for t in range(2, nspan * nwin - S, 16):
        x[t + table[d0], 1, np.arange(nfine), 0] += 8
    return dict(nchan=nchan, npair=npair, N=N, W=W, nwin=nwin, nt=nt, nspan=nspan, d0=d0, nfine=nfine, dms=dms, hdr=hdr, S=S, tsamp=tsamp, x=x)


def test_chain_source_dedisperse_cand_fold_on_device_rings():
    """Source -> BeamDedisperse -> BeamCandFold with three candidates at 16 windows: the planted (pair, trial), the same trial of the
    other pair and a far trial of the planted pair.  The one span of the output ring equals a direct run of xengCandfoldRun on the
    spans BeamDedisperse wrote, bit for bit; its sequence begins at the first span past the dedisperser's partial sums; on_folded
    receives the planted candidate alone, at the unrefined trial."""
    c = chain_case()
    npair, nwin, nt, ndm, nbin, nsub = c['npair'], c['nwin'], c['nt'], len(c['dms']), 16, 4
    period = 16 * c['tsamp']
    cands = [dict(pair=1, idm=c['d0'], period=period), dict(pair=0, idm=c['d0'], period=period), dict(pair=1, idm=0, freq=1.0 / period)]
    r0, r1, r2 = Ring("ub-output", space="cuda"), Ring("dd-output", space="cuda"), Ring("cf-output", space="cuda_host")
    got = []
    dd = BeamDedisperse(LOG, r0, r1, npair=npair, nchan=c['nchan'], nupchan=c['N'], nwin=nwin, dms=c['dms'], gpu=0)
    cf = BeamCandFold(LOG, r1, r2, npair=npair, ndm=ndm, nwin=nwin, ncand_max=4, nbin=nbin, nsub=nsub, nsubwin=nt // nsub, nwidth=2, ndrift=2, ncurve=1,
                      candidates=cands, threshold=8.0, on_folded=got.extend, gpu=0)
    ospan = 4 * (16 + 4 * nbin)
    mid, sink = Sink(r1, nwin * npair * ndm * 4), Sink(r2, ospan)
    run_blocks([dd, cf], Source(r0, [(c['hdr'], c['x'], nwin * npair * c['nfine'] * 16)]), [mid, sink])
    (dh, _, dspans), = mid.sequences
    (hd, tag, spans), = sink.sequences
    acc_len = c['W'] * c['N']
    skipped = -(-c['S'] // nwin)
    assert skipped == 1 and len(dspans) == c['nspan'] and len(spans) == 1
    assert tag == hd['seq0'] == 4096 + skipped * nwin * acc_len
    assert (hd['ncand'], hd['ncand_max'], hd['nbin'], hd['nsub'], hd['nsubwin'], hd['nwidth'], hd['profile_offset']) == (3, 4, nbin, nsub, nt // nsub, 2, 4 * 16)
    d1, d2 = candfold_trials(2, 1)
    assert hd['d1'] == d1.tolist() and hd['d2'] == d2.tolist() and [(k['pair'], k['idm']) for k in hd['candidates']] == [(1, c['d0']), (0, c['d0']), (1, 0)]
    assert [k['cand'] for k in got] == [0] and got[0]['snr'] > 8 and (got[0]['d1'], got[0]['d2']) == (0, 0) and got[0]['width'] == 1
    assert abs(got[0]['period'] - period) < 1e-9 * period
    assert cf.stats['nfolded'] == 1 and cf.stats['nstartup'] == skipped and cf.stats['nsegment_done'] == 1 and cf.stats['ndropped'] == 0
    # a direct run on the dedispersed spans with the block's own oscillators
    oscs = candfold_oscillators(cands, nt * c['tsamp'] / 2, c['tsamp'], nt)
    direct = CF(npair, ndm, nwin, 1, 4, nbin, nsub, nt // nsub, 2, d1, d2)
    direct.set([(o['pair'] * ndm + o['idm'], o['phi0'], o['dphi'], o['ddphi'], 1) for o in oscs])
    out = direct.stream(np.concatenate([sp.view(np.float32).reshape(nwin, npair, ndm, 1) for sp in dspans[skipped:]]), [nwin] * (c['nspan'] - skipped))
    direct.close()
    assert len(out) == 1 and out[0] == spans[0].tobytes()
