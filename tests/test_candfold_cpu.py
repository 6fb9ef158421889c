"""BeamCandFold without a GPU: the integer shift rule against Python's big integers (exact halves, negative numerators, odd nsub,
its symmetries), the trial table, the oscillators against fold_phase (an accelerated candidate included), a planted drifting pulse
train on the restatement (tests/candfold_ref.py) and what candfold_refined makes of its record, the tie rule on an integer cube,
NaN cells, empty and inactive slots, the NEWEST_ENGINES row under the per-row checks of tests/test_engine_table_cpu.py, the C entry
points' argument checks, and the block on CPU rings with a backend that serves xengCandfold* by the restatement -- window counting,
the start-up skip, a gap, the `candidates` command's timing, the header, the constructor's refusals."""
import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import (CANDFOLD_RECORD, BeamCandFold, as_records_candfold, candfold_candidates, candfold_gains, candfold_oscillators,
                                            candfold_refined, candfold_shifts, candfold_sigma, candfold_trials, fold_phase)
from caltech_bifrost_dsp_amd.blocks.accel_search import C_LIGHT
from caltech_bifrost_dsp_amd.ring import Ring
from tests import candfold_ref, test_engine_table_cpu
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_pulse_cpu import dedisp_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*


# ---------------------------------------------------------------- the shift rule
def _shift_big(d1, d2, s, nsub):
    """r = floor(x + 1/2), x = N / D exactly, in Python's integers and Fractions"""
    u = 2 * s + 1 - nsub
    x = Fraction(d1 * u * nsub + 2 * d2 * u * u, 32 * nsub * nsub)
    return (x + Fraction(1, 2)).__floor__()


@pytest.mark.parametrize("nsub", [2, 3, 7, 16, 63, 64])
def test_shifts_equal_big_integer_arithmetic(nsub):
    """Random trials up to the limit of 2^20, the limits themselves, and trials whose quotients are exact halves with either sign
    (d1 = +-16 nsub at u = +-1, even nsub; d1 = +-8 nsub at u = +-2, odd nsub; d2 = +-8 nsub^2 at odd u): numpy's int64 floor
    division is the rule."""
    rng = np.random.default_rng(nsub)
    d1 = np.concatenate([rng.integers(-(1 << 20), (1 << 20) + 1, 200), [1 << 20, -(1 << 20), 0, 1, -1, 16, -16, 8 * nsub, -8 * nsub, 16 * nsub, -16 * nsub, 0, 0]])
    d2 = np.concatenate([rng.integers(-(1 << 20), (1 << 20) + 1, 200), [-(1 << 20), 1 << 20, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8 * nsub * nsub, -8 * nsub * nsub]])
    r = candfold_shifts(d1, d2, nsub)
    assert r.dtype == np.int64 and r.shape == (d1.size, nsub)
    halves = neg = 0
    for t in range(d1.size):
        for s in range(nsub):
            u = 2 * s + 1 - nsub
            N, D = int(d1[t]) * u * nsub + 2 * int(d2[t]) * u * u, 32 * nsub * nsub
            assert int(r[t, s]) == _shift_big(int(d1[t]), int(d2[t]), s, nsub) == (2 * N + D) // (2 * D)
            halves += (2 * N) % (2 * D) == D
            neg += N < 0
    assert neg > 100 and halves >= 4
    assert np.array_equal(candfold_shifts(d1, d2, nsub, 64), r % 64) and (candfold_shifts(d1, d2, nsub, 64) >= 0).all()


def test_exact_halves_round_up_with_either_sign():
    """nsub = 2, u = -1, +1, D = 128: N = 2 d1 u + 2 d2.  d1 = 32: x = -1/2 and +1/2 -> r = 0 and 1 (half up, not away from zero)."""
    assert candfold_shifts([32], [0], 2).tolist() == [[0, 1]]
    assert candfold_shifts([-32], [0], 2).tolist() == [[1, 0]]
    assert candfold_shifts([0], [-32], 2).tolist() == [[0, 0]] and candfold_shifts([0], [32], 2).tolist() == [[1, 1]]
    assert candfold_shifts([96], [0], 2).tolist() == [[-1, 2]]


@pytest.mark.parametrize("nsub", [2, 5, 16, 33])
def test_symmetries_of_the_shifts(nsub):
    """With d2 = 0 the numerator is odd in d1 and in u, so exactly r(-d1, 0)(s) = r(d1, 0)(nsub - 1 - s).  Against the negated shift
    the half-up rule shows: r(-d1, 0)(s) = -r(d1, 0)(s) where the quotient N / D is not an exact half, and -r(d1, 0)(s) + 1 where
    it is (floor(-x + 1/2) = -floor(x + 1/2) + 1 exactly when x + 1/2 is whole).  With d1 = 0 the shifts are even in u:
    r(0, d2)(s) = r(0, d2)(nsub - 1 - s)."""
    d = np.concatenate([np.arange(-40, 41) * 8, [12345, 1 << 20]])
    z = np.zeros_like(d)
    pos, neg = candfold_shifts(d, z, nsub), candfold_shifts(-d, z, nsub)
    assert np.array_equal(neg, pos[:, ::-1])
    u = 2 * np.arange(nsub) + 1 - nsub
    half = (2 * (d[:, None] * u[None, :] * nsub)) % (64 * nsub * nsub) == 32 * nsub * nsub
    assert np.array_equal(neg, -pos + half) and (half.any() or nsub in (5, 33))
    bow = candfold_shifts(z, d, nsub)
    assert np.array_equal(bow, bow[:, ::-1])
    # the meaning: d1 sixteenths of a bin across the segment, d2 at either end
    assert candfold_shifts([16 * 12], [0], 64)[0, [0, -1]].tolist() == [-6, 6] and candfold_shifts([0], [16 * 6], 64)[0, [0, 32, -1]].tolist() == [6, 0, 6]


def test_trial_table_order_and_bounds():
    d1, d2 = candfold_trials(16, 8)
    assert d1.dtype == d2.dtype == np.int32 and d1.size == 33 * 17 and (d1[0], d2[0]) == (0, 0)
    assert len({(a, b) for a, b in zip(d1.tolist(), d2.tolist())}) == d1.size and np.abs(d1).max() == 256 and np.abs(d2).max() == 128
    rank = np.abs(d1) // 16 + np.abs(d2) // 16
    assert (np.diff(rank) >= 0).all()
    assert list(zip(d1[:9].tolist(), d2[:9].tolist())) == [(0, 0), (16, 0), (-16, 0), (0, 16), (0, -16), (32, 0), (-32, 0), (16, 16), (16, -16)]
    e1, e2 = candfold_trials(0, 0)
    assert e1.tolist() == [0] and e2.tolist() == [0]
    f1, _ = candfold_trials(2, 0, step=5)
    assert f1.tolist() == [0, 5, -5, 10, -10]
    assert candfold_trials(31, 32)[0].size == 4095
    for bad in ((32, 32), (-1, 0), (1, 1, 0), (1, 0, 1 << 21)):
        with pytest.raises(ValueError):
            candfold_trials(*bad)
    g = candfold_gains(64, 6)
    assert g.dtype == np.float32 and g[0] == np.float32(1 / np.sqrt(1 - 1 / 64)) and g[5] == np.float32(1 / np.sqrt(32 * 0.5))
    with pytest.raises(ValueError):
        candfold_gains(64, 7)


# ---------------------------------------------------------------- the oscillators
def test_oscillators_against_fold_phase_with_an_accelerated_candidate():
    """A plain candidate folds at its frequency from the window t0; `period` stands for 1 / freq.  An accelerated candidate has
    f1 = -accel * freq / c about the middle of the segment it was found in: the oscillator's frequency at mid-segment is freq, and at
    t0 it is freq + f1 (t0 - T / 2).  The integers are fold_phase's."""
    tsamp, nt = 1e-3, 1 << 15
    cands = [dict(pair=1, idm=3, freq=7.25), dict(pair=0, idm=2, period=0.125, snr=9.0), dict(pair=2, idm=0, freq=30.0, accel=25.0, ia=3)]
    t0 = nt * tsamp
    o = candfold_oscillators(cands, t0, tsamp, nt)
    assert [(k['pair'], k['idm'], k['f0']) for k in o] == [(1, 3, 7.25), (0, 2, 8.0), (2, 0, 30.0)]
    assert o[0]['f1'] == o[1]['f1'] == 0.0 and o[2]['f1'] == -25.0 * 30.0 / C_LIGHT and o[2]['pepoch'] == nt * tsamp / 2
    for k in o:
        assert (k['phi0'], k['dphi'], k['ddphi']) == fold_phase(k['f0'], k['f1'], Fraction(nt) * Fraction(tsamp) / 2, t0, tsamp)
    assert o[0]['ddphi'] == 0 and o[2]['ddphi'] < 0
    # turns per window at the first window, from the integers: freq + f1 (t0 + tsamp / 2 - T / 2), to the rounding of 2^-64
    f_at = o[2]['dphi'] / 2.0 ** 64 / tsamp
    assert abs(f_at - (30.0 + o[2]['f1'] * (t0 + tsamp / 2 - nt * tsamp / 2))) < 1e-12
    for bad in ([dict(pair=0, freq=1.0)], [dict(pair=0, idm=0)], [dict(pair=0, idm=0, freq=-1.0)]):
        with pytest.raises(ValueError):
            candfold_oscillators(bad, 0.0, tsamp, nt)
    with pytest.raises(ValueError):
        candfold_oscillators(cands, 0.0, 0.0, nt)


# ---------------------------------------------------------------- a planted train
PLANTED = dict(nsub=16, nsubwin=2048, nbin=64, nwidth=5, period=100.37, drift=12, bow=6)
RATIO = 2.366       # S / S0 of the restatement on tests/golden/candfold_planted.npy


def test_planted_drift_and_bow_are_recovered_exactly_and_refined_to_a_grid_step():
    """tests/golden/candfold_planted.npy: 2^15 windows of noise of mean 55 and sigma 1 with a Gaussian pulse of height 1.0 and a duty
    cycle of 2 % (FWHM) whose phase runs ahead of a fold at 100.37 windows by (12 tau + 6 (2 tau)^2) / 64 turns, tau = (n + 1/2) / NT
    - 1/2: a drift of 12 bins over the segment and a bow of 6 bins at its ends.  Folded at 100.37 windows in 16 x 2048 windows and 64
    bins and refined over a 33 x 21 grid of whole bins, the restatement names the planted trial (+192, +96) exactly -- the sign of
    the contract: a positive d1 is a source faster than the fold -- and candfold_refined returns the planted f0 and f1 to within one
    grid step.  Measured: S / S0 = 2.366 (S = 0.8125, S0 = 0.3434); the assertion stands at half the excess over 1, 1.683."""
    c = PLANTED
    nt = c['nsub'] * c['nsubwin']
    z = np.load(os.path.join(ROOT, "tests", "golden", "candfold_planted.npy"))
    assert z.shape == (nt,) and z.dtype == np.float32
    d1, d2 = candfold_trials(16, 10)
    assert d1.size == 33 * 21
    tsamp = 1e-3
    cand = dict(pair=0, idm=0, period=c['period'] * tsamp)
    (o,) = candfold_oscillators([cand], 0.0, tsamp, nt)
    ref = candfold_ref.CandfoldRef(1, 1, 1, 1, c['nbin'], c['nsub'], c['nsubwin'], c['nwidth'], d1, d2, candfold_gains(c['nbin'], c['nwidth']))
    ref.set_candidates([0], [o['phi0']], [o['dphi']], [o['ddphi']], [1])
    rec, prof = ref.run(z.reshape(nt, 1, 1, 1))
    r = rec[0]
    print("planted train: S = %.4f, S0 = %.4f, S / S0 = %.4f, trial (%d, %d), width %d" % (r['S'], r['S0'], r['S'] / r['S0'], d1[r['it']], d2[r['it']], 1 << r['iw']))
    assert (d1[r['it']], d2[r['it']]) == (16 * c['drift'], 16 * c['bow'])
    assert r['S'] / r['S0'] >= 1 + (RATIO - 1) / 2
    T = nt * tsamp
    f0, f1 = candfold_refined(o, r, d1, d2, c['nbin'], nt, tsamp)
    want0, want1 = 1 / (c['period'] * tsamp) + c['drift'] / (c['nbin'] * T), 8.0 * c['bow'] / (c['nbin'] * T * T)
    assert abs(f0 - want0) <= 16 / (16.0 * c['nbin'] * T) and abs(f1 - want1) <= 16 / (2.0 * c['nbin'] * T * T)
    assert f0 > 1 / (c['period'] * tsamp) and f1 > 0
    # in sigma: the robust sigma of the cube is the noise's, and the refined fold stands far above a threshold the plain one misses
    sigma = candfold_sigma(ref.cube, ref.hits)
    assert abs(sigma[0] - 1.0) < 0.05
    (k,) = candfold_candidates(rec, prof, [o], sigma, d1, d2, c['nbin'], nt, tsamp, 12.0)
    assert k['snr'] > 12 > k['snr0'] and (k['d1'], k['d2'], k['cand']) == (192, 96, 0) and np.array_equal(k['profile'], prof[0])
    assert abs(k['snr'] - r['S'] * np.sqrt(nt / c['nbin']) / sigma[0]) < 1e-9 and candfold_candidates(rec, prof, [o], sigma, d1, d2, c['nbin'], nt, tsamp, 100.0) == []
    # the best profile is the winning trial's, and the pulse is where the record says
    assert int(np.argmax(prof[0])) in ((r['j'] + i) % c['nbin'] for i in range(1 << r['iw']))


# ---------------------------------------------------------------- the tie rule, NaN cells, empty slots
def _cube(nsub, nbin, cells, h=4):
    cube, hits = np.zeros((nsub, nbin), np.float32), np.full((nsub, nbin), h, np.uint32)
    for (s, b), v in cells.items():
        cube[s, b] = v
    return cube, hits


def test_tie_rule_on_an_integer_cube():
    """nsub 4 x nbin 16, 4 hits a cell, pulses of 8 a window at bins 3 and 9: p = 8 there, total 16.  Gains (6, 7): width 1 scores
    (8 - 1) 6 = 42 at bins 3 and 9, width 2 (8 - 2) 7 = 42 at bins 2, 3, 8 and 9.  Trials (64, 0), (1, 0), (0, 0), (-1, 0): the second
    and fourth shift nothing.  The first of the equal maxima in (t, iw, j) order: trial 1, width 0, bin 3; S0 is trial 2's 42."""
    cells = {(s, b): 32.0 for s in range(4) for b in (3, 9)}
    cube, hits = _cube(4, 16, cells)
    d1, d2 = [64, 1, 0, -1], [0, 0, 0, 0]
    rot = candfold_shifts(d1, d2, 4, 16)
    assert rot[1:].any() == 0 and rot[0].tolist() == [15, 0, 1, 2]
    rec, prof = candfold_ref.refine(cube, hits, rot, np.array([6, 7], np.float32), 2, 2)
    assert rec == (42.0, 42.0, 1, 0, 3, 0) and prof.tolist() == [8.0 if b in (3, 9) else 0.0 for b in range(16)]
    # without a zero trial S0 reads +0; with the table reversed the same maximum is named at the first trial again
    assert candfold_ref.refine(cube, hits, rot[:2], np.array([6, 7], np.float32), 2, -1)[0] == (42.0, 0.0, 1, 0, 3, 0)
    assert candfold_ref.refine(cube, hits, rot[::-1], np.array([6, 7], np.float32), 2, 1)[0] == (42.0, 42.0, 0, 0, 3, 0)
    # -0 and +0 are equal: an all-zero cube names (0, 0, 0) whatever the signs of its zeros
    cube0, _ = _cube(4, 16, {(1, 5): -0.0})
    assert candfold_ref.refine(cube0, hits, rot, np.array([6, 7], np.float32), 2, 2)[0] == (0.0, 0.0, 0, 0, 0, 0)


def test_nan_cells_empty_bins_and_inactive_slots():
    """A NaN cell is in total_c, so no score of its candidate is a number: the record is empty and S0 reads +0.  A NaN in a cell of
    another candidate changes nothing here.  Bins without hits read +0 in the profile.  Inactive and unset slots read
    {+0, +0, -1, -1, -1, 0} and a zero profile, and their cubes stay zero."""
    cells = {(s, b): 32.0 for s in range(4) for b in (3, 9)}
    cube, hits = _cube(4, 16, cells)
    rot = candfold_shifts([0, 16], [0, 0], 4, 16)
    g = candfold_gains(16, 2)
    bad = cube.copy()
    bad[2, 7] = np.nan
    rec, prof = candfold_ref.refine(bad, hits, rot, g, 2, 0)
    assert rec == candfold_ref.EMPTY and not prof.any()
    holes = hits.copy()
    holes[:, 5] = 0
    holes[:, 3] = 0
    rec, prof = candfold_ref.refine(cube, holes, rot, g, 2, 0)
    assert prof[5] == 0 and prof[3] == 0 and not np.signbit(prof[[3, 5]]).any() and rec[2:5] == (0, 0, 9)
    d1, d2 = candfold_trials(1, 0)
    ref = candfold_ref.CandfoldRef(1, 2, 1, 4, 16, 2, 8, 2, d1, d2, g)
    o = fold_phase(1 / 5.0, 0, 0, 0, 1)
    ref.set_candidates([0, 1, 0], [o[0]] * 3, [o[1]] * 3, [o[2]] * 3, [1, 1, 0])
    x = np.arange(32, dtype=np.float32).reshape(16, 1, 2, 1)
    x[5, 0, 1, 0] = np.nan
    rec, prof = ref.run(x)
    assert rec['it'][0] >= 0 and tuple(rec[1]) == tuple(rec[2]) == tuple(rec[3]) == candfold_ref.EMPTY and not prof[1:].any()
    assert np.isnan(ref.cube[1]).sum() == 1 and not ref.cube[2:].any() and not ref.hits[2:].any() and ref.hits[0].sum() == 16
    assert rec.dtype == CANDFOLD_RECORD and CANDFOLD_RECORD.itemsize == 16
    r2, p2 = as_records_candfold(np.frombuffer(ref.span((rec, prof)), np.uint8), 4, 16)
    assert r2.tobytes() == rec.tobytes() and p2.tobytes() == prof.tobytes()
    with pytest.raises(ValueError):
        as_records_candfold(np.zeros(10, np.uint8), 4, 16)


def test_restatement_does_not_depend_on_the_calls():
    """The restatement itself: one call, single windows, and a straddling call give the same bytes, and a set given mid-segment holds
    from the boundary with m = 0."""
    rng = np.random.default_rng(8)
    d1, d2 = candfold_trials(2, 1)
    g = candfold_gains(16, 3)
    x = (55 + rng.standard_normal((100, 1, 3, 1))).astype(np.float32)
    o, o2 = fold_phase(1 / 7.3, 1e-5, 0, 0, 1), fold_phase(1 / 4.1, 0, 0, 0, 1)
    outs = []
    for sizes in ([40, 40, 20], [1] * 100, [39, 40, 21], [40, 1, 40, 19]):
        ref = candfold_ref.CandfoldRef(1, 3, 1, 2, 16, 4, 10, 3, d1, d2, g)
        ref.set_candidates([2, 0], [o[0], o2[0]], [o[1], o2[1]], [o[2], o2[2]], [1, 1])
        n, got = 0, []
        for nc in sizes:
            out = ref.run(x[n:n + nc])
            n += nc
            if out is not None:
                got.append(ref.span(out) + ref.cube.tobytes() + ref.hits.tobytes())
        assert len(got) == 2
        outs.append(got)
    assert all(o_ == outs[0] for o_ in outs[1:]) and outs[0][0] != outs[0][1]
    ref = candfold_ref.CandfoldRef(1, 3, 1, 2, 16, 4, 10, 3, d1, d2, g)
    ref.set_candidates([2], [o[0]], [o[1]], [o[2]], [1])
    ref.run(x[:7])
    ref.set_candidates([0], [o2[0]], [o2[1]], [o2[2]], [1])
    first = ref.run(x[7:47])
    second = ref.run(x[47:80])
    fresh = candfold_ref.CandfoldRef(1, 3, 1, 2, 16, 4, 10, 3, d1, d2, g)
    fresh.set_candidates([0], [o2[0]], [o2[1]], [o2[2]], [1])
    assert first is not None and ref.span(second) == fresh.span(fresh.run(x[40:80]))


# ---------------------------------------------------------------- the engine table and the C entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.NEWEST_ENGINES == [("Candfold", "candfold", True)]
    older = ffi.ENGINES + ffi.MORE_ENGINES + ffi.NEWER_ENGINES
    assert not {r[0] for r in ffi.NEWEST_ENGINES} & {r[0] for r in older} and not {r[1] for r in ffi.NEWEST_ENGINES} & {r[1] for r in older}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.NEWEST_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.NEWEST_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported, declared and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are
    not; HipBackend has a method for each.  Initialize refuses every size outside the contract's table before it touches a device;
    Run and the getters refuse null and misaligned pointers before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    names = ["xengCandfold" + n for n in ("Initialize", "SetCandidates", "Run", "Reset", "GetInfo", "GetCube", "CheckGuards", "Mark", "Wait", "TicketDone", "Sync",
                                          "Destroy")]
    for name in names:
        assert hasattr(L, name) and name in ffi.SYMBOLS and name in test_engine_table_cpu.DECLARED, name
        assert (name in ffi.ENQUEUE_ONLY) == (name[12:] in ("Run", "Reset", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_candidates", "run", "reset", "info", "cube", "guards_intact", "mark", "wait", "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "candfold_" + m)), m
    pi, pf = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
    d = np.zeros(4097, np.int32)
    big = np.full(1, (1 << 20) + 1, np.int32)
    g = np.ones(8, np.float32)
    inf = np.array([1.0, np.inf], np.float32)

    def init(*sizes, d1=d, d2=d, gains=g, ntrial=1):
        return L.xengCandfoldInitialize(0, *sizes, ntrial, d1.ctypes.data_as(pi), d2.ctypes.data_as(pi), gains.ctypes.data_as(pf))

    # (npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth)
    good = [2, 4, 64, 1, 3, 16, 2, 40, 2]
    for i, v in ((0, 0), (1, 0), (2, 0), (2, 81), (3, 2), (3, 3), (4, 0), (4, 4097), (5, 8), (5, 24), (5, 512), (6, 1), (6, 65), (7, 0), (7, 1 << 30), (8, 0),
                 (8, 5)):
        args = list(good)
        args[i] = v
        assert init(*args) == INVALID_ARGUMENT, args
    assert init(2, 4, 64, 1, 3, 256, 33, 40, 2) == INVALID_ARGUMENT                 # nsub * nbin > 8192
    assert init(1 << 13, 1 << 12, 64, 1, 3, 16, 2, 40, 2) == INVALID_ARGUMENT       # more than 2^24 series
    assert init(*good, ntrial=0) == INVALID_ARGUMENT and init(*good, ntrial=4097) == INVALID_ARGUMENT
    assert init(*good, d1=big) == INVALID_ARGUMENT and init(*good, d2=-big) == INVALID_ARGUMENT and init(*good, gains=inf) == INVALID_ARGUMENT
    assert init(*good, gains=np.zeros(2, np.float32)) == INVALID_ARGUMENT and init(*good, gains=np.array([np.nan, 1], np.float32)) == INVALID_ARGUMENT
    assert L.xengCandfoldInitialize(0, *good, 1, None, d.ctypes.data_as(pi), g.ctypes.data_as(pf)) == INVALID_ARGUMENT
    assert init(1, 1, 64, 1, 4096, 256, 32, 64, 2) == INVALID_ARGUMENT              # 512 MiB of state: above XENG_CANDFOLD_MAX_STATE_BYTES
    assert b"state" in L.xengGetLastError()
    if not _gpu_present():
        assert init(*good) not in (0, INVALID_ARGUMENT)                             # (a good table gets as far as the device)
    comp = ctypes.c_int(-1)
    for args in ((None, 1, 16, ctypes.byref(comp)), (16, 1, 16, None), (20, 1, 16, ctypes.byref(comp)), (16, 1, 24, ctypes.byref(comp))):
        assert L.xengCandfoldRun(*args) == INVALID_ARGUMENT
    assert L.xengCandfoldGetInfo(None, None) == INVALID_ARGUMENT and L.xengCandfoldGetCube(None, None) == INVALID_ARGUMENT
    assert L.xengCandfoldSetCandidates(1, None, None, None, None, None) == INVALID_ARGUMENT
    if not _gpu_present():
        n = ctypes.c_longlong()
        assert L.xengCandfoldRun(16, 1, 16, ctypes.byref(comp)) == INVALID_STATE and L.xengCandfoldReset() == INVALID_STATE
        assert L.xengCandfoldGetInfo(ctypes.byref(n), ctypes.byref(n)) == INVALID_STATE and comp.value == -1


# ---------------------------------------------------------------- the block on CPU rings
class CandfoldBackend(OracleBackend):
    """The oracle backend plus xengCandfold* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.cf, self.calls, self.sets = None, [], []

    def candfold_initialize(self, gpu, npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains):
        self.cf = candfold_ref.CandfoldRef(npair, ndm, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains)
        self.dims = (nwin, npair, ndm, nprod)
        self.calls.append(('init', nprod, len(d1)))
        return 0

    def candfold_set_candidates(self, series, phi0, dphi, ddphi, active):
        self.cf.set_candidates(series, phi0, dphi, ddphi, active)
        self.sets.append((self.cf.nwindows, list(series)))
        self.calls.append('set')
        return 0

    def candfold_run(self, in_arr, nwin_call, out_arr):
        assert 1 <= nwin_call <= self.dims[0]
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape((nwin_call,) + self.dims[1:])
        out = self.cf.run(x)
        if out is None:
            assert out_arr is None
        else:
            out_arr.numpy().reshape(-1).view(np.uint8)[...] = np.frombuffer(self.cf.span(out), np.uint8)
        self.calls.append('run' if out is None else 'run+')
        return 0, int(out is not None)

    def candfold_cube(self, ncand_max, nsub, nbin):
        return self.cf.cube.copy(), self.cf.hits.copy()

    def candfold_reset(self):
        self.cf.reset()
        self.calls.append('reset')

    def candfold_mark(self):
        return self.beam_mark()

    def candfold_wait(self, ticket):
        self.beam_wait(ticket)

    def candfold_sync(self):
        pass


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


BLK = dict(npair=2, ndm=3, nwin=32, ncand_max=4, nbin=16, nsub=4, nsubwin=32, nwidth=2, ndrift=2, ncurve=1)
NT, NWIN = BLK['nsub'] * BLK['nsubwin'], BLK['nwin']


def _pulsed(rng, nwindows, nprod, period, series, amp=30.0):
    """integer noise 0..49 with a pulse of `amp` every `period` windows in one series (the last two of four words are cross terms)"""
    x = rng.integers(0, 50, (nwindows, BLK['npair'], BLK['ndm'], nprod)).astype(np.float32)
    n = np.arange(nwindows)
    x[(n % period) == 3, series // BLK['ndm'], series % BLK['ndm'], 0] += amp
    return x


def _expected(x, nprod, oscs_per_segment):
    """the spans of whole segments of x, each from a fresh restatement whose set starts at that segment's first window"""
    d1, d2 = candfold_trials(BLK['ndrift'], BLK['ncurve'])
    out = []
    for k, oscs in enumerate(oscs_per_segment):
        ref = candfold_ref.CandfoldRef(BLK['npair'], BLK['ndm'], nprod, BLK['ncand_max'], BLK['nbin'], BLK['nsub'], BLK['nsubwin'], BLK['nwidth'], d1, d2,
                                       candfold_gains(BLK['nbin'], BLK['nwidth']))
        ref.set_candidates([o['pair'] * BLK['ndm'] + o['idm'] for o in oscs], [o['phi0'] for o in oscs], [o['dphi'] for o in oscs], [o['ddphi'] for o in oscs],
                           [1] * len(oscs))
        out.append(ref.span(ref.run(x[k * NT:(k + 1) * NT])))
    return out


def test_block_counts_windows_skips_the_start_up_and_writes_the_header():
    """dedisp_latency = 40 windows and spans of 32: spans 0 and 1 begin inside the partial sums and are skipped; a segment of 4 spans
    completes at span 5, a second one at span 9 with m running on, and 2 spans more complete nothing.  Two spans of 4 records and 4
    profiles, the restatement's; only the completing calls carry an output; the header names the sizes, the trial table, where the
    profiles start and the candidates with their fold frequencies; on_folded gets the planted candidate, in sigma."""
    nprod, seq0, acc_len, S = 4, 4096, 32, 40
    nspan = 2 + 2 * NT // NWIN + 2
    rng = np.random.default_rng(5)
    x = _pulsed(rng, nspan * NWIN, nprod, 16, 4, amp=150.0)
    hdr = dedisp_header(BLK['npair'], BLK['ndm'], nprod, seq0=seq0, S=S, acc_len=acc_len)
    tsamp = hdr['tsamp']
    cands = [dict(pair=1, idm=1, period=16 * tsamp, sigma=9.0), dict(pair=0, idm=2, freq=1 / (23.5 * tsamp))]
    be, got = CandfoldBackend(), []
    cf = BeamCandFold(LOG, Ring("dd-output"), Ring("cf-output"), candidates=cands, threshold=6.0, on_folded=got.append, backend=be, **BLK)
    ospan = BLK['ncand_max'] * (16 + 4 * BLK['nbin'])
    sink = Sink(cf.oring, ospan)
    run_blocks([cf], Source(cf.iring, [(hdr, x, NWIN * BLK['npair'] * BLK['ndm'] * nprod * 4)]), [sink])
    (hd, tag, spans), = sink.sequences
    first = seq0 + 2 * NWIN * acc_len
    assert tag == first == hd['seq0'] and len(spans) == 2
    d1, d2 = candfold_trials(2, 1)
    assert (hd['ncand'], hd['ncand_max'], hd['nbin'], hd['nsub'], hd['nsubwin'], hd['nwidth'], hd['profile_offset'], hd['threshold']) == (2, 4, 16, 4, 32, 2, 64, 6.0)
    assert hd['d1'] == d1.tolist() and hd['d2'] == d2.tolist() and hd['dedisp_latency'] == S and hd['nprod'] == nprod
    assert [(c['pair'], c['idm'], c['f1']) for c in hd['candidates']] == [(1, 1, 0.0), (0, 2, 0.0)] and hd['candidates'][0]['f0'] == 1 / (16 * tsamp)
    # the block's oscillators: without seq_mid the frequency holds at the set's first window (t0 = pepoch = half a segment)
    oscs = candfold_oscillators(cands, NT * tsamp / 2, tsamp, NT)
    ref = candfold_ref.CandfoldRef(BLK['npair'], BLK['ndm'], nprod, 4, 16, 4, 32, 2, d1, d2, candfold_gains(16, 2))
    ref.set_candidates([4, 2], [o['phi0'] for o in oscs], [o['dphi'] for o in oscs], [o['ddphi'] for o in oscs], [1, 1])
    exp = [ref.span(ref.run(x[(2 + 4 * k) * NWIN:(6 + 4 * k) * NWIN])) for k in range(2)]
    assert [s.tobytes() for s in spans] == exp and exp[0] != exp[1]
    run4 = ['run'] * (NT // NWIN - 1) + ['run+']
    assert be.calls == [('init', nprod, 15), 'set'] + run4 + run4 + ['run'] * 2 and be.sets == [(0, [4, 2])]
    assert cf.stats['nstartup'] == 2 and cf.stats['nwindow'] == (nspan - 2) * NWIN and cf.stats['nsegment_done'] == 2 and cf.stats['ndropped'] == 0
    assert len(got) == 2 and all([k['cand'] for k in g] == [0] for g in got) and cf.stats['nfolded'] == 2 and cf.stats['ncand'] == 2
    k = got[1][0]
    assert k['snr'] > 6 and (k['pair'], k['idm'], k['width']) == (1, 1, 1) and abs(k['period'] - 16 * tsamp) < 0.02 * 16 * tsamp and k['profile'].shape == (16,)
    assert cf.stats['folded'][0]['cand'] == 0 and 'profile' not in cf.stats['folded'][0]


def test_block_gap_drops_the_partial_segment_and_candidates_hold_from_the_next_segment():
    """Spans 0..5 and 7..18 of a sequence (6 never read), segments of 4 spans: segment 0 completes at span 3, spans 4 and 5 are a
    partial segment that the gap drops; the context is reset, the set starts again at span 7 and the output restarts in a sequence
    of its own there.  A `candidates` command before span 8 -- inside the segment of spans 7..10 -- leaves that segment alone and
    holds from span 11, where the output goes on in a third sequence whose header carries the new list; set_candidates() before
    span 15, on a boundary, holds at once.  A command with a pair outside the table is refused."""
    nprod, seq0, acc_len = 1, 700, 32
    rng = np.random.default_rng(11)
    x = _pulsed(rng, 19 * NWIN, nprod, 16, 4)
    hdr = dedisp_header(BLK['npair'], BLK['ndm'], nprod, seq0=seq0, S=0, acc_len=acc_len)
    tsamp = hdr['tsamp']
    a = [dict(pair=1, idm=1, period=16 * tsamp)]
    b = [dict(pair=0, idm=0, freq=1 / (9.0 * tsamp)), dict(pair=1, idm=1, period=16 * tsamp)]
    c3 = [dict(pair=1, idm=2, freq=1 / (5.0 * tsamp), accel=3.0e6, seq_mid=seq0)]
    be, r1, box, got = CandfoldBackend(), Ring("cf-output"), {}, []

    def spans():
        for k in list(range(6)) + list(range(7, 19)):
            if k == 8:
                box['cf'].process_command_strings(_cmd(candidates=b))
                assert box['cf'].last_response['val']['status'] == 'normal'
                box['cf'].process_command_strings(_cmd("2", candidates=[dict(pair=2, idm=0, freq=1.0)]))
                assert box['cf'].last_response['val']['status'] == 'error'
            if k == 15:
                box['cf'].set_candidates(c3)
            yield k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])

    cf = box['cf'] = BeamCandFold(LOG, _FakeRing([_FakeSeq(hdr, spans(), NWIN * BLK['npair'] * BLK['ndm'] * 4)]), r1, candidates=a, threshold=1000,
                                  on_folded=got.append, backend=be, **BLK)
    sink = Sink(r1, BLK['ncand_max'] * (16 + 4 * BLK['nbin']))
    sink.start()
    cf.main()
    sink.join(20)
    run4 = ['run'] * 3 + ['run+']
    assert be.calls == [('init', 1, 15), 'set'] + run4 + ['run'] * 2 + ['reset', 'set'] + run4 + ['set'] + run4 + ['set'] + run4
    assert be.sets == [(0, [4]), (0, [4]), (NT, [0, 4]), (2 * NT, [5])]
    (h0, t0, s0), (h1, t1, s1), (h2, t2, s2), (h3, t3, s3) = sink.sequences
    step = NWIN * acc_len
    assert (t0, t1, t2, t3) == (seq0, seq0 + 7 * step, seq0 + 11 * step, seq0 + 15 * step) and [h['seq0'] for h in (h0, h1, h2, h3)] == [t0, t1, t2, t3]
    assert [len(s) for s in (s0, s1, s2, s3)] == [1, 1, 1, 1] and [h['ncand'] for h in (h0, h1, h2, h3)] == [1, 1, 2, 1]
    assert [(k['pair'], k['idm']) for k in h2['candidates']] == [(0, 0), (1, 1)] and h3['candidates'][0]['f1'] == -3.0e6 * h3['candidates'][0]['f0'] / C_LIGHT
    half = NT * tsamp / 2
    oa, ob = candfold_oscillators(a, half, tsamp, NT), candfold_oscillators(b, half, tsamp, NT)
    oc = candfold_oscillators(c3, half + 15 * NWIN * tsamp, tsamp, NT)         # (seq_mid = seq0: 15 spans before the set's first window)
    assert oc[0]['ddphi'] != 0
    for got_span, first, oscs in ((s0, 0, oa), (s1, 7, oa), (s2, 11, ob), (s3, 15, oc)):
        assert got_span[0].tobytes() == _expected(x[first * NWIN:], nprod, [oscs])[0]
    assert cf.stats['ndropped'] == 1 and cf.stats['nsegment_done'] == 4 and cf.stats['ncand'] == 1 and got == []
    with pytest.raises(ValueError):
        cf.set_candidates([])


@pytest.mark.parametrize("kw", [dict(npair=0), dict(nwin=NT + 1), dict(nwin=48), dict(ncand_max=0), dict(ncand_max=4097), dict(nbin=8), dict(nbin=48),
                                dict(nbin=512), dict(nsub=1), dict(nsub=65), dict(nbin=256, nsub=64, nsubwin=2), dict(nsubwin=0), dict(nwidth=0),
                                dict(nwidth=5), dict(ndrift=40, ncurve=40), dict(ndrift=-1), dict(step=0), dict(threshold=float('nan')), dict(on_folded=3),
                                dict(candidates=[]), dict(candidates=[dict(pair=0, idm=0)]), dict(candidates=[dict(pair=0, idm=3, freq=1.0)]),
                                dict(candidates=[dict(pair=0, idm=0, freq=0.0)]), dict(candidates=[dict(pair=0, idm=0, freq=1.0)] * 5),
                                dict(candidates=[dict(pair=0, idm=0, freq=1.0, accel=float('inf'))]), dict(candidates="x")])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(BLK)
    args.update(kw)
    be = CandfoldBackend()
    with pytest.raises(ValueError, match="BEAM_CAND_FOLD"):
        BeamCandFold(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.cf is None


def test_block_without_candidates_fails_loudly():
    """No candidates at construction and none given: the first span past the start-up raises instead of folding nothing."""
    hdr = dedisp_header(BLK['npair'], BLK['ndm'], 1, seq0=0, S=0, acc_len=32)
    x = np.zeros((NWIN, BLK['npair'], BLK['ndm'], 1), np.float32)
    cf = BeamCandFold(LOG, _FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("cf-output"), backend=CandfoldBackend(), **BLK)
    with pytest.raises(RuntimeError, match="no candidates"):
        cf.main()
