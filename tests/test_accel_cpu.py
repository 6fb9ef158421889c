"""BeamAccelSearch without a GPU: the index rule (its ends, monotone and in range at the limit |alpha| * NT = 0.5 for both signs,
half-even rounding at exact ties), accel_alpha / accel_of / accel_trials and their refusals, accel_candidates on hand-built planes,
the best-over-trials rule of the restatement (tests/accel_ref.py), a planted accelerated pulse train on the restatement, the block
on CPU rings with a backend that keeps the context's state and serves xengAccel* by the float32 restatement -- window counting,
the start-up skip, a gap, the commands, the header, the constructor's refusals; the NEWER_ENGINES row under the per-row checks of
tests/test_engine_table_cpu.py; and the C entry points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import (ACCEL_RECORD, BeamAccelSearch, BeamPeriodSearch, accel_alpha, accel_candidates, accel_index, accel_of, accel_trials,
                                            as_records_accel, period_bands, period_candidates_long, period_sift)
from caltech_bifrost_dsp_amd.blocks.accel_search import C_LIGHT
from caltech_bifrost_dsp_amd.ring import Ring
from tests import accel_ref, plong_ref, test_engine_table_cpu
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_pulse_cpu import dedisp_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
NT, NWIN = 1 << 15, 1 << 12                     # the smallest segment; 8 spans fill it


# ---------------------------------------------------------------- the index rule
@pytest.mark.parametrize("nt", [1 << 15, 1 << 16, 1 << 20])
def test_index_map_ends_monotone_and_in_range_at_the_limit(nt):
    """s(0) = s(NT - 1) = 0 for every admissible alpha; at |alpha| * NT = 0.5 exactly, both signs, the map is non-decreasing,
    stays inside [0, NT - 1] and steps by 0, 1 or 2 windows; the mid-segment shift is -alpha NT^2 / 4; beyond the limit: refused.
    The block's function and the restatement's are the same integers."""
    for alpha in (0.5 / nt, -0.5 / nt, 0.0, 0.123 / nt, -1e-13, 2.0 ** -21 * (1 << 15) / nt):
        idx = accel_index(alpha, nt)
        assert idx.dtype == np.int64 and idx.tobytes() == accel_ref.accel_index(alpha, nt).tobytes()
        assert idx[0] == 0 and idx[-1] == nt - 1
        assert idx.min() >= 0 and idx.max() <= nt - 1
        d = np.diff(idx)
        assert d.min() >= 0 and d.max() <= 2
        assert abs((idx[nt // 2] - nt // 2) + alpha * nt * nt / 4) <= 0.5
    assert (accel_index(0.0, nt) == np.arange(nt)).all()
    assert accel_index(0.5 / nt, nt)[nt // 2] == nt // 2 - nt // 8 and accel_index(-0.5 / nt, nt)[nt // 2] == nt // 2 + nt // 8
    for bad in (np.nextafter(0.5 / nt, 1.0), -0.51 / nt, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            accel_index(bad, nt)


def test_index_map_rounds_exact_halves_to_even():
    """alpha = +-2^-21 at NT = 2^15: alpha * n (n - NT) is an exact half at n = 1024 * odd (n (n - NT) = 2^20 * odd * odd), and the
    shift there must be the EVEN neighbour.  Every one of these halves has an odd integer part (odd * (odd - 32) is 1 mod 4), so
    half-even rounds them away from zero: that tells half-even from floor(x + 0.5) at alpha > 0, where the products are negative,
    but not from rounding half away from zero.  alpha = +-3 * 2^-21 gives halves with an even integer part, which half-even rounds
    TOWARDS zero: together the two tell it from every other rule."""
    nt = 1 << 15
    n = 1024 * np.arange(1, 32, 2)
    q = n * (n - nt)
    assert (q % (1 << 21) == 1 << 20).all()     # (exact halves of 2^21)
    for m in (1.0, -1.0, 3.0, -3.0):
        alpha = m * 2.0 ** -21
        s = accel_index(alpha, nt)[n] - n
        x = alpha * q.astype(np.float64)
        assert (np.abs(x - np.trunc(x)) == 0.5).all()
        assert (s % 2 == 0).all() and (np.abs(s - x) == 0.5).all()
        away = np.where(x > 0, np.ceil(x), np.floor(x))
        assert (s == away).all() if abs(m) == 1 else (s == np.trunc(x)).all()
        if m == 1.0:
            assert (x < 0).all() and (s != np.floor(x + 0.5)).all()     # (round-half-up would differ)


# ---------------------------------------------------------------- the trial table
def test_accel_alpha_round_trips_and_sign_convention():
    """alpha = acc * tsamp / 2c; alpha > 0 undoes a source accelerating away: its pulses arrive late by acc t^2 / 2c, window n's
    emission at n + alpha n^2 = (n + alpha n (n - NT)) + alpha NT n, the map plus a constant stretch of the period."""
    tsamp = 2.5e-4
    for acc in (0.0, 3.7, -250.0):
        a = accel_alpha(acc, tsamp)
        assert isinstance(a, float) and a == acc * tsamp / (2 * C_LIGHT) and abs(accel_of(a, tsamp) - acc) <= 1e-12 * abs(acc)
        assert (a > 0) == (acc > 0)
    arr = accel_alpha(np.array([1.0, -2.0]), tsamp)
    assert arr.shape == (2,) and np.allclose(accel_of(arr, tsamp), [1.0, -2.0], rtol=1e-14, atol=0)
    # a source accelerating away at acc: a pulse emitted at window tau arrives at tau + alpha tau^2
    nt, acc = NT, 40.0
    alpha = accel_alpha(acc, tsamp)
    tau = np.arange(0, nt, 997.0)
    late = alpha * tau ** 2
    assert (late >= 0).all() and np.allclose(late, acc * (tau * tsamp) ** 2 / (2 * C_LIGHT) / tsamp)
    assert np.allclose(tau + late, tau + alpha * tau * (tau - nt) + alpha * nt * tau)


def test_accel_trials_table_and_refusals():
    nt, tsamp, fmax = 1 << 20, 1e-3, 500.0
    T = nt * tsamp
    da = C_LIGHT / (T * T * fmax)
    al = accel_trials(10.0, tsamp, nt, fmax)
    n = (al.size - 1) // 2
    assert al.dtype == np.float64 and al.size % 2 == 1 and al[n] == 0.0 and (al[::-1] == -al).all() and (np.diff(al) > 0).all()
    assert n == int(np.ceil(10.0 / da)) and np.allclose(accel_of(al, tsamp), da * np.arange(-n, n + 1), rtol=1e-12, atol=0)
    assert accel_of(al, tsamp)[-1] >= 10.0 > accel_of(al, tsamp)[-2]
    # neighbouring trials differ by zstep bins of drift at fmax: z = 2 alpha nt k with k = fmax * T
    assert np.allclose(2 * np.diff(al) * nt * (fmax * T), 1.0, rtol=1e-9)
    assert np.allclose(2 * np.diff(accel_trials(10.0, tsamp, nt, fmax, zstep=2.0)) * nt * (fmax * T), 2.0, rtol=1e-9)
    assert accel_trials(0.0, tsamp, nt, fmax).tolist() == [0.0]
    assert accel_trials(127 * da, tsamp, nt, fmax).size == 255
    with pytest.raises(ValueError, match="more than 256"):
        accel_trials(128 * da, tsamp, nt, fmax)
    with pytest.raises(ValueError, match="limit of the index map"):
        accel_trials(1.01 * C_LIGHT / (NT * 1e-3), 1e-3, NT, 0.02)      # (beyond c / T with few trials)
    for bad in (dict(amax=-1.0), dict(amax=float('nan')), dict(tsamp=0.0), dict(fmax=0.0), dict(zstep=0.0)):
        args = dict(amax=10.0, tsamp=tsamp, nt=nt, fmax=fmax, zstep=1.0)
        args.update(bad)
        with pytest.raises(ValueError):
            accel_trials(**args)


# ---------------------------------------------------------------- the best-over-trials rule and the candidates
def test_best_over_trials_rule_of_the_restatement():
    """Hand-built trial records: the larger H wins, among equals the smaller trial; an empty record and a NaN never enter; H0 is
    the first zero trial's H, +0 where that record is empty or there is no zero trial."""
    trec = np.zeros((4, 5), plong_ref.RECORD)
    trec['k'] = -1
    #            rec 0       rec 1       rec 2      rec 3 (empty everywhere)  rec 4
    trec[0] = [(3.0, 10), (0.0, -1), (5.0, 7), (0.0, -1), (np.nan, 4)]
    trec[1] = [(4.0, 11), (2.0, 20), (5.0, 6), (0.0, -1), (1.0, 9)]
    trec[2] = [(4.0, 12), (0.0, -1), (5.0, 5), (0.0, -1), (0.5, 8)]
    trec[3] = [(1.0, 13), (2.0, 21), (9.0, 4), (0.0, -1), (np.nan, 3)]
    out = accel_ref.best_over_trials(trec, [1e-7, 0.0, 0.0, -1e-7])
    assert out.tolist() == [(4.0, 11, 1, 4.0), (2.0, 20, 1, 2.0), (9.0, 4, 3, 5.0), (0.0, -1, -1, 0.0), (1.0, 9, 1, 1.0)]
    out = accel_ref.best_over_trials(trec, [1e-7, 2e-7, 0.0, -1e-7])
    assert out.tolist() == [(4.0, 11, 1, 4.0), (2.0, 20, 1, 0.0), (9.0, 4, 3, 5.0), (0.0, -1, -1, 0.0), (1.0, 9, 1, 0.5)]
    out = accel_ref.best_over_trials(trec, [1e-7, 2e-7, 3e-7, -1e-7])
    assert (out['H0'] == 0).all() and not np.signbit(out['H0']).any() and out['ia'].tolist() == [1, 1, 3, -1, 1]


def test_candidates_of_an_accel_plane():
    """One strong record in (pair 1, trials 1 and 2 of 3 DMs) at level 2: accel_candidates is period_candidates_long (nstack = 1) with
    the trials factor multiplied by ntrial, and carries ia, accel, H0 and z = 2 alpha nt k; period_sift takes it unchanged; raw
    bytes are taken with the four sizes."""
    npair, ndm, nlevel, nt, tsamp = 2, 3, 3, NT, 1e-3
    kedge = [2, 600, NT // 2]
    alphas = accel_trials(60.0, tsamp, nt, 100.0)
    assert alphas.size >= 3
    plane = np.zeros((npair, ndm, nlevel, 2), ACCEL_RECORD)
    plane['k'], plane['ia'] = -1, -1
    plane[1, 1, 2, 0] = (60.0, 1200, alphas.size - 1, 11.0)
    plane[1, 2, 2, 0] = (50.0, 1201, alphas.size - 1, 10.0)
    plane[0, 0, 0, 1] = (3.0, 900, 0, 3.0)                      # (noise: below the threshold)
    dms = [0.0, 0.5, 1.0]
    cands = accel_candidates(plane, 6.0, dms, nt, tsamp, kedge, alphas)
    c, = cands
    assert (c['pair'], c['idm'], c['h'], c['band'], c['k'], c['ntrial'], c['H']) == (1, 1, 4, 0, 1200, 2, 60.0)
    assert c['ia'] == alphas.size - 1 and c['H0'] == 11.0 and abs(c['accel'] - accel_of(alphas[-1], tsamp)) < 1e-9 and c['accel'] >= 60.0
    assert abs(c['z'] - 2 * alphas[-1] * nt * 1200) < 1e-9 and abs(c['z'] - c['accel'] * (nt * tsamp) ** 2 * (1200 / (nt * tsamp)) / C_LIGHT) < 1e-6
    hk = np.zeros(plane.shape, plong_ref.RECORD)
    hk['H'], hk['k'] = plane['H'], plane['k']
    plain, = period_candidates_long(hk, 6.0, dms, nt, 1, tsamp, kedge)
    assert abs((c['log10_pfa'] - plain['log10_pfa']) - np.log10(alphas.size)) < 1e-9
    assert {k: c[k] for k in plain if k != 'log10_pfa' and k != 'sigma'} == {k: plain[k] for k in plain if k != 'log10_pfa' and k != 'sigma'}
    s, = period_sift(cands, nt)
    assert s['ia'] == c['ia'] and s['harmonics'] == []
    raw = as_records_accel(plane.tobytes(), npair, ndm, nlevel, 2)
    assert raw.tobytes() == plane.tobytes() and as_records_accel(plane) is plane
    for bad in (lambda: as_records_accel(plane.tobytes()), lambda: as_records_accel(plane.tobytes()[:-16], npair, ndm, nlevel, 2),
                lambda: accel_candidates(plane, 6.0, dms, nt, tsamp, kedge, alphas[:2]), lambda: accel_candidates(plane, 6.0, dms, nt, tsamp, kedge, [])):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------- a planted accelerated pulse train
@pytest.mark.parametrize("shift", [24, -12])
def test_planted_accelerated_pulse_train_on_the_restatement(shift):
    """NT = 2^15, chi^2 noise with mean / sigma = 55, pulses of 10 sigma one window wide emitted every 37.3 windows and received at
    rint(tau + a0 tau (tau - NT)), a0 a mid-segment shift of 24 (and -12) windows; 17 trials with mid-segment shifts -32 .. 32 in
    steps of 4.  A condition on the input, checked on the float32 restatement: it picks the planted trial at all five levels with
    H >= 2 H0.  (Observed: H / H0 from 3.0 to 8.9 over both cases and, at shift 24, k = 1757, 3514, 7028, 14056, 14056 -- the
    fundamental NT / 37.3 = 878.5 lies between two bins, so level 1 finds the second harmonic.  The 2 is a floor under that.)"""
    nt, nlevel = NT, 5
    z, alphas, planted = accel_ref.planted_case(shift)
    assert alphas.size == 17 and alphas[8] == 0.0 and abs(-alphas[planted] * nt * nt / 4 - shift) < 1e-9
    plane = accel_ref.best_over_trials(accel_ref.trial_records(z, nt, nlevel, 64, [2, nt // 2], alphas), alphas)
    got = plane[0, :, 0]
    print("planted shift=%d: ia %s k %s H/H0 %s" % (shift, got['ia'], got['k'], got['H'] / got['H0']))
    assert (got['ia'] == planted).all() and (got['H'] >= 2.0 * got['H0']).all() and (got['H0'] > 0).all()
    assert (np.abs(got['k'] / (nt / 37.3) - np.rint(got['k'] / (nt / 37.3))) < 0.02).all()     # a harmonic of the planted period
    cands = period_sift(accel_candidates(plane[None], 6.0, [0.0], nt, 1e-3, [2, nt // 2], alphas), nt)
    assert len(cands) == 1 and cands[0]['ia'] == planted and abs(cands[0]['z']) > 1 and cands[0]['harmonics']


# ---------------------------------------------------------------- the block on CPU rings
class AccelBackend(OracleBackend):
    """The oracle backend plus xengAccel* served by the float32 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.ac, self.calls = None, []

    def accel_initialize(self, gpu, npair, ndm, nwin, nprod, nt, nlevel, nwhite, kedge, alphas):
        self.ac = dict(npair=npair, ndm=ndm, nwin=nwin, nprod=nprod, nt=nt, nlevel=nlevel, nwhite=nwhite, kedge=list(kedge), alphas=np.array(alphas, np.float64))
        self.keep, self.seg = None, []
        self.calls.append(('init', nprod, len(alphas)))
        return 0

    def accel_set_mask(self, keep):
        self.keep = None if keep is None else np.array(keep, np.uint8)
        self.calls.append('mask')
        return 0

    def accel_run(self, in_arr, nwin_call, out_arr):
        u = self.ac
        assert 1 <= nwin_call <= u['nwin']
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, u['npair'] * u['ndm'], u['nprod'])
        completed = 0
        self.seg.append(plong_ref.series(x, np.float32))
        if sum(len(s) for s in self.seg) == u['nt']:
            trec = accel_ref.trial_records(np.concatenate(self.seg), u['nt'], u['nlevel'], u['nwhite'], u['kedge'], u['alphas'], self.keep)
            plane = accel_ref.best_over_trials(trec.reshape(len(u['alphas']), u['npair'], u['ndm'], u['nlevel'], -1), u['alphas'])
            out_arr.numpy().reshape(-1).view(np.uint8)[...] = plane.reshape(-1).view(np.uint8)
            self.seg, completed = [], 1
        if not completed:
            assert out_arr is None
        self.calls.append('run+' if completed else 'run')
        return 0, completed

    def accel_reset(self):
        self.seg = []
        self.calls.append('reset')

    def accel_mark(self):
        return self.beam_mark()

    def accel_wait(self, ticket):
        self.beam_wait(ticket)

    def accel_sync(self):
        pass


def _noise(rng, nwindows, npair, ndm, nprod):
    return rng.integers(0, 50, (nwindows, npair, ndm, nprod)).astype(np.float32)


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _expected_planes(x, nt, nlevel, nwhite, kedge, alphas, keep=None):
    z = plong_ref.series(x, np.float32).reshape(x.shape[0], -1)
    out = []
    for s in range(z.shape[0] // nt):
        trec = accel_ref.trial_records(z[s * nt:(s + 1) * nt], nt, nlevel, nwhite, kedge, alphas, keep)
        out.append(accel_ref.best_over_trials(trec.reshape(len(alphas), x.shape[1], x.shape[2], nlevel, -1), alphas))
    return out


def test_block_counts_windows_skips_the_start_up_and_writes_the_header():
    """dedisp_latency = 5000 windows and spans of 4096: spans 0 and 1 begin inside the partial sums and are skipped; a segment of 8
    spans completes at span 9, a second one at span 17, and 3 spans more complete nothing.  Two planes, the restatement's, of
    nlevel x nband records of 16 bytes per series; only the completing calls carry an output; the trials come from amax / fmax
    and the header's tsamp, and the header names them."""
    npair, ndm, nlevel, nwhite, nprod, seq0, acc_len, S = 1, 3, 3, 64, 4, 4096, 32, 5000
    nspan = 2 + 2 * NT // NWIN + 3
    rng = np.random.default_rng(5)
    x = _noise(rng, nspan * NWIN, npair, ndm, nprod)
    hdr = dedisp_header(npair, ndm, nprod, seq0=seq0, S=S, acc_len=acc_len)
    T = NT * hdr['tsamp']
    amax = 2.2 * C_LIGHT / (T * T * 50.0)                       # 2.2 steps at fmax = 50 Hz: 7 trials
    be, got = AccelBackend(), []
    pr = BeamAccelSearch(LOG, Ring("dd-output"), Ring("ac-output"), npair=npair, ndm=ndm, nwin=NWIN, nt=NT, amax=amax, fmax=50.0, nlevel=nlevel, nwhite=nwhite,
                         kmin=3, nband=5, threshold=0.5, on_candidates=got.append, backend=be)
    assert isinstance(pr, BeamPeriodSearch) and pr.kedge == period_bands(NT, 5, 3) and pr.nband == 5 and pr.nstack == 1
    sink = Sink(pr.oring, npair * ndm * nlevel * 5 * 16)
    run_blocks([pr], Source(pr.iring, [(hdr, x, NWIN * npair * ndm * nprod * 4)]), [sink])
    (hd, tag, planes), = sink.sequences
    first = seq0 + 2 * NWIN * acc_len
    assert tag == first == hd['seq0'] and len(planes) == 2
    alphas = accel_trials(amax, hdr['tsamp'], NT, 50.0)
    assert alphas.size == 7 and alphas[3] == 0.0
    exp = _expected_planes(x[2 * NWIN:], NT, nlevel, nwhite, pr.kedge, alphas)
    assert [p.tobytes() for p in planes] == [e.tobytes() for e in exp] and exp[0].shape == (npair, ndm, nlevel, 5) and exp[0].dtype.itemsize == 16
    assert (hd['nt'], hd['nlevel'], hd['nwhite'], hd['kmin'], hd['nband'], hd['kedge'], hd['threshold'], hd['ntrial']) == (
        NT, nlevel, nwhite, 3, 5, pr.kedge, 0.5, 7)
    assert hd['alpha'] == alphas.tolist() and np.allclose(hd['accel'], accel_of(alphas, hdr['tsamp'])) and hd['accel'][3] == 0.0
    assert hd['dedisp_latency'] == S and hd['nprod'] == nprod and hd['dms'] == hdr['dms']
    run8 = ['run'] * (NT // NWIN - 1) + ['run+']
    assert be.calls == [('init', nprod, 7)] + run8 + run8 + ['run'] * 3
    assert pr.stats['nstartup'] == 2 and pr.stats['nwindow'] == (nspan - 2) * NWIN and pr.stats['nstack_done'] == 2 and pr.stats['ndropped'] == 0
    assert pr.stats['ncand'] == sum(len(c) for c in got) and all('harmonics' in c and 'ia' in c and 'accel' in c and 'H0' in c and 'z' in c for cs in got for c in cs)


def test_block_gap_drops_the_partial_segment_and_commands_take_effect():
    """Spans 0..10 and 12..27 of a sequence (11 never read), segments of 8 spans: segment 0 completes at span 7, spans 8-10 are a
    partial segment that the gap drops; the output restarts in a sequence of its own at span 12's sample.  A tone at bin 3000.  A
    `threshold` command before span 12 makes the second sequence's first segment report it, in the zero trial; a `mask` command
    before span 20 zaps it in the last segment, whose plane is the restatement under that mask."""
    npair, ndm, nlevel, nwhite, seq0, acc_len = 1, 3, 1, 64, 700, 32
    kedge = [2, 500, 5000, NT // 2]
    alphas = [-0.05 / NT, 0.0, 0.05 / NT]
    rng = np.random.default_rng(11)
    x = _noise(rng, 28 * NWIN, npair, ndm, 1)
    x[:, 0, 1, 0] += np.round(20 * np.cos(2 * np.pi * 3000 * np.arange(28 * NWIN) / NT)).astype(np.float32)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, S=0, acc_len=acc_len)
    be, r1, box, got = AccelBackend(), Ring("ac-output"), {}, []

    def spans():
        for k in list(range(11)) + list(range(12, 28)):
            if k == 12:
                box['pr'].process_command_strings(_cmd(threshold=6.0))
                assert box['pr'].last_response['val']['status'] == 'normal'
            if k == 20:
                box['pr'].process_command_strings(_cmd("2", mask=[[2990, 3010]]))
                assert box['pr'].last_response['val']['status'] == 'normal'
                box['pr'].process_command_strings(_cmd("3", mask=[[5, 2]]))
                assert box['pr'].last_response['val']['status'] == 'error'
            yield k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])

    pr = box['pr'] = BeamAccelSearch(LOG, _FakeRing([_FakeSeq(hdr, spans(), NWIN * npair * ndm * 4)]), r1, npair=npair, ndm=ndm, nwin=NWIN, nt=NT,
                                     alphas=alphas, nlevel=nlevel, nwhite=nwhite, kedge=kedge, threshold=1000, on_candidates=got.append, backend=be)
    sink = Sink(r1, npair * ndm * nlevel * 3 * 16)
    sink.start()
    pr.main()
    sink.join(20)
    run8 = ['run'] * 7 + ['run+']
    assert be.calls == [('init', 1, 3)] + run8 + ['run'] * 3 + ['reset'] + run8 + ['mask'] + run8
    (h0, t0, a), (h1, t1, b) = sink.sequences
    step = NWIN * acc_len
    assert (h0['seq0'], t0, h1['seq0'], t1) == (seq0, seq0, seq0 + 12 * step, seq0 + 12 * step) and (len(a), len(b)) == (1, 2)
    keep = np.ones(NT // 2, np.uint8)
    keep[2990:3010] = 0
    assert a[0].tobytes() == _expected_planes(x[:NT], NT, nlevel, nwhite, kedge, alphas)[0].tobytes()
    free, zapped = _expected_planes(x[12 * NWIN:], NT, nlevel, nwhite, kedge, alphas), _expected_planes(x[12 * NWIN:], NT, nlevel, nwhite, kedge, alphas, keep)
    assert [o.tobytes() for o in b] == [free[0].tobytes(), zapped[1].tobytes()]
    assert tuple(free[0][0, 1, 0, 1])[1:3] == (3000, 1) and free[0][0, 1, 0, 1]['H0'] == free[0][0, 1, 0, 1]['H'] and zapped[1]['k'][0, 1, 0, 1] != 3000
    assert len(got) == 1 and [(c['pair'], c['idm'], c['band'], c['k'], c['h'], c['ia'], c['accel'], c['z']) for c in got[0]] == [(0, 1, 1, 3000, 1, 1, 0.0, 0.0)]
    assert pr.stats['ndropped'] == 1 and pr.stats['nstack_done'] == 3 and pr.stats['threshold'] == 6.0 and pr.stats['ncand'] == 1


@pytest.mark.parametrize("kw", [dict(npair=0), dict(nwin=NT + 1), dict(nt=1 << 14), dict(nt=1 << 21), dict(nt=40000), dict(nlevel=6),
                                dict(nwhite=4), dict(nwhite=1 << 14), dict(nwhite=24), dict(kmin=0), dict(kmin=NT // 32), dict(nband=0), dict(nband=33),
                                dict(kedge=[2]), dict(kedge=[2, 2]), dict(kedge=[5, 3, 9]), dict(kedge=[0, 9]), dict(kedge=[NT // 32, NT // 2]),
                                dict(kedge=[2, NT // 2 + 1]), dict(kedge=list(range(2, 36))), dict(threshold=float('nan')), dict(on_candidates=3),
                                dict(alphas=None), dict(amax=1.0, fmax=10.0), dict(alphas=[]), dict(alphas=[0.0] * 257), dict(alphas=[float('nan')]),
                                dict(alphas=[0.6 / NT]), dict(alphas=None, amax=1.0), dict(alphas=None, amax=-1.0, fmax=10.0),
                                dict(alphas=None, amax=1.0, fmax=10.0, zstep=0)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(npair=1, ndm=5, nwin=NWIN, nt=NT, alphas=[0.0])
    args.update(kw)
    be = AccelBackend()
    with pytest.raises(ValueError, match="BEAM_ACCEL_SEARCH|period_bands"):
        BeamAccelSearch(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.ac is None


# ---------------------------------------------------------------- the engine table and the C entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.NEWER_ENGINES == [("Accel", "accel", True)] and ffi.MORE_ENGINES == [("Plong", "plong", True)] and len(ffi.ENGINES) == 19
    older = ffi.ENGINES + ffi.MORE_ENGINES
    assert not {r[0] for r in ffi.NEWER_ENGINES} & {r[0] for r in older} and not {r[1] for r in ffi.NEWER_ENGINES} & {r[1] for r in older}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.NEWER_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.NEWER_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def _edges(*e):
    return (ctypes.c_int * len(e))(*e)


def _alphas(*a):
    return (ctypes.c_double * len(a))(*a)


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported, declared and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are
    not; HipBackend has a method for each.  Initialize refuses every size outside the contract's table before it touches a device;
    Run refuses null and misaligned pointers, the getters null results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    names = ["xengAccel" + n for n in ("Initialize", "SetMask", "Run", "Reset", "GetInfo", "GetTrialRecords", "SetBatch", "GetBatch", "CheckGuards", "Mark",
                                       "Wait", "TicketDone", "Sync", "Destroy")]
    for name in names:
        assert hasattr(L, name) and name in ffi.SYMBOLS and name in test_engine_table_cpu.DECLARED, name
        assert (name in ffi.ENQUEUE_ONLY) == (name[9:] in ("Run", "Reset", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_mask", "run", "reset", "info", "trial_records", "set_batch", "get_batch", "guards_intact", "mark", "wait", "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "accel_" + m)), m
    nt = 1 << 15
    # (gpu, npair, ndm, nwin, nprod, nt, nlevel, nwhite, nband, kedge, ntrial, alpha)
    good = [0, 16, 256, 30, 1, nt, 5, 64, 2, _edges(2, 100, 1 << 14), 3, _alphas(-0.5 / nt, 0.0, 0.5 / nt)]
    bad = [(1, 0), (2, 0), (3, 0), (3, nt + 1), (4, 2), (5, 1 << 14), (5, 1 << 21), (5, 40000), (6, 0), (6, 6), (7, 4), (7, 48),
           (7, 1 << 14), (8, 0), (8, 33), (8, 3), (9, None), (9, _edges(0, 100, 1 << 14)), (9, _edges(1 << 10, 2000, 1 << 14)),
           (9, _edges(2, 2, 1 << 14)), (9, _edges(2, 100, 50)), (9, _edges(2, 100, (1 << 14) + 1)), (10, 0), (10, -1), (10, 257), (11, None),
           (11, _alphas(0.0, float('nan'), 0.0)), (11, _alphas(float('-inf'), 0.0, 0.0)), (11, _alphas(0.0, 0.0, np.nextafter(0.5 / nt, 1.0))),
           (11, _alphas(-0.500001 / nt, 0.0, 0.0))]
    for i, v in bad:
        args = list(good)
        args[i] = v
        if (i, v) == (8, 3):
            args[9] = _edges(2, 100, 1 << 14, 1 << 14)          # (the last edge repeated)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengAccelInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, (i, v)
    for npair, ndm, n in ((1 << 13, 1 << 12, 1 << 15), (16384, 4, 1 << 20)):
        with pytest.raises(ffi.XengError) as ei:                # 2^25 series; 2^16 series of 2^20 windows are 2^38 bytes of time buffer
            ffi.call("xengAccelInitialize", 0, npair, ndm, 30, 1, n, 1, 8, 1, _edges(1, n // 2), 1, _alphas(0.0))
        assert ei.value.status == INVALID_ARGUMENT
    buf = np.zeros(64, np.uint8)
    n, s = ctypes.c_longlong(), ctypes.c_int()
    for name, args in (("xengAccelRun", (None, 1, 4096, ctypes.byref(s))), ("xengAccelRun", (4096, 1, 4096, None)),
                       ("xengAccelRun", (4100, 1, 4096, ctypes.byref(s))), ("xengAccelRun", (4096, 1, 4104, ctypes.byref(s))),
                       ("xengAccelGetInfo", (None, ctypes.byref(n))), ("xengAccelGetInfo", (ctypes.byref(n), None)),
                       ("xengAccelGetTrialRecords", (0, 1, None)), ("xengAccelGetBatch", (None, ctypes.byref(s))), ("xengAccelGetBatch", (ctypes.byref(s), None)),
                       ("xengAccelMark", (None,)), ("xengAccelTicketDone", (1, None)), ("xengAccelCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_accel_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengAccelRun", (4096, 1, 4096, ctypes.byref(s))), ("xengAccelRun", (4096, 1, None, ctypes.byref(s))), ("xengAccelReset", ()),
                       ("xengAccelSetMask", (None,)), ("xengAccelGetInfo", (ctypes.byref(n), ctypes.byref(n))),
                       ("xengAccelGetTrialRecords", (0, 1, buf.ctypes.data)), ("xengAccelSetBatch", (1,)), ("xengAccelGetBatch", (ctypes.byref(s), ctypes.byref(s))),
                       ("xengAccelMark", (ctypes.byref(t),)), ("xengAccelWait", (1,)), ("xengAccelTicketDone", (1, ctypes.byref(s))), ("xengAccelSync", ()),
                       ("xengAccelCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengAccelDestroy")        # (nothing to destroy: success)
