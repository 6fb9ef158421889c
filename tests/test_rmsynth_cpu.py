"""BeamRmSynth without a GPU: the host helpers (rm_lambda2, rm_plan, rm_table, rmsf, rm_refine, rm_significance, rm_error,
pol_profile), the RMSYNTH_ENGINES row under the per-row checks of tests/test_engine_table_cpu.py, the C entry points' argument
checks, the restatement (tests/rmsynth_ref.py) against the float64 statement (rm_reference) on integer data, the block on CPU rings
with a backend that serves xengRmsynth* by the restatement -- the header keys, the refusals, an inactive pair, a `masks` and a
`weights` command -- and a planted Faraday-rotated pulse, checked in float64."""
import ctypes
import json
import threading

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import (RM_RECORD, BeamRmSynth, as_rmsynth, pol_profile, rm_error, rm_lambda2, rm_offsets, rm_plan, rm_reference, rm_refine,
                                            rm_significance, rm_table, rmsf)
from caltech_bifrost_dsp_amd.ring import Ring
from tests import rmsynth_cases, rmsynth_ref, test_engine_table_cpu
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2
_pf, _pb = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)


# ---------------------------------------------------------------- the host helpers
def test_plan_table_rmsf_refine_significance_and_profile():
    freqs = rmsynth_cases.FREQS
    bw = freqs[1] - freqs[0]
    lam2 = rm_lambda2(freqs)
    assert abs(lam2[0] - (299792458.0 / 60e6) ** 2) < 1e-12 and np.all(np.diff(lam2) < 0)
    with pytest.raises(ValueError):
        rm_lambda2([0.0, 1e6])
    p = rm_plan(freqs, bw, 3.0, 4)
    span = (299792458.0 / (60e6 - bw / 2)) ** 2 - (299792458.0 / (79.6e6 + bw / 2)) ** 2
    assert abs(p['span'] - span) < 1e-9 and abs(p['fwhm'] - 3.8 / span) < 1e-12 and abs(p['dphi'] - p['fwhm'] / 4) < 1e-15
    half = int(np.ceil(3.0 / p['dphi']))
    assert p['nphi'] == 2 * half + 1 and p['phis'][half] == 0 and p['phis'][-1] >= 3.0 > p['phis'][-2] and len(p['phis']) == p['nphi']
    widest = (299792458.0 / (60e6 - bw / 2)) ** 2 - (299792458.0 / (60e6 + bw / 2)) ** 2
    assert abs(p['phi_max_chan'] - np.sqrt(3.0) / widest) < 1e-9 and abs(p['max_scale'] - np.pi / (299792458.0 / (79.6e6 + bw / 2)) ** 2) < 1e-12
    for bad in ((freqs, 0.0, 3.0, 4), (freqs, bw, -1.0, 4), (freqs, bw, 3.0, 0.5), (freqs, bw, 1e4, 4), (freqs, 2 * 60e6, 3.0, 4)):
        with pytest.raises(ValueError):
            rm_plan(*bad)
    # the table against a direct float64 evaluation, each word rounded once
    w = rmsynth_cases.weights()
    w[3] = 0.5
    phis = rmsynth_cases.phis(130)
    T, wf, use, lam0 = rm_table(freqs, phis, w)
    assert T.shape == (70, 130, 2) and T.dtype == np.float32 and wf.dtype == np.float32 and use.dtype == np.uint8 and T.flags.c_contiguous
    assert use.tolist() == (w != 0).astype(int).tolist() and abs(lam0 - np.sum(w * lam2) / np.sum(w)) < 1e-12
    for g, k in ((0, 0), (3, 17), (69, 129), (11, 40), (30, 65)):
        th = 2.0 * phis[k] * (lam2[g] - lam0)
        assert T[g, k, 0] == np.float32(w[g] * np.cos(th)) and T[g, k, 1] == np.float32(w[g] * np.sin(th))
    assert np.array_equal(T[:, 65, 0], wf) and not T[:, 65, 1].any()          # (phi = 0: Tc = w, Ts = 0)
    with pytest.raises(ValueError):
        rm_table(freqs, phis, np.zeros(70))
    with pytest.raises(ValueError):
        rm_table(freqs, np.zeros(4097))
    r = rmsf(freqs, phis, w)
    assert abs(r[65] - 1.0) < 1e-15 and np.all(np.abs(r) <= 1 + 1e-12) and abs(r[0]) < 0.5
    # the half-power width of |R| is the plan's fwhm to a tenth (3.8 / span is the rule of thumb for a band flat in lambda^2)
    fine = np.linspace(-1, 1, 4001)
    a = np.abs(rmsf(freqs, fine))
    width = fine[a >= 0.5][-1] - fine[a >= 0.5][0]
    assert abs(width - p['fwhm']) < 0.15 * p['fwhm']
    # exact on a parabola: the vertex and its height
    x = phis[40:50]
    phi, peak = rm_refine(7.0 - 3.0 * (x - (x[4] + 0.013)) ** 2, x)
    assert abs(phi - (x[4] + 0.013)) < 1e-12 and abs(peak - 7.0) < 1e-12
    assert rm_refine([3.0, 2.0, 1.0], [0.0, 1.0, 2.0]) == (0.0, 3.0) and rm_refine([1.0, 1.0, 1.0], [0.0, 1.0, 2.0], 1) == (1.0, 1.0)
    snr, med, mad = rm_significance([1.0, 2.0, 3.0, 4.0, 100.0])
    assert (med, mad) == (3.0, 1.0) and abs(snr - 97.0 / 1.4826) < 1e-12 and rm_significance([2.0, 2.0, 2.0])[0] == 0.0
    assert abs(rm_error(0.35, 10.0) - 0.0175) < 1e-15 and rm_error(0.35, 0.0) == np.inf
    pp = pol_profile(np.array([[2.0, 0.0], [1.0, 5.0], [1.0, 5.0], [-1.0, 1.0]]))
    assert abs(pp['L'][0] - np.sqrt(2)) < 1e-15 and abs(pp['PA'][0] - np.pi / 8) < 1e-15 and abs(pp['frac_L'][0] - np.sqrt(0.5)) < 1e-15
    assert pp['frac_V'][0] == -0.5 and np.isnan(pp['frac_L'][1]) and np.isnan(pp['frac_V'][1])
    assert RM_RECORD == rmsynth_ref.RECORD and rm_offsets(2, 130, 40) == rmsynth_ref.offsets(2, 130, 40) == (32, 32 + 1040, 32 + 1040 + 1280)
    with pytest.raises(ValueError):
        as_rmsynth(np.zeros(100, np.uint8), 2, 130, 40)


# ---------------------------------------------------------------- the engine table and the C entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.RMSYNTH_ENGINES == [("Rmsynth", "rmsynth", True)]
    older = ffi.ENGINES + ffi.MORE_ENGINES + ffi.NEWER_ENGINES + ffi.NEWEST_ENGINES + ffi.LATEST_ENGINES + ffi.FURTHER_ENGINES + ffi.CUTOUT_ENGINES
    assert not {r[0] for r in ffi.RMSYNTH_ENGINES} & {r[0] for r in older} and not {r[1] for r in ffi.RMSYNTH_ENGINES} & {r[1] for r in older}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.RMSYNTH_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.RMSYNTH_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    L = ffi.lib()
    names = ["xengRmsynth" + n for n in ("Initialize", "SetTable", "SetMasks", "SetActive", "Run", "Reset", "GetInfo", "CheckGuards", "Mark", "Wait", "TicketDone",
                                         "Sync", "Destroy")]
    for name in names:
        assert hasattr(L, name) and name in ffi.SYMBOLS and name in test_engine_table_cpu.DECLARED, name
        assert (name in ffi.ENQUEUE_ONLY) == (name[11:] in ("Run", "Reset", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_table", "set_masks", "set_active", "run", "reset", "info", "guards_intact", "mark", "wait", "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "rmsynth_" + m)), m
    good = [2, 8, 16, 4, 0]                                         # (npair, nchg, nbin, nphi, feeds)
    for i, v in ((0, 0), (0, 65536), (1, 0), (1, 65537), (2, 0), (2, 65537), (3, 0), (3, 4097), (4, -1), (4, 2)):
        args = list(good)
        args[i] = v
        assert L.xengRmsynthInitialize(0, *args) == INVALID_ARGUMENT, args
    assert L.xengRmsynthInitialize(0, 1, 65536, 16, 4096, 0) == INVALID_ARGUMENT and b"table" in L.xengGetLastError()      # 2 GiB of table
    assert L.xengRmsynthInitialize(0, 65535, 8, 65536, 4, 0) == INVALID_ARGUMENT and b"4 GiB" in L.xengGetLastError()      # 17 GB of profiles
    if not _gpu_present():
        assert L.xengRmsynthInitialize(0, *good) not in (0, INVALID_ARGUMENT)          # (good sizes get as far as the device)
    for a, b in ((None, 16), (16, None), (20, 16), (16, 24)):
        assert L.xengRmsynthRun(a, b) == INVALID_ARGUMENT
    assert L.xengRmsynthGetInfo(None, None, None, None, None) == INVALID_ARGUMENT and L.xengRmsynthSetTable(None, None, None) == INVALID_ARGUMENT
    if not _gpu_present():
        n, k = ctypes.c_longlong(), ctypes.c_int()
        T = np.zeros((8, 4, 2), np.float32)
        assert L.xengRmsynthRun(16, 16) == INVALID_STATE and L.xengRmsynthReset() == INVALID_STATE
        assert L.xengRmsynthSetTable(T.ctypes.data_as(_pf), None, None) == INVALID_STATE and L.xengRmsynthSetMasks(None, None) == INVALID_STATE
        assert L.xengRmsynthSetActive(None) == INVALID_STATE
        assert L.xengRmsynthGetInfo(ctypes.byref(n), ctypes.byref(k), ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == INVALID_STATE


# ---------------------------------------------------------------- the restatement against the float64 statement
@pytest.mark.parametrize("feeds", [0, 1])
def test_on_integer_data_the_restatement_equals_the_float64_statement_exactly(feeds):
    """Integers 0..3 (cross words -2..2) in 2 pairs x 70 groups x 40 bins, 8 off-pulse bins (the baseline is a multiple of 1/8: every
    float32 step is exact), weights of 0, 1 and 2, and the phi = 0 column of the table alone (Tc = w, Ts = 0): records, spectrum and
    profile equal rm_reference's float64 values word for word (every sum stays an integer multiple of 1/64 below 2^24)."""
    w = np.ones(70)
    w[::3] = 2
    w[list(rmsynth_cases.LEFT_OUT)] = 0
    T, wf, use, _ = rm_table(rmsynth_cases.FREQS, [0.0], w)
    assert np.array_equal(T[:, 0, 0], wf) and not T[:, 0, 1].any()
    X = rmsynth_cases.poison_left_out(rmsynth_cases.integer_scene(3 + feeds, 2, 70, 40), use)
    off = np.zeros((2, 40), np.uint8)
    off[0, :8], off[1, 30:38] = 1, 1
    on = np.zeros((2, 40), np.uint8)
    on[:, 12:29] = 1
    rec, spec, prof = rmsynth_ref.rmsynth(X, T, wf, use, off, on, None, feeds)
    e = rm_reference(np.where(np.isfinite(X), X, 0), T, wf, use, off, on, None, feeds)
    assert np.array_equal(spec.astype(np.float64), e['spec']) and np.array_equal(prof.astype(np.float64), e['prof']) and e['spec'].max() * 64 < 2 ** 24
    assert rec['k'].tolist() == e['k'].tolist() == [0, 0] and rec['peak'].astype(np.float64).tolist() == e['peak'].tolist()
    assert rec['n_on'].tolist() == [17, 17] and rec['n_off'].tolist() == [8, 8] and spec.min() > 0


# ---------------------------------------------------------------- the block on CPU rings
class RmsynthBackend(OracleBackend):
    """The oracle backend plus xengRmsynth* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.k, self.calls, self.tab, self.masks, self.active = None, [], None, (None, None), None

    def rmsynth_initialize(self, gpu, npair, nchg, nbin, nphi, feeds):
        self.k = dict(npair=npair, nchg=nchg, nbin=nbin, nphi=nphi, feeds=feeds)
        self.calls.append(('init', npair, nchg, nbin, nphi, feeds))
        return 0

    def rmsynth_set_table(self, T, w=None, use=None):
        assert T.dtype == np.float32 and T.shape == (self.k['nchg'], self.k['nphi'], 2) and T.flags.c_contiguous
        self.tab = (T.copy(), w.copy(), use.copy())
        self.calls.append('set_table')
        return 0

    def rmsynth_set_masks(self, off=None, on=None):
        for m in (off, on):
            assert m is None or (m.dtype == np.uint8 and m.shape == (self.k['npair'], self.k['nbin']))
        self.masks = (off, on)
        self.calls.append('set_masks')
        return 0

    def rmsynth_set_active(self, active=None):
        self.active = None if active is None else active.copy()
        self.calls.append(('set_active', None if active is None else active.tolist()))
        return 0

    def rmsynth_run(self, in_arr, out_arr):
        k = self.k
        X = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(k['npair'], 4, k['nchg'], k['nbin'])
        out = rmsynth_ref.out_bytes(*rmsynth_ref.rmsynth(X, *self.tab, self.masks[0], self.masks[1], self.active, k['feeds']))
        out_arr.numpy().reshape(-1).view(np.uint8)[...] = out
        self.calls.append('run')
        return 0

    def rmsynth_reset(self):
        self.calls.append('reset')

    def rmsynth_mark(self):
        return self.beam_mark()

    def rmsynth_wait(self, ticket):
        self.beam_wait(ticket)

    def rmsynth_sync(self):
        pass


NPAIR, NCHAN, NUP, NFSCR, NBIN = 2, 2, 8, 2, 12
NCHG = NCHAN * NUP // NFSCR
PHIS = rmsynth_cases.phis(9, 0.2)
PSR = dict(f0=2.0, f1=0.0, pepoch=0.0, dm=1.0)


def fold_header(seq0=0, **extra):
    """The sequence header BeamFold(stokes='full') writes (beam_fold_block.py output_header) over 60 to 79.6 MHz."""
    chan_bw = 19.6e6 / NCHAN
    hdr = source_header(NCHAN, NPAIR, 2, seq0=seq0, sfreq=60e6, chan_bw=chan_bw)
    hdr.update(nstand=NPAIR, nbeam=NPAIR, npol=2, complex=True, nbit=32, nupchan=NUP, nframe_sum=1, fine_bw_hz=chan_bw / NUP, fine_sfreq=60e6, pair0=0,
               acc_len=NUP, nbin=NBIN, nfscr=NFSCR, nprod=4, tsamp=1e-3, nsub=2, pulsars=[PSR, PSR], normalise=True, hits=[[1] * NBIN] * NPAIR,
               subint_start=seq0, subint_nwindow=8)
    hdr.update(extra)
    return hdr


def _block(seqs, be=None, **kw):
    be = be or RmsynthBackend()
    r1 = Ring("rm-output")
    nbytes = NPAIR * 4 * NCHG * NBIN * 4
    blk = BeamRmSynth(LOG, _FakeRing([_FakeSeq(h, [(0, x)], nbytes) for h, x in seqs]), r1, backend=be, **dict(dict(npair=NPAIR, nchg=NCHG, nbin=NBIN, phis=PHIS), **kw))
    return blk, be, Sink(r1, rm_offsets(NPAIR, PHIS.size, NBIN)[2])


def test_block_writes_one_sequence_per_sub_integration_with_the_header_keys_an_inactive_pair_and_commands():
    """Four sub-integrations.  The first with both pairs; the second's header has no pulsar for pair 1 (inactive: -1 and +0); before
    the third a `masks` command (on = bins 3..6, off = the rest, for both pairs) and before the fourth a `weights` command that
    leaves group 2 out: each holds from the next span, and the table is made again for the weights only."""
    x = [rmsynth_cases.float_scene(40 + i, NPAIR, NCHG, NBIN) for i in range(4)]
    hdrs = [fold_header(0), fold_header(100, pulsars=[PSR, None]), fold_header(200), fold_header(300)]
    on = np.zeros((NPAIR, NBIN), np.uint8)
    on[:, 3:7] = 1
    blk, be, sink = _block(list(zip(hdrs, x)), feeds='circular')
    wnew = [1.0, 1.0, 0.0, 1.0, 0.5, 1.0, 1.0, 1.0]
    seen = []

    def on_span(hdr, n):
        seen.append(hdr['seq0'])
        if hdr['seq0'] == 100:
            blk.process_command_strings(json.dumps({'cmd': 'update', 'id': '1', 'val': {'kwargs': {'masks': dict(off=(1 - on).tolist(), on=on.tolist())}}}))
        if hdr['seq0'] == 200:
            blk.process_command_strings(json.dumps({'cmd': 'update', 'id': '2', 'val': {'kwargs': {'weights': wnew}}}))
        gate.set()
    gate = threading.Event()
    sink.on_span = on_span
    # (the fake input ring hands the sequences over at once: run the block from the sink's side span by span)
    orig = blk._check_header
    first = [True]

    def stepped(ihdr):
        if not first[0]:
            assert gate.wait(20)
            gate.clear()
        first[0] = False
        orig(ihdr)
    blk._check_header = stepped
    sink.start()
    blk.main()
    sink.join(20)
    assert seen == [0, 100, 200, 300] and len(sink.sequences) == 4 and all(len(s[2]) == 1 for s in sink.sequences)
    freqs = 60e6 + (19.6e6 / NCHAN / NUP) * (NFSCR * np.arange(NCHG) + 0.5)
    assert np.array_equal(blk.group_frequencies(hdrs[0]), freqs)
    T0, w0, use0, lam0 = rm_table(freqs, PHIS, None)
    T1, w1, use1, lam1 = rm_table(freqs, PHIS, wnew)
    a, b, n = rm_offsets(NPAIR, PHIS.size, NBIN)
    want = [(T0, w0, use0, None, None, None, lam0), (T0, w0, use0, None, None, np.array([1, 0], np.uint8), lam0),
            (T0, w0, use0, 1 - on, on, None, lam0), (T1, w1, use1, 1 - on, on, None, lam1)]
    for (hd, tag, spans), h, xi, (T, w, use, off, onm, act, lam) in zip(sink.sequences, hdrs, x, want):
        assert tag == h['seq0'] and hd['rm_phis'] == PHIS.tolist() and hd['lambda0_sq'] == lam and hd['rm_feeds'] == 'circular'
        assert (hd['record_offset'], hd['spec_offset'], hd['profile_offset'], hd['span_bytes']) == (0, a, b, n) and hd['nbin'] == NBIN and hd['nprod'] == 4
        assert hd['rm_n_on'] == ([NBIN] * 2 if onm is None else [4, 4]) and hd['rm_n_off'] == ([NBIN] * 2 if off is None else [NBIN - 4] * 2)
        exp = rmsynth_ref.out_bytes(*rmsynth_ref.rmsynth(xi, T, w, use, off, onm, act, 1))
        assert spans[0].tobytes() == exp.tobytes()
        rec, spec, prof = as_rmsynth(spans[0], NPAIR, PHIS.size, NBIN)
        assert rec[0]['k'] >= 0 and (act is None or (rec[1].tolist() == (-1, 0.0, 0, 0) and not spec[1].any() and not prof[1].any()))
    assert be.calls[0] == ('init', NPAIR, NCHG, NBIN, 9, 1) and be.calls.count('set_table') == 2 and be.calls.count('run') == 4
    assert [c for c in be.calls if isinstance(c, tuple) and c[0] == 'set_active'] == [('set_active', [1, 1]), ('set_active', [1, 0]), ('set_active', [1, 1])]
    assert blk.stats['nsubint'] == 4 and blk.stats['npeak'] == 7


@pytest.mark.parametrize("change,msg", [(dict(nbin=None), "nbin"), (dict(nprod=1), "nprod"), (dict(rm_phis=[0.0]), "rm_phis"), (dict(nbin=16), "bins"),
                                        (dict(nfscr=4), "groups"), (dict(nbeam=3), "pairs"), (dict(fine_bw_hz=0.0), "fine_bw_hz")])
def test_block_refuses_what_is_not_a_folded_dual_pol_cube(change, msg):
    hdr = fold_header()
    for k, v in change.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    blk, be, _ = _block([(hdr, rmsynth_cases.float_scene(1, NPAIR, NCHG, NBIN))])
    with pytest.raises(ValueError, match=msg):
        blk.main()
    assert 'run' not in be.calls


@pytest.mark.parametrize("kw", [dict(npair=0), dict(nchg=0), dict(nbin=65537), dict(nchg=2.0), dict(phis=[]), dict(phis=[0.0, float('nan')]), dict(phis=np.zeros(4097)),
                                dict(feeds='both'), dict(weights=[1.0]), dict(weights=[0.0] * NCHG), dict(off=np.ones((NPAIR, NBIN + 1), np.uint8)),
                                dict(on=np.full((NPAIR, NBIN), 2, np.uint8))])
def test_constructor_refuses_bad_arguments(kw):
    be = RmsynthBackend()
    with pytest.raises(ValueError, match="BEAM_RM_SYNTH"):
        BeamRmSynth(LOG, Ring("a"), Ring("b"), backend=be, **dict(dict(npair=NPAIR, nchg=NCHG, nbin=NBIN, phis=PHIS), **kw))
    assert be.k is None


# ---------------------------------------------------------------- the planted scene
def test_planted_scene_the_float64_statement_finds_the_rotation_measure_and_derotates_the_pulse():
    """70 groups over 60 to 79.6 MHz, two of weight 0; 40 bins, a Gaussian pulse of sigma 2 bins at bin 20, 60 % linear with
    PA 0.3 + 0.05 (b - 20), RM 1.37 rad/m^2, Q and U offsets of +0.8 and -0.2, noise 0.3; off-pulse = the bins outside 12..28; 130
    depths of 0.05 rad/m^2 with 0 at k = 65.  The float64 statement peaks at k = 92 (phi = 1.35), the parabola refines it to within
    dphi / 4 of the planted value, and the peak stands 20 times or more above the spectrum's median; at the pulse's peak bin the
    band-summed |Q + iU| of the cube as it is (phi = 0) is below a third of the de-rotated one.  The restatement names the same k."""
    X, off, on = rmsynth_cases.planted()
    phis = rmsynth_cases.phis(130)
    assert phis[65] == 0 and abs(phis[92] - 1.35) < 1e-12
    T, w, use, lam0 = rm_table(rmsynth_cases.FREQS, phis, rmsynth_cases.weights())
    e = rm_reference(X, T, w, use, off, on, None, 0)
    k = int(e['k'][0])
    dphi = rmsynth_cases.DPHI
    assert k == 92 and abs(phis[k] - 1.37) <= dphi / 2
    phi, peak = rm_refine(e['spec'][0], phis)
    snr, med, _ = rm_significance(e['spec'][0])
    print("planted scene: k = %d, refined phi = %.4f, peak / median = %.1f, snr = %.1f" % (k, phi, e['peak'][0] / med, snr))
    assert abs(phi - 1.37) <= dphi / 4 and e['peak'][0] >= 20 * med and peak >= e['peak'][0]
    raw, derot = abs(e['F'][0, 20, 65]), abs(e['F'][0, 20, k])
    assert raw < derot / 3 and derot > 0.5 * 0.6 * 10.0 * 68
    pp = pol_profile(e['prof'][0])
    assert int(np.argmax(pp['L'])) == 20 and 0.5 < pp['L'][20] / (e['prof'][0, 0, 20]) < 0.7
    # the position angle across the pulse keeps its planted slope of 0.05 rad a bin
    assert abs(np.angle(np.exp(2j * (pp['PA'][22] - pp['PA'][18]))) / 2 - 0.2) < 0.05
    rec, spec, prof = rmsynth_ref.rmsynth(X, T, w, use, off, on, None, 0)
    assert rec[0]['k'] == k and np.allclose(spec[0], e['spec'][0], rtol=1e-4) and rec[0]['n_on'] == 17 and rec[0]['n_off'] == 23
