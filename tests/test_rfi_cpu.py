"""BeamRfiClean without a GPU: the median, MAD and tree rules against brute force (ties, even counts, -0), rfi_controls, rfi_weights and
rfi_occupancy, the LATEST_ENGINES row under the per-row checks of tests/test_engine_table_cpu.py, the C entry points' argument
checks, the block on CPU rings with a backend that serves xengRfi* by the restatement (tests/rfi_ref.py) -- time alignment, the
uncommitted head, a gap, the `control` and `mask` commands' timing, the header, the constructor's refusals -- and a planted scene
(tests/golden/rfi_planted.npy) cleaned by the restatement and dedispersed by tests/dedisp_ref.py."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import BeamRfiClean, rfi_controls, rfi_mad, rfi_median, rfi_occupancy, rfi_tree_sum, rfi_weights
from caltech_bifrost_dsp_amd.ring import Ring
from tests import rfi_cases, rfi_ref, test_engine_table_cpu
from tests.dedisp_ref import dedisperse
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_dedisp_cpu import power_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfi_planted.npy")
F = np.float32


# ---------------------------------------------------------------- the median, the MAD and the tree
def _brute_median(v, live):
    """rank = the count of live entries below it, ties by index, compared as floats with -0 = +0"""
    idx = [i for i in range(len(v)) if live[i]]
    n = len(idx)
    if n == 0:
        return F(0)
    rank = {}
    for i in idx:
        rank[sum(1 for j in idx if v[j] < v[i] or (v[j] == v[i] and j < i))] = v[i]
    return rank[n // 2] if n & 1 else F(F(0.5) * F(rank[(n - 1) // 2] + rank[n // 2]))


@pytest.mark.parametrize("seed", range(6))
def test_median_and_mad_against_brute_force_with_ties_and_even_counts(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    v = rng.integers(-3, 4, n).astype(F) * F(0.1)               # few distinct values: many ties
    v[rng.random(n) < 0.2] = F(-0.0)
    live = rng.random(n) < 0.8
    med = rfi_median(v, live)
    assert med.tobytes() == np.asarray(_brute_median(v, live), F).tobytes()
    assert med.tobytes() == rfi_ref.median_ties_by_index(v, live).tobytes()
    m2, mad = rfi_mad(v, live)
    dev = np.abs(v - med)
    assert m2.tobytes() == med.tobytes() and mad.tobytes() == np.asarray(_brute_median(dev, live), F).tobytes()


def test_median_of_none_of_one_and_of_two():
    v = np.array([3.0, 1.0, 2.0, 1.0], F)
    assert rfi_median(v, np.zeros(4, bool)) == 0 and rfi_median(v, [0, 0, 1, 0]) == 2 and rfi_median(v, [1, 1, 0, 0]) == 2
    assert rfi_median(v) == F(1.5) and rfi_mad(np.array([1, 1, 1, 5], F)) == (1, 0)
    big = np.array([3e38, 3e38], F)
    assert np.isinf(rfi_median(big))                            # (lo + hi overflows before the halving: one float32 addition)


@pytest.mark.parametrize("nfine", [1, 7, 255, 256, 257, 300, 700])
def test_tree_sum_against_brute_force(nfine):
    rng = np.random.default_rng(nfine)
    y = (rng.standard_normal((nfine, 4)) * 10.0 ** rng.integers(-3, 4, (nfine, 1))).astype(F)
    P = [np.zeros(4, F) for _ in range(256)]
    for q in range(nfine):
        P[q % 256] = (P[q % 256] + y[q]).astype(F)
    h = 128
    while h:
        for t in range(h):
            P[t] = (P[t] + P[t + h]).astype(F)
        h //= 2
    assert rfi_tree_sum(y).tobytes() == P[0].tobytes() == rfi_ref.tree_sum(y).tobytes()


# ---------------------------------------------------------------- the host helpers
def test_rfi_controls_folds_the_constants_in():
    k, c, b, n = rfi_controls(nsig_chan=4.0, nsig_clip=5.0, nsig_broad=6.0, min_fraction=0.3, nfine=3072)
    assert (k, c, b, n) == (float(F(1.4826 * 4)), float(F(math.sqrt(2) * 5)), float(F(math.sqrt(2) * 6)), 922)
    assert rfi_controls(nfine=7, min_fraction=0.0)[3] == 0 and rfi_controls(nfine=7, min_fraction=1.0)[3] == 7
    for kw in (dict(nsig_chan=0.0), dict(nsig_clip=float('nan')), dict(nsig_broad=float('inf')), dict(nsig_chan=-1), dict(min_fraction=1.5),
               dict(min_fraction=-0.1), dict(nsig_clip=True), dict(nsig_chan="4")):
        with pytest.raises(ValueError):
            rfi_controls(nfine=16, **kw)
    with pytest.raises(ValueError):
        rfi_controls()
    with pytest.raises(ValueError):
        rfi_controls(nfine=0)


def test_rfi_weights_and_occupancy():
    flags = np.array([[0, 1, 0, 4, 0], [0, 0, 2, 0, 0]], np.uint8)
    assert rfi_weights(flags).tolist() == [1, 0, 0, 0, 1] and rfi_weights(flags).dtype == np.float32 and rfi_weights(flags[1]).tolist() == [1, 1, 0, 1, 1]
    with pytest.raises(ValueError):
        rfi_weights(np.zeros((2, 2, 2)))
    # two pairs of 10 channels: pair 0 loses 1 + 1 of 10 in a good window, everything in a flagged one; pair 1 is dead
    stats = np.array([[[0, 0, 4, 0], [0, 0, 4, 0]], [[8, 1, 0, 1], [0, 0, 1, 10]], [[9, 0, 2, 1], [0, 0, 1, 10]]], np.int32)
    assert rfi_occupancy(stats).tolist() == [(2 + 10) / 20.0, 1.0]
    assert np.isnan(rfi_occupancy(stats[:1])).all()


# ---------------------------------------------------------------- the engine table and the C entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.LATEST_ENGINES == [("Rfi", "rfi", True)]
    older = ffi.ENGINES + ffi.MORE_ENGINES + ffi.NEWER_ENGINES + ffi.NEWEST_ENGINES
    assert not {r[0] for r in ffi.LATEST_ENGINES} & {r[0] for r in older} and not {r[1] for r in ffi.LATEST_ENGINES} & {r[1] for r in older}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.LATEST_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.LATEST_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported, declared and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are
    not; HipBackend has a method for each.  Initialize refuses every size outside the contract's ranges before it touches a device;
    SetControl refuses floats that are not finite and positive, and Run and the getters null and misaligned pointers, before
    looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    names = ["xengRfi" + n for n in ("Initialize", "SetControl", "SetMask", "Run", "Reset", "GetInfo", "GetBlock", "CheckGuards", "Mark", "Wait", "TicketDone", "Sync",
                                     "Destroy")]
    for name in names:
        assert hasattr(L, name) and name in ffi.SYMBOLS and name in test_engine_table_cpu.DECLARED, name
        assert (name in ffi.ENQUEUE_ONLY) == (name[7:] in ("Run", "Reset", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_control", "set_mask", "run", "reset", "info", "block", "guards_intact", "mark", "wait", "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "rfi_" + m)), m
    good = [2, 64, 4, 8]                        # (npair, nfine, nwin, nstat)
    for i, v in ((0, 0), (0, 65536), (1, 3), (1, 8193), (2, 0), (2, 9), (3, 1), (3, (1 << 20) + 1)):
        args = list(good)
        args[i] = v
        assert L.xengRfiInitialize(0, *args) == INVALID_ARGUMENT, args
    assert L.xengRfiInitialize(0, 16, 8192, 1 << 10, 1 << 11) == INVALID_ARGUMENT          # 3072 windows of 2 MiB: above XENG_RFI_MAX_HISTORY_BYTES
    assert b"history" in L.xengGetLastError()
    assert L.xengRfiInitialize(0, 16, 8192, 1 << 10, 1 << 10) == INVALID_ARGUMENT          # exactly 2^32 bytes: not below the limit
    if not _gpu_present():
        assert L.xengRfiInitialize(0, *good) not in (0, INVALID_ARGUMENT)                  # (good sizes get as far as the device)
    for ctl in ((0.0, 1.0, 1.0, 1, 1), (1.0, float('nan'), 1.0, 1, 1), (1.0, 1.0, float('inf'), 1, 1), (-1.0, 1.0, 1.0, 1, 1), (1.0, 1.0, 1.0, 1, 2)):
        assert L.xengRfiSetControl(*ctl) == INVALID_ARGUMENT, ctl
    comp = ctypes.c_int(-1)
    for args in ((None, 1, 16, 16, ctypes.byref(comp)), (16, 1, None, 16, ctypes.byref(comp)), (16, 1, 16, None, ctypes.byref(comp)), (16, 1, 16, 16, None),
                 (20, 1, 16, 16, ctypes.byref(comp)), (16, 1, 24, 16, ctypes.byref(comp)), (16, 1, 16, 8, ctypes.byref(comp))):
        assert L.xengRfiRun(*args) == INVALID_ARGUMENT
    assert L.xengRfiGetInfo(None, None) == INVALID_ARGUMENT and L.xengRfiGetBlock(None, None, None, None, None) == INVALID_ARGUMENT
    if not _gpu_present():
        n = ctypes.c_longlong()
        assert L.xengRfiRun(16, 1, 16, 16, ctypes.byref(comp)) == INVALID_STATE and L.xengRfiReset() == INVALID_STATE
        assert L.xengRfiSetControl(1.0, 1.0, 1.0, 1, 1) == INVALID_STATE and L.xengRfiSetMask(None) == INVALID_STATE
        assert L.xengRfiGetInfo(ctypes.byref(n), ctypes.byref(n)) == INVALID_STATE and comp.value == -1


# ---------------------------------------------------------------- the block on CPU rings
class RfiBackend(OracleBackend):
    """The oracle backend plus xengRfi* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.rf, self.calls = None, []

    def rfi_initialize(self, gpu, npair, nfine, nwin, nstat):
        self.rf = rfi_ref.RfiRef(npair, nfine, nstat)
        self.dims = (nwin, npair, nfine)
        self.calls.append(('init', nwin, nstat))
        return 0

    def rfi_set_control(self, k_chan, t_clip, t_broad, min_count, zerodm):
        self.rf.set_control(k_chan, t_clip, t_broad, min_count, zerodm)
        self.calls.append(('control', self.rf.n, int(zerodm)))
        return 0

    def rfi_set_mask(self, mask):
        self.rf.set_mask(mask)
        self.calls.append(('mask', self.rf.n))
        return 0

    def rfi_run(self, in_arr, nwin_call, out_arr, stats_arr):
        assert 1 <= nwin_call <= self.dims[0]
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape((nwin_call,) + self.dims[1:] + (4,))
        before = self.rf.nblocks
        out, st = self.rf.run(x)
        out_arr.numpy().reshape(-1).view(np.uint8)[...] = np.frombuffer(out.tobytes(), np.uint8)
        stats_arr.numpy().reshape(-1).view(np.uint8)[...] = np.frombuffer(st.tobytes(), np.uint8)
        self.calls.append('run')
        return 0, int(self.rf.nblocks > before)

    def rfi_block(self, npair, nfine):
        return self.rf.block

    def rfi_reset(self):
        self.rf.reset()
        self.calls.append('reset')

    def rfi_mark(self):
        return self.beam_mark()

    def rfi_wait(self, ticket):
        self.beam_wait(ticket)

    def rfi_sync(self):
        pass


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


BLK = dict(npair=2, nchan=2, nupchan=8, nwin=4, nstat=8)
NFINE, NWIN, NSTAT, HEAD = 16, 4, 8, 2
SPAN = NWIN * BLK['npair'] * NFINE * 16
CTL = dict(nsig_chan=4.0, nsig_clip=5.0, nsig_broad=5.0, min_fraction=0.25)


def _reference(x, events=(), zerodm=True, **ctl):
    """The restatement over the spans of x; events: {span index: ('control', dict) or ('mask', array)} given before that span.
    Returns the outputs per call."""
    c = dict(CTL, zerodm=zerodm)
    c.update(ctl)
    ref = rfi_ref.RfiRef(BLK['npair'], NFINE, NSTAT)
    ref.set_control(*(rfi_controls(nfine=NFINE, **dict((k, c[k]) for k in CTL)) + (int(c['zerodm']),)))
    outs = []
    for j in range(x.shape[0] // NWIN):
        for kind, v in events.get(j, ()) if isinstance(events, dict) else ():
            if kind == 'mask':
                ref.set_mask(v)
            else:
                c.update(v)
                ref.set_control(*(rfi_controls(nfine=NFINE, **dict((k, c[k]) for k in CTL)) + (int(c['zerodm']),)))
        outs.append(ref.run(x[j * NWIN:(j + 1) * NWIN]))
    return outs


def test_block_is_time_aligned_leaves_the_head_uncommitted_and_writes_the_header():
    """7 spans of 4 windows, blocks of 8: every span is enqueued, the first two outputs (what lies before the sequence) are not
    committed, and output span j is the cleaned input span j: the output sequence has the input's seq0 and time tag, 5 spans; the
    tail of 8 windows is not flushed.  The header is the input's plus the rfi_ keys; the stats count windows and blocks."""
    seq0, acc_len = 4096, 32
    x = rfi_cases.scene(21, 7 * NWIN, BLK['npair'], NFINE, NSTAT)
    hdr = power_header(BLK['nchan'], BLK['npair'], BLK['nupchan'], acc_len // BLK['nupchan'], seq0=seq0)
    be = RfiBackend()
    rc = BeamRfiClean(LOG, Ring("ub-output"), Ring("rc-output"), backend=be, **dict(BLK, **CTL))
    sink = Sink(rc.oring, SPAN)
    run_blocks([rc], Source(rc.iring, [(hdr, x, SPAN)]), [sink])
    (hd, tag, spans), = sink.sequences
    assert tag == seq0 == hd['seq0'] and len(spans) == 7 - HEAD
    exp = _reference(x)
    assert [s.tobytes() for s in spans] == [o.tobytes() for o, _ in exp[HEAD:]] and any(o.any() for o, _ in exp[HEAD:])
    assert (hd['rfi_cleaned'], hd['rfi_nstat'], hd['rfi_zerodm']) == (True, NSTAT, True)
    assert (hd['rfi_nsig_chan'], hd['rfi_nsig_clip'], hd['rfi_nsig_broad'], hd['rfi_min_fraction']) == (4.0, 5.0, 5.0, 0.25)
    assert all(hd[k] == v for k, v in hdr.items() if k != 'seq0')
    assert be.calls == [('init', NWIN, NSTAT), ('control', 0, 1)] + ['run'] * 7
    assert rc.stats['nwindow'] == 28 and rc.stats['nblock'] == 3 and rc.stats['ngap'] == 0
    occ = rfi_occupancy(np.concatenate([st for _, st in exp[HEAD:]]))
    tot = np.concatenate([st for _, st in exp[HEAD:]]).astype(np.int64)
    lost = np.where(tot[..., 2] == 0, NFINE - tot[..., 0], NFINE).sum()
    assert abs(rc.stats['frac_samples'] - lost / (tot.shape[0] * tot.shape[1] * NFINE)) < 1e-12 and 0 < occ.min()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rc.flags(), be.rf.block))
    # a cleaned ring is not cleaned again
    rc2 = BeamRfiClean(LOG, _FakeRing([_FakeSeq(hd, [(0, x[:NWIN])], SPAN)]), Ring("x"), backend=RfiBackend(), **BLK)
    with pytest.raises(ValueError, match="cleaned already"):
        rc2.main()


def test_block_gap_resets_and_commands_hold_from_the_next_block():
    """Spans 0..4 and 6..14 of a sequence (5 never read): the first output sequence has spans 0..2 (cleaned input 0..2), the gap resets
    the context and the output restarts at span 6's time in a sequence of its own, again two spans short.  A `control` command
    (zerodm off) and a `mask` command before span 9 -- inside the block of spans 8, 9 -- leave the blocks decided before alone and
    hold from that block on; a command with an unknown key or a mask of the wrong length is refused."""
    seq0, acc_len = 640, 32
    x = rfi_cases.scene(22, 15 * NWIN, BLK['npair'], NFINE, NSTAT)
    hdr = power_header(BLK['nchan'], BLK['npair'], BLK['nupchan'], acc_len // BLK['nupchan'], seq0=seq0)
    mask = [0] * NFINE
    mask[6] = mask[11] = 1
    be, r1, box = RfiBackend(), Ring("rc-output"), {}

    def spans():
        for k in list(range(5)) + list(range(6, 15)):
            if k == 9:
                box['rc'].process_command_strings(_cmd(control=dict(zerodm=False, nsig_clip=4.0)))
                assert box['rc'].last_response['val']['status'] == 'normal'
                box['rc'].process_command_strings(_cmd("2", mask=mask))
                assert box['rc'].last_response['val']['status'] == 'normal'
                box['rc'].process_command_strings(_cmd("3", control=dict(nsig=3.0)))
                assert box['rc'].last_response['val']['status'] == 'error'
                box['rc'].process_command_strings(_cmd("4", mask=[0, 1]))
                assert box['rc'].last_response['val']['status'] == 'error'
            yield k, np.ascontiguousarray(x[k * NWIN:(k + 1) * NWIN])

    rc = box['rc'] = BeamRfiClean(LOG, _FakeRing([_FakeSeq(hdr, spans(), SPAN)]), r1, backend=be, **dict(BLK, **CTL))
    sink = Sink(r1, SPAN)
    sink.start()
    rc.main()
    sink.join(20)
    (h0, t0, s0), (h1, t1, s1) = sink.sequences
    step = NWIN * acc_len
    assert (t0, t1) == (seq0, seq0 + 6 * step) and (h0['seq0'], h1['seq0']) == (t0, t1) and (len(s0), len(s1)) == (5 - HEAD, 9 - HEAD)
    assert [s.tobytes() for s in s0] == [o.tobytes() for o, _ in _reference(x[:5 * NWIN])[HEAD:]]
    events = {3: [('control', dict(zerodm=False, nsig_clip=4.0)), ('mask', mask)]}          # span 9 is the fourth after the gap
    exp = _reference(x[6 * NWIN:], events)
    assert [s.tobytes() for s in s1] == [o.tobytes() for o, _ in exp[HEAD:]]
    plain = _reference(x[6 * NWIN:])
    same = [a[0].tobytes() == b[0].tobytes() for a, b in zip(exp, plain)]
    assert same[:4] == [True] * 4 and not any(same[4:])         # (calls 2, 3 write block 0, decided before the commands; call 4 on, block 1)
    assert be.calls == [('init', NWIN, NSTAT), ('control', 0, 1)] + ['run'] * 5 + ['reset'] + ['run'] * 3 + [('control', 12, 0), ('mask', 12)] + ['run'] * 6
    assert rc.stats['ngap'] == 1 and rc.stats['nwindow'] == 14 * NWIN
    # the Python entries
    rc.set_control(nsig_chan=7.0)
    rc.set_mask(None)
    assert rc._control['nsig_chan'] == 7.0 and rc._control['zerodm'] is False and not rc._mask.any() and rc.update_pending
    for bad in (dict(nsig_chan=0.0), dict(min_fraction=2.0), dict(unknown=1.0), dict(zerodm="yes")):
        with pytest.raises(ValueError, match="BEAM_RFI_CLEAN"):
            rc.set_control(**bad)
    with pytest.raises(ValueError, match="BEAM_RFI_CLEAN"):
        rc.set_mask([1, 0])


@pytest.mark.parametrize("kw", [dict(npair=0), dict(npair=65536), dict(nchan=1, nupchan=2), dict(nchan=2, nupchan=8192), dict(nwin=0), dict(nstat=1), dict(nwin=16),
                                dict(nstat=10), dict(nstat=(1 << 20) + 4), dict(npair=4096, nchan=64, nupchan=64, nstat=64), dict(nsig_chan=0.0),
                                dict(nsig_clip=float('nan')), dict(min_fraction=1.5), dict(zerodm=None), dict(mask=[1, 0]), dict(nwin=2.0)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(BLK)
    args.update(kw)
    be = RfiBackend()
    with pytest.raises(ValueError, match="BEAM_RFI_CLEAN"):
        BeamRfiClean(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.rf is None


# ---------------------------------------------------------------- the planted scene
NSIG_CHAN = 10.0


def _clean(x, zerodm=True):
    """The restatement over the scene in calls of a block; (cleaned windows 0..447, their stats, the flags of the 8 blocks)."""
    P = rfi_cases.PLANTED
    ref = rfi_ref.RfiRef(1, P['nfine'], P['nstat'])
    ref.set_control(*rfi_cases.controls(P['nfine'], zerodm=zerodm, min_fraction=0.5, nsig_chan=NSIG_CHAN))
    outs, stats, flags = [], [], []
    for k in range(P['nwindows'] // P['nstat']):
        o, st = ref.run(x[k * P['nstat']:(k + 1) * P['nstat']])
        outs.append(o)
        stats.append(st)
        flags.append(ref.block[0][0].copy())
    return np.concatenate(outs)[P['nstat']:], np.concatenate(stats)[P['nstat']:], flags


@pytest.fixture(scope="module")
def planted():
    x = np.load(GOLDEN)
    assert x.shape == (512, 1, 32, 4) and x.dtype == np.float32
    return dict(x=x, dirty=_clean(x), quiet=_clean(rfi_cases.planted_scene(interference=False)))


def test_planted_scene_flags_the_bursting_and_the_dead_channel_in_the_blocks_they_spoil_and_no_other(planted):
    """The fixture is rfi_cases.planted_scene() as it was written out once: one pair, 32 channels x 512 windows, chi-squared noise on a
    bandpass of 10:1, channel 9 bursting in blocks 2 and 5, channel 20 dead, a broadband impulse at window 200, a pulse dispersed
    over 16 windows from window 300.  Thresholds: 5 sigma on samples and windows; 10 robust sigma on channels -- R of 64 windows
    scatters by 13 % and its MAD over 32 channels is itself uncertain (in block 6 of the fixture it comes out at a third of the
    expected 0.088 med, which puts four clean channels at 5 to 7 'sigma'), while the bursts raise R eighty-fold, hundreds of sigma.
    Recorded from the restatement: flags {2: [9], 5: [9]} with bit 2, channel 20 with bit 1 in all 8 blocks, nothing else; window 200
    {count 28, clipped 3, code 2, not kept 1} and no other window with a code."""
    P = rfi_cases.PLANTED
    out, st, flags = planted['dirty']
    for k, f in enumerate(flags):
        exp = np.zeros(P['nfine'], np.uint8)
        exp[P['dead_chan']] = 2
        if k in P['burst_blocks']:
            exp[P['burst_chan']] = 4
        assert f.tolist() == exp.tolist(), k
    assert all(not f.any() for f in planted['quiet'][2])
    assert np.flatnonzero(st[:, 0, 2]).tolist() == [P['impulse_at']] and st[P['impulse_at'], 0].tolist() == [28, 3, 2, 1]
    assert not planted['quiet'][1][:, 0, 2].any() and not out[P['impulse_at']].any()
    assert not out[:, 0, P['dead_chan']].any() and not out[128:192, 0, P['burst_chan']].any() and out[192:256, 0, P['burst_chan']].any()


def test_planted_scene_keeps_the_dispersed_pulse_and_removes_the_impulse(planted):
    """Dedispersed by tests/dedisp_ref.py at zero DM and at the pulse's sweep.  Recorded from the restatement: the pulse's peak at its
    own trial is 128.15 with the interference and 133.34 without (ratio 0.961; the floor of one half is the requirement set for this stage), and it is the
    maximum of its trial in both; the zero-DM trial reads 1.5e-8 where the impulse was (the window is dropped, and zerodm leaves
    rounding errors in that trial everywhere), against 439 above the mean -- half the pulse's 851 -- in the raw scene."""
    P = rfi_cases.PLANTED
    s = rfi_cases.planted_delays()
    S = int(s.max())
    assert S == P['sweep'] > 8
    dirty = dedisperse(planted['dirty'][0], s)[:, 0, :, 0]
    quiet = dedisperse(planted['quiet'][0], s)[:, 0, :, 0]
    n, ni = P['pulse_at'] + S, P['impulse_at'] + S
    print("pulse with interference %.3f, without %.3f, zero-DM at the impulse %.3g" % (dirty[n, 1], quiet[n, 1], dirty[ni, 0]))
    assert dirty[n, 1] >= 0.5 * quiet[n, 1] > 0 and dirty[:, 1].argmax() == n == quiet[:, 1].argmax()
    assert abs(dirty[ni, 0]) < dirty[n, 1] and np.abs(dirty[:, 0]).max() < 1e-4
    raw = dedisperse(planted['x'][:448], s)[:, 0, :, 0]
    assert raw[ni, 0] - raw[:, 0].mean() > 0.4 * (raw[n, 1] - raw[:, 1].mean())      # (what the search behind would have seen)
    # without zerodm the impulse's window is dropped all the same
    plain = dedisperse(_clean(planted['x'], zerodm=False)[0], s)[:, 0, :, 0]
    assert abs(plain[ni, 0]) < 3 * plain[:, 0].std() and plain[n, 1] > 100
