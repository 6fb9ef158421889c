"""BeamDedisperse without a GPU, both ring implementations: dm_delays against the cold-plasma formula at a header's
frequencies; the restatement (tests/dedisp_ref.py) against a term-by-term loop and on an injected dispersed pulse; the block on
CPU rings with a backend that keeps the context's state (the windows since the reset, the table, the weights) -- spans within
and across sequences, the output header, a gap (reset, a new output sequence), a weights command landing at the next span,
max_delay given or taken from the table, refusals -- and the C entry points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import BeamDedisperse, dm_delays
from caltech_bifrost_dsp_amd.blocks.dedisp import KDM
from caltech_bifrost_dsp_amd.ring import Ring
from tests import dedisp_cases
from tests.dedisp_ref import dedisperse, dedisperse_naive, dedisperse_one_chain32, dedisperse_ordered32
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
CHAN_BW = 23925.78125
SFREQ = 20e6                                    # (low enough that a DM of 0.1 crosses two coarse channels in a few windows)
DMS = [0.0, 0.05, 0.1, 0.2]


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def power_header(nchan, npair, N, W, seq0=0, **extra):
    """The sequence header UpchanSumBeams writes (upchan_sum_beams_block.py output_header)."""
    hdr = source_header(nchan, npair, 2, seq0=seq0, sfreq=SFREQ, chan_bw=CHAN_BW)
    hdr.update(nstand=npair, nbeam=npair, npol=2, complex=True, nbit=32, nupchan=N, nframe_sum=W, fine_bw_hz=CHAN_BW / N,
               fine_sfreq=SFREQ - CHAN_BW / 2, pair0=0, acc_len=W * N)
    hdr.update(extra)
    return hdr


def header_table(hdr, nfine, dms=DMS):
    """The table the block must build: the formula written out at the header's fine-channel centres."""
    tsamp = hdr['acc_len'] * hdr['nchan'] / hdr['bw_hz']
    f_mhz = (hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(nfine)) * 1e-6
    s = np.array([[round(KDM * dm * (f ** -2 - f_mhz[-1] ** -2) / tsamp) for f in f_mhz] for dm in dms])
    return s.astype(np.int32), tsamp


def _powers(rng, nwindows, npair, nfine):
    return rng.integers(0, 50, (nwindows, npair, nfine, 4)).astype(np.float32)


def _cmd(weights, seq_id="1"):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': {'weights': weights}}})


class DedispBackend(OracleBackend):
    """The oracle backend plus xengDedisp* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.dd, self.calls = None, []

    def dedisp_initialize(self, gpu, npair, nfine, nwin, ndm, max_delay, nprod):
        self.dd = dict(npair=npair, nfine=nfine, nwin=nwin, ndm=ndm, max_delay=max_delay, nprod=nprod)
        self.s, self.w, self.x = None, None, []
        self.calls.append(('init', max_delay))
        return 0

    def dedisp_set_delays(self, delays):
        u = self.dd
        assert delays.dtype == np.int32 and delays.shape == (u['ndm'], u['nfine']) and delays.flags.c_contiguous
        if delays.min() < 0 or delays.max() > u['max_delay']:
            return INVALID_ARGUMENT
        self.s, self.x = delays.copy(), []
        self.calls.append('set_delays')
        return 0

    def dedisp_set_weights(self, weights):
        assert weights is None or (weights.dtype == np.float32 and weights.shape == (self.dd['nfine'],))
        self.w = None if weights is None else weights.copy()
        self.calls.append('set_weights')
        return 0

    def dedisp_run(self, in_arr, nwin_call, out_arr):
        u = self.dd
        assert self.s is not None and 1 <= nwin_call <= u['nwin']
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, u['npair'], u['nfine'], 4)
        self.x.append(x.copy())
        y = dedisperse(np.concatenate(self.x), self.s, self.w, u['nprod'])[-nwin_call:]
        out_arr.numpy().reshape(-1).view(np.uint8).view(np.float32)[...] = y.reshape(-1)
        self.calls.append('run')
        return 0

    def dedisp_reset(self):
        self.x = []
        self.calls.append('reset')

    def dedisp_mark(self):
        return self.beam_mark()

    def dedisp_wait(self, ticket):
        self.beam_wait(ticket)

    def dedisp_sync(self):
        pass


# ---------------------------------------------------------------- the table
def test_dm_delays_is_the_formula_at_the_headers_frequencies():
    """rint(KDM * DM * (f^-2 - f_ref^-2) / tsamp), f in MHz, f_ref the top channel by default: delay 0 there and at DM 0,
    ascending with DM and towards low frequencies; at 50 MHz a DM of 10 crosses the 96 coarse channels in about 1.4 s."""
    hdr = power_header(3, 2, 8, 4)
    s, tsamp = header_table(hdr, 24)
    freqs = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(24)
    got = dm_delays(freqs, DMS, tsamp)
    assert got.dtype == np.int32 and got.shape == (4, 24) and np.array_equal(got, s)
    assert (got[0] == 0).all() and (got[:, -1] == 0).all() and (np.diff(got, axis=1) <= 0).all() and (np.diff(got, axis=0) >= 0).all()
    assert got.max() > 4
    band = 50e6 + CHAN_BW * np.arange(96)
    assert abs(dm_delays(band, [10.0], 1e-3)[0, 0] - 1400) < 40
    lo = dm_delays(freqs, [0.1], tsamp, f_ref_hz=2 * freqs[-1])             # (a reference above the band: every delay grows)
    assert (lo[0] > got[2]).all()
    for bad in (dict(dms=[-1.0]), dict(f_ref_hz=freqs[0]), dict(tsamp_s=0.0), dict(dms=[]), dict(freqs_hz=[0.0, 1e6])):
        kw = dict(freqs_hz=freqs, dms=[0.1], tsamp_s=tsamp)
        kw.update(bad)
        with pytest.raises(ValueError, match="dm_delays"):
            dm_delays(**kw)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("nprod", [1, 4])
def test_restatement_is_the_definition(nprod):
    """Against one term at a time: weights with zeros, a NaN and an Inf in the channels left out, S larger than the run."""
    rng = np.random.default_rng(3 + nprod)
    nwindows, npair, nfine, ndm = 9, 2, 7, 3
    x = rng.standard_normal((nwindows, npair, nfine, 4))
    s = rng.integers(0, 6, (ndm, nfine))
    w = rng.uniform(0.5, 1.5, nfine)
    w[[1, 4]] = 0
    exp = dedisperse_naive(x, s, w, nprod)
    x[2, :, 1] = np.nan
    x[5, 1, 4, 0] = np.inf
    got = dedisperse(x, s, w, nprod)
    assert got.shape == (nwindows, npair, ndm, nprod) and np.isfinite(got).all() and np.allclose(got, exp, rtol=1e-12, atol=1e-12)
    xi = rng.integers(0, 100, (nwindows, npair, nfine, 4)).astype(np.float32)
    wi = rng.integers(0, 4, nfine)
    assert np.array_equal(dedisperse(xi, s, wi, nprod, np.int64), dedisperse_naive(xi, s, wi, nprod).astype(np.int64))
    far = np.zeros((ndm, nfine), np.int64)
    far[:, 0] = 20                                                          # (only channel 0 arrives within 9 windows)
    assert np.array_equal(dedisperse(xi, far, None, nprod, np.int64), dedisperse_naive(xi, far, None, nprod).astype(np.int64))


def test_restatement_recovers_an_injected_pulse():
    """A pulse of amplitude amp in XX at window t0 + s[d0][q] of every channel, on a background of 1 in XX and YY: output
    t0 + S of trial d0 holds nfine * (amp + 2), and no other output comes near."""
    nchan, N, W, nwindows, t0, d0, amp = 4, 8, 4, 40, 6, 2, 1000
    nfine = nchan * N
    s, _ = header_table(power_header(nchan, 1, N, W), nfine)
    S = int(s.max())
    x = np.zeros((nwindows, 1, nfine, 4), np.float32)
    x[..., :2] = 1
    x[t0 + s[d0], 0, np.arange(nfine), 0] += amp
    y = dedisperse(x, s, None, 1, np.int64)[:, 0, :, 0]
    assert np.unravel_index(y.argmax(), y.shape) == (t0 + S, d0) and y[t0 + S, d0] == nfine * (amp + 2)
    y[t0 + S, d0] = 0
    assert y.max() < nfine * (amp + 2) // 2


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("case", sorted(dedisp_cases.CASES))
def test_ordered_float32_restatement_is_exact_on_integers_and_within_the_bound_on_floats(case, nprod):
    """dedisperse_ordered32 (the contract's order in float32 steps): on integer data and weights below 2^24 it is the int64
    restatement word for word; on the float case, NaN in the zero-weight channels, it is finite and within the a-priori bound
    (nfine + 2) * 2^-24 * sum |w x| of the float64 restatement, which any order of an fp32 sum keeps."""
    x, s, w = dedisp_cases.float_case(case, nprod)
    rng = np.random.default_rng(5)
    xi = rng.integers(-5 if nprod == 4 else 0, 10, x.shape).astype(np.float32)
    wi = rng.integers(0, 4, w.size).astype(np.float32)
    exact = dedisperse(xi, s, wi, nprod, np.int64)
    got = dedisperse_ordered32(xi, s, wi, nprod)
    assert got.dtype == np.float32 and np.abs(exact).max() < 2 ** 24 and np.array_equal(got.astype(np.int64), exact)
    got = dedisperse_ordered32(x, s, w, nprod)
    assert np.isfinite(got).all()
    bound = (x.shape[2] + 2) * 2.0 ** -24 * dedisperse(x, s, w, nprod, absolute=True)
    assert (np.abs(got.astype(np.float64) - dedisperse(x, s, w, nprod)) <= bound).all()


@pytest.mark.parametrize("nprod", [1, 4])
def test_float_data_tell_the_contracts_order_from_one_ascending_chain(nprod):
    """On float case (a) one chain over all 70 channels gives other words than four segments added pairwise in more than half
    of the outputs: a test that holds this case bit for bit pins the order."""
    x, s, w = dedisp_cases.float_case("a", nprod)
    a, b = dedisperse_ordered32(x, s, w, nprod), dedisperse_one_chain32(x, s, w, nprod)
    assert np.mean(a.view(np.uint32) != b.view(np.uint32)) > 0.5
    bound = (x.shape[2] + 2) * 2.0 ** -24 * dedisperse(x, s, w, nprod, absolute=True)
    assert (np.abs(b.astype(np.float64) - dedisperse(x, s, w, nprod)) <= bound).all()         # (the a-priori bound passes either order)


# ---------------------------------------------------------------- the block on CPU rings
@pytest.mark.parametrize("stokes", ['I', 'full'])
def test_block_spans_within_and_across_sequences(stokes):
    """Source -> BeamDedisperse -> Sink on in-repo rings, two sequences of 3 spans of 4 windows.  The history crosses the spans
    of a sequence and not the sequences; every span equals the restatement with the table built from the header; the output
    header adds ndm, dms, dedisp_latency, nprod, tsamp."""
    nchan, npair, N, W, nwin, nspan = 2, 3, 8, 4, 4, 3
    nfine, nprod = nchan * N, {'I': 1, 'full': 4}[stokes]
    rng = np.random.default_rng(5 + nprod)
    xs = [_powers(rng, nspan * nwin, npair, nfine) for _ in range(2)]
    hdrs = [power_header(nchan, npair, N, W, seq0=1000 * (s + 1)) for s in range(2)]
    table, tsamp = header_table(hdrs[0], nfine)
    S = int(table.max())
    assert nwin < S < nspan * nwin
    r0, r1 = Ring("ub-output"), Ring("dd-output")
    be = DedispBackend()
    dd = BeamDedisperse(LOG, r0, r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, dms=DMS, max_delay=S + 3, stokes=stokes, backend=be)
    shape = (nwin, npair, len(DMS), nprod)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([dd], Source(r0, [(hdrs[s], xs[s], nwin * npair * nfine * 16) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hdrs[s]['seq0'] and hd['seq0'] == hdrs[s]['seq0'] and len(spans) == nspan
        exp = dedisperse(xs[s], table, None, nprod)
        for k, o in enumerate(spans):
            assert np.array_equal(o.view(np.float32).reshape(shape), exp[k * nwin:(k + 1) * nwin].astype(np.float32))
    hd = sink.sequences[0][0]
    assert hd['ndm'] == len(DMS) and hd['dms'] == DMS and hd['dedisp_latency'] == S and hd['nprod'] == nprod and hd['tsamp'] == tsamp
    assert hd['nupchan'] == N and hd['nframe_sum'] == W and hd['npol'] == 2 and hd['fine_sfreq'] == hdrs[0]['fine_sfreq']
    assert be.calls == [('init', S + 3)] + (['set_delays'] + ['run'] * nspan) * 2
    assert dd.stats['nwindow'] == 2 * nspan * nwin and dd.stats['dedisp_latency'] == S


def test_block_sizes_the_history_from_the_table_and_takes_upchan_beamforms_header():
    """max_delay = None: the context is made at the sequence with the table's own S.  The header of UpchanBeamform's dual-pol
    output has no acc_len: nframe_sum * nupchan stands in.  Initial weights go to the context before the first span."""
    nchan, npair, N, W, nwin = 2, 1, 8, 4, 2
    nfine = nchan * N
    rng = np.random.default_rng(9)
    x = _powers(rng, 4 * nwin, npair, nfine)
    hdr = power_header(nchan, npair, N, W)
    del hdr['acc_len'], hdr['pair0']
    table, _ = header_table(power_header(nchan, npair, N, W), nfine)
    w = rng.integers(0, 3, nfine).astype(np.float64)
    r0, r1 = Ring("ub-output"), Ring("dd-output")
    be = DedispBackend()
    dd = BeamDedisperse(LOG, r0, r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, dms=DMS, weights=w, backend=be)
    assert be.dd is None
    shape = (nwin, npair, len(DMS), 1)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    run_blocks([dd], Source(r0, [(hdr, x, nwin * npair * nfine * 16)]), [sink])
    (hd, _, spans), = sink.sequences
    exp = dedisperse(x, table, w, 1)
    assert np.array_equal(np.concatenate([o.view(np.float32).reshape(shape) for o in spans]), exp.astype(np.float32))
    assert be.calls[:3] == [('init', int(table.max())), 'set_weights', 'set_delays'] and be.calls[3:] == ['run'] * 4


def test_block_gap_resets_and_restarts_the_output_sequence():
    """Spans 0, 1, 3, 4 of a sequence (2 never read): the context is reset, the output restarts in a sequence of its own at span
    3's sample, and spans 3, 4 are the restatement of a history that begins at span 3."""
    nchan, npair, N, W, nwin, seq0 = 2, 2, 8, 4, 4, 700
    nfine = nchan * N
    rng = np.random.default_rng(11)
    x = _powers(rng, 5 * nwin, npair, nfine)
    hdr = power_header(nchan, npair, N, W, seq0=seq0)
    table, _ = header_table(hdr, nfine)
    seen = [(k, np.ascontiguousarray(x[k * nwin:(k + 1) * nwin])) for k in (0, 1, 3, 4)]
    be = DedispBackend()
    r1 = Ring("dd-output")
    dd = BeamDedisperse(LOG, _FakeRing([_FakeSeq(hdr, seen, nwin * npair * nfine * 16)]), r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, dms=DMS,
                        max_delay=int(table.max()), backend=be)
    shape = (nwin, npair, len(DMS), 1)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    sink.start()
    dd.main()
    sink.join(20)
    assert be.calls == [('init', int(table.max())), 'set_delays', 'run', 'run', 'reset', 'run', 'run']
    (h0, t0, a), (h1, t1, b) = sink.sequences
    step = nwin * W * N
    assert (h0['seq0'], t0, h1['seq0'], t1) == (seq0, seq0, seq0 + 3 * step, seq0 + 3 * step) and len(a) == len(b) == 2
    for spans, first in ((a, 0), (b, 3)):
        exp = dedisperse(x[first * nwin:], table, None, 1).astype(np.float32)
        for k, o in enumerate(spans):
            assert np.array_equal(o.view(np.float32).reshape(shape), exp[k * nwin:(k + 1) * nwin])
    assert dd.stats['ngap'] == 1


def test_block_weights_command_lands_at_the_next_span():
    """A `weights` command that arrives after span 1 was enqueued: spans 0 and 1 carry the old weights (all ones), span 2 on
    the new ones -- applied to the windows of spans 0 and 1 still in the history too.  A command of the wrong length or with a
    NaN is refused and changes nothing."""
    nchan, npair, N, W, nwin = 2, 1, 8, 4, 4
    nfine = nchan * N
    rng = np.random.default_rng(13)
    x = _powers(rng, 4 * nwin, npair, nfine)
    hdr = power_header(nchan, npair, N, W)
    table, _ = header_table(hdr, nfine)
    w = rng.integers(0, 3, nfine).astype(float).tolist()
    be = DedispBackend()
    r1 = Ring("dd-output")
    box = {}

    def spans():
        for k in range(4):
            if k == 2:
                box['dd'].process_command_strings(_cmd(w))
                assert box['dd'].last_response['val']['status'] == 'normal'
            if k == 3:
                for bad in (w[:-1], w[:-1] + [float('nan')], "ones"):
                    box['dd'].process_command_strings(_cmd(bad, "2"))
                    assert box['dd'].last_response['val']['status'] == 'error'
            yield k, np.ascontiguousarray(x[k * nwin:(k + 1) * nwin])

    seq = _FakeSeq(hdr, spans(), nwin * npair * nfine * 16)
    dd = box['dd'] = BeamDedisperse(LOG, _FakeRing([seq]), r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, dms=DMS, max_delay=20, backend=be)
    shape = (nwin, npair, len(DMS), 1)
    sink = Sink(r1, int(np.prod(shape)) * 4)
    sink.start()
    dd.main()
    sink.join(20)
    assert be.calls == [('init', 20), 'set_delays', 'run', 'run', 'set_weights', 'run', 'run']
    (_, _, out), = sink.sequences
    got = np.concatenate([o.view(np.float32).reshape(shape) for o in out])
    old, new = dedisperse(x, table, None, 1), dedisperse(x, table, w, 1)
    assert np.array_equal(got[:2 * nwin], old[:2 * nwin].astype(np.float32)) and np.array_equal(got[2 * nwin:], new[2 * nwin:].astype(np.float32))
    assert not np.array_equal(old[2 * nwin:], new[2 * nwin:])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(stokes='Q'), dict(nwin=0), dict(npair=0), dict(nupchan=-8), dict(dms=[]), dict(dms=[-1.0]), dict(dms=[float('nan')]),
                                dict(max_delay=-1), dict(weights=np.ones(15)), dict(weights=[float('inf')] * 16)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(npair=1, nchan=2, nupchan=8, nwin=4, dms=DMS, max_delay=8)
    args.update(kw)
    be = DedispBackend()
    with pytest.raises(ValueError, match="BEAM_DEDISPERSE"):
        BeamDedisperse(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.dd is None                    # (refused before the context is made)


@pytest.mark.parametrize("bad", [dict(npol=1), dict(nbit=8), dict(nbeam=2), dict(nchan=4), dict(nupchan=16), dict(nupchan=None), dict(nframe_sum=None),
                                 dict(fine_sfreq=None), dict(fine_bw_hz=0), dict(acc_len=33), dict(ndm=4), dict(max_delay=1)])
def test_block_refuses_what_is_not_fine_channel_power_beams(bad):
    """Voltage beams, other sizes, products that were not channelised or summed over windows, a span that has been dedispersed,
    a table that needs more history than max_delay gives: ValueError before any run."""
    nchan, npair, N, W, nwin = 2, 1, 8, 4, 4
    bad = dict(bad)
    max_delay = bad.pop('max_delay', 20)
    be = DedispBackend()
    hdr = power_header(nchan, npair, N, W)
    hdr.update(bad)
    x = np.zeros((nwin, npair, nchan * N, 4), np.float32)
    dd = BeamDedisperse(LOG, _FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), npair=npair, nchan=nchan, nupchan=N, nwin=nwin, dms=DMS,
                        max_delay=max_delay, backend=be)
    with pytest.raises(ValueError, match="BEAM_DEDISPERSE"):
        dd.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengDedispInitialize", "xengDedispSetDelays", "xengDedispSetWeights", "xengDedispRun", "xengDedispReset", "xengDedispGetInfo",
         "xengDedispMark", "xengDedispWait", "xengDedispTicketDone", "xengDedispSync", "xengDedispDestroy", "xengDedispCheckGuards")


def test_backend_forwards_every_call_the_block_makes():
    """HipBackend has a method for each dedisp_* call of the block (and the fake backend above has the same ones)."""
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("dedisp_initialize", "dedisp_set_delays", "dedisp_set_weights", "dedisp_run", "dedisp_reset", "dedisp_info", "dedisp_mark",
              "dedisp_wait", "dedisp_sync", "dedisp_guards_intact"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("dedisp_initialize", "dedisp_set_delays", "dedisp_set_weights", "dedisp_run", "dedisp_reset", "dedisp_mark", "dedisp_wait", "dedisp_sync"):
        assert callable(getattr(DedispBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait (the setters
    among them) are not.  Initialize refuses bad sizes, nprod, max_delay and an oversized history before it touches a device;
    Run refuses null and misaligned pointers, SetDelays a null table, GetInfo / Mark / TicketDone null results, before looking
    for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengDedispRun", "xengDedispReset", "xengDedispMark", "xengDedispTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengDedispInitialize", "xengDedispSetDelays", "xengDedispSetWeights", "xengDedispWait", "xengDedispSync", "xengDedispCheckGuards"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, npair, nfine, nwin, ndm, max_delay, nprod); the last: 16 x 3072 x 4 words x 2^20 windows = 824 GB of history
    for args in ((0, 0, 3072, 30, 256, 107, 1), (0, 16, 0, 30, 256, 107, 1), (0, 16, 3072, 0, 256, 107, 1), (0, 16, 3072, 30, 0, 107, 1),
                 (0, 16, 3072, 30, 256, -1, 1), (0, 16, 3072, 30, 256, 107, 2), (0, 16, 3072, 30, 256, 107, 0), (0, 16, 3072, 30, 256, 1 << 20, 4),
                 (0, 70000, 8, 1, 1, 0, 1)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengDedispInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    for name, args in (("xengDedispRun", (None, 1, 4096)), ("xengDedispRun", (4096, 1, None)), ("xengDedispRun", (4100, 1, 4096)),
                       ("xengDedispRun", (4096, 1, 4104)), ("xengDedispSetDelays", (None,)), ("xengDedispGetInfo", (None, None)),
                       ("xengDedispMark", (None,)), ("xengDedispTicketDone", (1, None)), ("xengDedispCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_dedisp_gpu.py covers the rest)
    s, n, t = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_ulonglong()
    table = np.zeros(8, np.int32)
    for name, args in (("xengDedispRun", (4096, 1, 4096)), ("xengDedispSetDelays", (table.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),)),
                       ("xengDedispSetWeights", (None,)), ("xengDedispReset", ()), ("xengDedispGetInfo", (ctypes.byref(s), ctypes.byref(n))),
                       ("xengDedispMark", (ctypes.byref(t),)), ("xengDedispWait", (1,)), ("xengDedispTicketDone", (1, ctypes.byref(s))),
                       ("xengDedispSync", ()), ("xengDedispCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengDedispDestroy")       # (nothing to destroy: success)
