"""UpchanFlag without a GPU: the host functions of blocks/flagging.py; the restatement's own properties (tests/flag_ref.py: the
median's definition, a MAD of 0, fewer than 4 live stands, the channel window's edges, detection of the injections); and the block
on CPU rings (both implementations) with a backend, defined here, that serves flag_* from the float32 restatement -- one span per
span, the header keys, the commands, a gap, set_weights and set_control at the next integration, flags()."""
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ring
from caltech_bifrost_dsp_amd.blocks import UpchanFlag, flag_factors, flag_summary, flag_visibilities, stand_weights
from caltech_bifrost_dsp_amd.ring import Ring
from tests import flag_ref as fr
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks
from tests.test_calapply_cpu import ACC_LEN, vis_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


# ---------------------------------------------------------------- the restatement
def test_median_definition():
    """v[n / 2] for odd n, 0.5f * (v[(n-1) / 2] + v[n / 2]) for even n, one float32 add and one exact halving"""
    assert fr.median([3, 1, 2]) == 2 and fr.median([4, 1, 3, 2]) == np.float32(2.5) and fr.median([7]) == 7
    a, b = np.float32(1), np.float32(1 + 2.0 ** -23)
    assert fr.median([a, b]) == np.float32(0.5) * (a + b) and fr.median([a, b]).dtype == np.float32
    assert fr.median([5, 5, 1, 9]) == 5


def test_a_mad_of_zero_flags_every_stand_that_differs():
    """More than half of the stands share one value: mad = 0, the threshold is 0 and every d > 0 flags, for any k > 0; k = 0 flags
    none."""
    x = np.array([2, 2, 2, 2, 2, 3, 2, 1.5], np.float32)
    med, mad, d, out = fr.outliers(x, fr.thresholds(6)[0])
    assert med == 2 and mad == 0 and list(np.flatnonzero(out)) == [5, 7]
    assert not fr.outliers(x, 0)[3].any()
    stats = np.zeros((1, 2, 8, 2), np.float32)
    stats[0, :, :, 0] = x
    stats[0, :, :, 1] = 1
    mask, chan = fr.flags(stats, np.ones(8), *fr.thresholds(), 0)
    assert list(np.flatnonzero(mask[0, 0] & 1)) == [5, 7] and not (mask & 2).any() and chan[0, 0, 1] == 0


def test_fewer_than_four_live_stands():
    """3 live stands in (channel 1, pol 0): no stand test (an obvious outlier is not flagged), bit 2 on every stand, the weight-0
    ones included, med_R = mad_R = b = +0, and the channel test of pol 0 leaves channel 1 out."""
    stats = np.ones((3, 2, 6, 2), np.float32)
    stats[:, :, :, 0] += np.arange(6, dtype=np.float32) * 0.01
    stats[1, 0, 0, 0] = np.nan
    stats[1, 0, 1, 1] = np.inf
    stats[1, 0, 2, 0] = 1e6
    w = np.array([1, 1, 1, 1, 1, 0], np.float32)
    mask, chan = fr.flags(stats, w, *fr.thresholds(), 0)
    assert chan[1, 0, 3] == 3 and (chan[1, 0, :3].view(np.uint32) == 0).all()
    assert list(mask[1, 0]) == [12, 12, 4, 4, 4, 20]
    assert (mask[[0, 2], 0] == [0, 0, 0, 0, 0, 16]).all() and (mask[:, 1] == [0, 0, 0, 0, 0, 16]).all()
    assert chan[0, 0, 2] == chan[2, 0, 2] == fr.median([chan[0, 0, 0], chan[2, 0, 0]])


def test_channel_window_edges():
    """y = 1 .. 9 over 9 channels with channel 4 at 100: with wchan = 1 the baseline of channel 0 is the median of {y0, y1}, that of
    channel 8 the median of {y7, y8}, that of channel 4 the median of {y3, 100, y5}; with wchan = 0 one median for all."""
    stats = np.ones((9, 2, 5, 2), np.float32)
    y = np.arange(1, 10, dtype=np.float32)
    y[4] = 100
    stats[:, :, :, 0] = y[:, None, None]
    _, chan = fr.flags(stats, np.ones(5), *fr.thresholds(), 1)
    assert (chan[:, 0, 0] == y).all()
    assert list(chan[:, 0, 2]) == [1.5, 2, 3, 4, 6, 7, 7, 8, 8.5]
    mask, chan = fr.flags(stats, np.ones(5), *fr.thresholds(), 0)
    assert (chan[:, :, 2] == 6).all() and (mask[4] == 4).all() and not mask[[0, 1, 2, 3, 5, 6, 7, 8]].any()
    mask, _ = fr.flags(stats, np.ones(5), *fr.thresholds(6, 6, 0), 0)
    assert not mask.any()


def test_statistics_orders_agree_and_leave_out_what_they_must():
    """The kernel-order float32 sum, the term-by-term float32 sum and the float64 sum agree to rounding; a stand of weight 0, the
    upper triangle and the cross hands are not looked at; a NaN word reaches its two stands' R in its (channel, pol) only."""
    V = fr.case(35, 2)
    w = np.ones(35, np.float32)
    w[3] = 0
    ref = fr.statistics(V, w)
    bad = fr.upper_and_cross_nan(V)
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.nan
    for R, A in (fr.statistics_kernel_order(bad, w), fr.statistics(bad, w, np.float32)):
        assert fr.stat_error(R, ref[0], w).max() < 1e-6 and np.array_equal(A, ref[1].astype(np.float32)) and (R[:, :, 3] == 0).all()
    nan = bad.copy()
    nan[1, 20, 1, 9, 1] = np.nan
    R, A = fr.statistics_kernel_order(nan, w)
    R0, _ = fr.statistics_kernel_order(bad, w)
    hit = np.zeros(R.shape, bool)
    hit[1, 1, [9, 20]] = True
    assert np.isnan(R[hit]).all() and np.array_equal(R[~hit], R0[~hit])


def test_injections_are_detected_by_the_restatement():
    """tests/test_flag_gpu.py's detection case on the restatement: see there."""
    V, w, expect = detection_case()
    stats = np.stack(fr.statistics_kernel_order(V, w), axis=-1)
    detail = []
    mask, _ = fr.flags(stats, w, *fr.thresholds(), 0, detail)
    assert fr.margin(detail) >= 0.01
    assert np.array_equal(mask, expect)


def detection_case(nstand=70, nfine=12):
    """(V, w, the mask expected): stand 7 eight times too loud in channel 2; stand 11's autos times 0.01; every stand five times too
    loud in channel 5; a NaN word between stands 20 and 9 in (channel 8, pol 1); stand 3 of weight 0 and full of NaN.

    The mask is written down from the injections.  Stand 7's R in channel 2 is 64 times the others' and its A 4096 times: bits 0 and
    1 there.  Its 64-fold cross-power is also one of the 68 terms of every other stand's R in that channel, which all rise by the
    same factor 1 + 63 / 68 -- no stand moves against the others, but the channel's median R nearly doubles against a spread over the
    channels of a few per cent: bit 2 on channel 2.  Stand 11: bit 1 in every (channel, pol).  Channel 5: R times 625 and A times 25
    at every stand alike: bit 2 only.  The NaN word: bit 3 at stands 20 and 9 of (8, 1).  Stand 3: bit 4 everywhere."""
    V = fr.case(nstand, nfine)
    fr.scale_stand(V, 2, 7, 8)
    fr.scale_auto(V, 11, 0.01)
    fr.scale_channel(V, 5, 5)
    V[8, 20, 1, 9, 1] = np.nan
    V[:, 3] = np.nan
    V[:, :, :, 3] = np.nan
    w = np.ones(nstand, np.float32)
    w[3] = 0
    expect = np.zeros((nfine, 2, nstand), np.uint8)
    expect[2, :, 7] |= 3
    expect[2] |= 4
    expect[:, :, 11] |= 2
    expect[5] |= 4
    expect[8, 1, [20, 9]] |= 8
    expect[:, :, 3] = 16
    expect[[2, 5], :, 3] |= 4
    return V, w, expect


# ---------------------------------------------------------------- the host functions
def _mask():
    m = np.zeros((3, 2, 5), np.uint8)
    m[0, 0, 1] = 1
    m[1, 1, 1] = 2
    m[2, 0, 1] = 8
    m[2, 1, 1] = 1
    m[1, :, :] |= 4
    m[:, :, 4] |= 16
    m[0, 1, 2] = 2
    return m


def test_flag_factors():
    m = _mask()
    h = (np.arange(30).reshape(3, 2, 5) + 1j).astype(np.complex64)
    f = flag_factors(h, m)
    assert f.dtype == np.complex64 and f.flags['C_CONTIGUOUS']
    assert np.array_equal(f == 0, (m & 0x0f) != 0) and np.array_equal(f[f != 0], h[(m & 0x0f) == 0])
    assert (flag_factors(h, m)[:, :, 4][[0, 2]] != 0).all()                  # bit 4 alone does not zero a factor
    assert np.array_equal(flag_factors(h, m, bits=0x10) == 0, (m & 0x10) != 0)
    assert np.array_equal(flag_factors(h, m, bits=0), h)
    for bad in (dict(h=h[:2]), dict(mask=m.astype(np.int32)), dict(mask=m[0]), dict(bits=256), dict(bits=1.5)):
        args = dict(h=h, mask=m)
        args.update(bad)
        with pytest.raises(ValueError):
            flag_factors(**args)


def test_stand_weights():
    m = _mask()
    w = np.array([1, 2, 0.5, 1, 3], np.float32)
    # stand 1: 4 of 6 cells with one of the bits 0, 1, 3; stand 2: 1 of 6; the channel bit and the weight bit do not count
    assert list(stand_weights(m, w)) == [1, 0, 0.5, 1, 3]
    assert list(stand_weights(m, w, max_fraction=0.7)) == [1, 2, 0.5, 1, 3]
    assert list(stand_weights(m, w, max_fraction=0.1)) == [1, 0, 0, 1, 3]
    assert list(stand_weights(m, w, max_fraction=0.1, bits=0x1f)) == [0, 0, 0, 0, 0]
    assert list(stand_weights(m, w, max_fraction=4 / 6)) == [1, 2, 0.5, 1, 3]   # "more than": 4 of 6 is not more than 4 / 6 of them
    assert stand_weights(m, w).dtype == np.float32
    for bad in (dict(w=w[:4]), dict(max_fraction=1.5), dict(max_fraction=-0.1), dict(mask=m[:, :1])):
        args = dict(mask=m, w=w)
        args.update(bad)
        with pytest.raises(ValueError):
            stand_weights(**args)


def test_flag_visibilities_and_summary():
    m = _mask()
    V = (np.arange(3 * 10 * 10).reshape(3, 5, 2, 5, 2) + 1).astype(np.complex64)
    Z = flag_visibilities(V, m)
    bad = ((m & 0x0f) != 0).transpose(0, 2, 1).reshape(3, 10)
    gone = bad[:, :, None] | bad[:, None, :]
    assert np.array_equal(Z.reshape(3, 10, 10) == 0, gone) and np.array_equal(Z.reshape(3, 10, 10)[~gone], V.reshape(3, 10, 10)[~gone])
    assert V.min() == 1                                                      # (a copy)
    with pytest.raises(ValueError):
        flag_visibilities(V[:2], m)
    s = flag_summary(m)
    assert s['ncell'] == 30 and s['bits'] == {'cross': 2, 'auto': 2, 'chan': 10, 'nonfinite': 1, 'weight': 6}
    assert s['nflagged'] == int((m != 0).sum()) and s['fraction'] == s['nflagged'] / 30
    assert list(s['per_channel']) == [2, 10, 2] and list(s['per_stand']) == [2, 5, 3, 2, 2]


# ---------------------------------------------------------------- the block on CPU rings
NSTAND, NFINE = 6, 3
SPAN = NFINE * (2 * NSTAND) ** 2 * 8
MASK_BYTES = NFINE * 2 * NSTAND
STATS_OFFSET = (MASK_BYTES + 15) & ~15
CHAN_OFFSET = STATS_OFFSET + MASK_BYTES * 8
OSPAN = CHAN_OFFSET + NFINE * 2 * 16


class FlagBackend(OracleBackend):
    """The oracle backend plus xengFlag* served by the float32 restatement in the kernel's order, with the context's state."""

    def __init__(self):
        super().__init__()
        self.fl, self.calls = None, []
        self.w, self.control = None, (6.0, 6.0, 6.0, 0)

    def flag_initialize(self, gpu, nstand, nfine):
        if nstand < 4 or nstand > 512 or nfine > 8192:
            return 1
        self.fl = dict(nstand=nstand, nfine=nfine)
        self.w, self.control = np.ones(nstand, np.float32), (6.0, 6.0, 6.0, 0)
        self.calls.append('init')
        return 0

    def flag_set_weights(self, w):
        assert w.dtype == np.float32 and w.shape == (self.fl['nstand'],)
        if (w > 0).sum() < 4:
            return 1
        self.w = np.array(w)
        self.calls.append('weights')
        return 0

    def flag_set_control(self, nsig_cross, nsig_auto, nsig_chan, wchan):
        self.control = (nsig_cross, nsig_auto, nsig_chan, wchan)
        self.calls.append('control')
        return 0

    def flag_run(self, vis_arr, out_arr, stats_offset, chan_offset):
        u = self.fl
        V = vis_arr.numpy().reshape(-1).view(np.uint8).view(np.complex64).reshape(u['nfine'], u['nstand'], 2, u['nstand'], 2)
        mask, stats, chan = expect(V, self.w, self.control)
        out = out_arr.numpy().reshape(-1).view(np.uint8)
        out[:mask.size] = mask.reshape(-1)
        out[stats_offset:stats_offset + stats.nbytes] = stats.reshape(-1).view(np.uint8)
        out[chan_offset:chan_offset + chan.nbytes] = chan.reshape(-1).view(np.uint8)
        self.calls.append('run')
        return 0

    def flag_mark(self):
        return self.beam_mark()

    def flag_wait(self, ticket):
        self.beam_wait(ticket)

    def flag_sync(self):
        pass


def expect(V, w, control=(6.0, 6.0, 6.0, 0)):
    stats = np.ascontiguousarray(np.stack(fr.statistics_kernel_order(V, w), axis=-1))
    mask, chan = fr.flags(stats, w, *fr.thresholds(*control[:3]), control[3])
    return mask, stats, chan


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _data(rng, n):
    V = np.stack([fr.case(NSTAND, NFINE, seed=int(rng.integers(1 << 30)), ntime=64) for _ in range(n)])
    for k in range(n):
        fr.scale_stand(V[k], k % NFINE, k % NSTAND, 8)
    return V


def _parts(span):
    raw = np.asarray(span).view(np.uint8).reshape(-1)
    return (raw[:MASK_BYTES].reshape(NFINE, 2, NSTAND), raw[STATS_OFFSET:CHAN_OFFSET].view(np.float32).reshape(NFINE, 2, NSTAND, 2),
            raw[CHAN_OFFSET:OSPAN].view(np.float32).reshape(NFINE, 2, 4))


def _check(span, V, w, control=(6.0, 6.0, 6.0, 0)):
    for got, exp in zip(_parts(span), expect(V, w, control)):
        assert got.tobytes() == exp.tobytes()


def test_block_one_span_per_span_header_and_flags(ring_impl):
    """Source -> UpchanFlag -> Sink, two sequences of three integrations, the second calibrated: every output span is the
    restatement of its input span -- mask padded to 16 bytes, stats, chan at the header's offsets; the header is the input's plus
    flagged, the controls and the offsets; flags() is the last integration's; a flagged header is not accepted as input."""
    rng = np.random.default_rng(13)
    hdrs = [vis_header(nstand=NSTAND, nfine=NFINE, seq0=1000, fine_sfreq=50e6), vis_header(nstand=NSTAND, nfine=NFINE, seq0=5000, fine_sfreq=62e6, calibrated=True)]
    Vs = [_data(rng, 3) for _ in range(2)]
    r0, r1 = Ring("corr-output"), Ring("flag-output")
    be = FlagBackend()
    fl = UpchanFlag(LOG, r0, r1, NSTAND, backend=be)
    assert fl.flags() is None and MASK_BYTES % 16 != 0
    sink = Sink(r1, OSPAN)
    run_blocks([fl], Source(r0, [(hdrs[s], Vs[s].reshape(-1).view(np.uint8), SPAN) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    ones = np.ones(NSTAND, np.float32)
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert len(spans) == 3
        for k in range(3):
            _check(spans[k], Vs[s][k], ones)
        assert tag == hd['seq0'] == hdrs[s]['seq0']
        assert hd['flagged'] is True and (hd['nsig_cross'], hd['nsig_auto'], hd['nsig_chan'], hd['wchan']) == (6.0, 6.0, 6.0, 0)
        assert (hd['stats_offset'], hd['chan_offset']) == (STATS_OFFSET, CHAN_OFFSET) and hd.get('calibrated') == (None, True)[s]
        assert all(hd[k] == hdrs[s][k] for k in ('nfine', 'fine_sfreq', 'fine_bw_hz', 'nstand', 'npol', 'acc_len', 'nupchan'))
        with pytest.raises(ValueError, match="UPCHAN_FLAG"):
            UpchanFlag(LOG, Ring("a"), Ring("b"), NSTAND, backend=be)._check_header(hd)
    seq, mask, stats, chan = fl.flags()
    em, es, ec = expect(Vs[1][2], ones)
    assert seq == 5000 + 2 * ACC_LEN and mask.tobytes() == em.tobytes() and stats.tobytes() == es.tobytes() and chan.tobytes() == ec.tobytes()
    assert mask.dtype == np.uint8 and stats.shape == (NFINE, 2, NSTAND, 2) and chan.shape == (NFINE, 2, 4)
    assert be.calls == ['init', 'weights', 'control'] + ['run'] * 6
    assert fl.stats['nflag'] == 6 and fl.stats['ngap'] == 0 and fl.stats['flagged_fraction'] == float((em != 0).mean())


def test_block_controls_at_the_next_integration_and_a_gap_opens_a_new_sequence(ring_impl):
    """Integrations 0..6 of a sequence, 3 never read.  set_weights before 1 (stand 4 out).  set_control before 2: a sequence of its
    own whose header names the new controls.  The gap ends that sequence; 4 opens one whose header starts there.  A `control` command
    before 5, a `weights` command before 6.  What is not a control or weights that leave 4 stands is refused and changes nothing."""
    rng = np.random.default_rng(17)
    hdr = vis_header(nstand=NSTAND, nfine=NFINE, seq0=960)
    V = _data(rng, 7)
    w1 = np.array([1, 2, 0.5, 1, 0, 1], np.float32)
    w2 = [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    c1, c2 = (3.0, 0.0, 2.0, 1), (4.0, 4.0, 0.0, 0)
    box = {}

    def spans():
        for k in (0, 1, 2, 4, 5, 6):
            fl = box['fl']
            if k == 1:
                fl.set_weights(w1)
                for bad in ([1.0] * 5, [1, 1, 1, 1, 1, -1], [1, 1, 1, 1, 1, np.nan], [1, 1, 1, 0, 0, 0]):
                    with pytest.raises(ValueError, match="UPCHAN_FLAG"):
                        fl.set_weights(bad)
                for bad in ((-1, 6, 6, 0), (6, np.inf, 6, 0), (6, 6, 6, 65), (6, 6, 6, 1.5), (6, 6, 6, -1), (6, 6, "x", 0)):
                    with pytest.raises(ValueError, match="UPCHAN_FLAG"):
                        fl.set_control(*bad)
            if k == 2:
                fl.set_control(*c1)
            if k == 5:
                fl.process_command_strings(_cmd(control=list(c2)))
                assert fl.last_response['val']['status'] == 'normal'
                for n, bad in enumerate(({'control': [6.0, 6.0, 6.0]}, {'control': [6.0, -1.0, 6.0, 0]}, {'weights': [1.0] * 5}, {'weights': [1.0, 1.0, 1.0, 0, 0, 0]})):
                    fl.process_command_strings(_cmd(str(2 + n), **bad))
                    assert fl.last_response['val']['status'] == 'error', bad
            if k == 6:
                fl.process_command_strings(_cmd("9", weights=w2))
                assert fl.last_response['val']['status'] == 'normal'
            yield k, V[k]

    be = FlagBackend()
    r1 = Ring("flag-output")
    fl = box['fl'] = UpchanFlag(LOG, _FakeRing([_FakeSeq(hdr, spans(), SPAN)]), r1, NSTAND, backend=be)
    sink = Sink(r1, OSPAN)
    sink.start()
    fl.main()
    sink.join(20)
    seqs = sink.sequences
    assert [(h['seq0'], t, len(s)) for h, t, s in seqs] == [(960, 960, 2), (960 + 2 * ACC_LEN, 960 + 2 * ACC_LEN, 1), (960 + 4 * ACC_LEN, 960 + 4 * ACC_LEN, 1),
                                                            (960 + 5 * ACC_LEN, 960 + 5 * ACC_LEN, 2)]
    d = (6.0, 6.0, 6.0, 0)
    assert [(h['nsig_cross'], h['nsig_auto'], h['nsig_chan'], h['wchan']) for h, _, _ in seqs] == [d, c1, c1, c2]
    ones = np.ones(NSTAND, np.float32)
    chain = [(V[0], ones, d), (V[1], w1, d), (V[2], w1, c1), (V[4], w1, c1), (V[5], w1, c2), (V[6], np.array(w2, np.float32), c2)]
    for k, sp in enumerate([sp for _, _, s in seqs for sp in s]):
        _check(sp, *chain[k])
    assert be.calls == ['init', 'weights', 'control', 'run', 'weights', 'run', 'control', 'run', 'run', 'control', 'run', 'weights', 'run']
    assert fl.stats['ngap'] == 1 and fl.stats['nflag'] == 6
    seq, mask, _, _ = fl.flags()
    assert seq == 960 + 6 * ACC_LEN and (mask[:, :, 2] & 16 == 16).all() and mask.tobytes() == expect(V[6], np.array(w2, np.float32), c2)[0].tobytes()


@pytest.mark.parametrize("kw", [dict(nstand=3), dict(nstand=513), dict(nstand=6.0), dict(weights=[1.0] * 5), dict(weights=[1, 1, 1, 1, 1, -1]),
                                dict(weights=[1, 1, 1, 0, 0, 0]), dict(nsig_cross=-1), dict(nsig_auto=np.nan), dict(nsig_chan="6"), dict(wchan=65), dict(wchan=-1),
                                dict(wchan=2.0)])
def test_constructor_refuses_bad_arguments(kw):
    be = FlagBackend()
    args = dict(nstand=NSTAND)
    args.update(kw)
    with pytest.raises(ValueError, match="UPCHAN_FLAG"):
        UpchanFlag(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.fl is None
    UpchanFlag(LOG, Ring("a"), Ring("b"), NSTAND, nsig_cross=0, nsig_auto=0, nsig_chan=0, wchan=64, backend=be)


@pytest.mark.parametrize("bad", [dict(npol=1), dict(nstand=7), dict(nfine=None), dict(nfine=0), dict(nfine=8193), dict(nbit=8), dict(complex=False), dict(npix=7),
                                 dict(nsrc=2), dict(acc_len=0), dict(flagged=True)])
def test_block_refuses_what_is_not_its_visibilities(bad):
    """npol != 2, a stand count that differs from the block's, more channels than the channel test takes, and headers that are not
    UpchanCorr's or UpchanCalApply's: refused at the sequence, before anything is run."""
    be = FlagBackend()
    hdr = vis_header(nstand=NSTAND, nfine=NFINE)
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NFINE, NSTAND, 2, NSTAND, 2), np.complex64)
    fl = UpchanFlag(LOG, _FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), NSTAND, backend=be)
    with pytest.raises(ValueError, match="UPCHAN_FLAG"):
        fl.main()
    assert 'run' not in be.calls
