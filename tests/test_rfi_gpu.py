"""BeamRfiClean on the MI355X: xengRfi* against the restatement (tests/rfi_ref.py), byte for byte and with no tolerance: out and
stats of every call and the tables of every decided block (flags, mu, V, R, gains), at the smallest shapes that can go wrong (fewer
channels than chains, chains of one and two channels, the live channel count; a NaN, a +inf, a constant channel, a masked one, a
dead pair, a window below min_count, a broadband spike); an integer scene with equal R in many channels; bit identity across splits
of a run over calls, after Reset against a fresh context, and beside an X-engine contraction and xengBeamformRun; SetControl and
SetMask holding from the next block; zerodm on and off; the ABI's refusals and tickets; and Source -> Beamform -> UpchanSumBeams ->
BeamRfiClean -> BeamDedisperse on device rings.  Out and stats sit between poisoned guard bands that are checked after every
call, the input is read back after every call and must be what was uploaded, the state's guards are checked at every close.  No
wall-clock assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Beamform, BeamDedisperse, BeamRfiClean, UpchanSumBeams, dm_delays, rfi_controls  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import rfi_cases, rfi_ref  # noqa: E402
from tests.dedisp_ref import dedisperse  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
_pf, _pu8 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)


def _info():
    n, k = ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengRfiGetInfo", ctypes.byref(n), ctypes.byref(k))
    return n.value, k.value


class RF:
    """The xengRfi context (one per process), an input buffer, out and stats between poisoned guard bands, and the restatement
    beside it: every call goes to both and is compared byte for byte, and so are the tables of every block decided."""

    def __init__(self, npair, nfine, nwin, nstat):
        self.npair, self.nfine, self.nwin, self.nstat = npair, nfine, nwin, nstat
        # the buffers come first, the context second: tests/test_accel_gpu.py says why
        self.din = ffi.DeviceBuffer(nwin * npair * nfine * 16)
        self.dout = ffi.DeviceBuffer(2 * GUARD + nwin * npair * nfine * 16)
        self.dst = ffi.DeviceBuffer(2 * GUARD + nwin * npair * 16)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        ffi.call("xengMemset", self.dst.ptr, POISON, self.dst.nbytes)
        ffi.call("xengRfiInitialize", 0, npair, nfine, nwin, nstat)
        self.ref = rfi_ref.RfiRef(npair, nfine, nstat)
        self.sent = None
        self.blocks = []                # the tables' bytes of every block decided

    def control(self, k_chan, t_clip, t_broad, min_count, zerodm):
        ffi.call("xengRfiSetControl", k_chan, t_clip, t_broad, min_count, zerodm)
        self.ref.set_control(k_chan, t_clip, t_broad, min_count, zerodm)

    def mask(self, m):
        m = None if m is None else np.ascontiguousarray(m, np.uint8)
        ffi.call("xengRfiSetMask", None if m is None else m.ctypes.data_as(_pu8))
        self.ref.set_mask(m)

    def reset(self):
        ffi.call("xengRfiReset")
        self.ref.reset()
        assert _info() == (0, 0)

    def enqueue(self, x):
        nc = x.shape[0]
        assert x.shape == (nc, self.npair, self.nfine, 4)
        self.sent = np.ascontiguousarray(x, np.float32)
        self.din.upload(self.sent)
        done = ctypes.c_int(-1)
        ffi.call("xengRfiRun", self.din.ptr, nc, self.dout.ptr + GUARD, self.dst.ptr + GUARD, ctypes.byref(done))
        assert done.value in (0, 1)
        return done.value

    def tables(self):
        flags = np.empty((self.npair, self.nfine), np.uint8)
        mu, var, r = (np.empty((self.npair, self.nfine), np.float32) for _ in range(3))
        g = np.empty((self.npair, self.nfine, 4), np.float32)
        ffi.call("xengRfiGetBlock", flags.ctypes.data_as(_pu8), mu.ctypes.data_as(_pf), var.ctypes.data_as(_pf), r.ctypes.data_as(_pf), g.ctypes.data_as(_pf))
        return flags, mu, var, r, g

    def result(self, nc):
        """After a sync: the input is byte for byte what was uploaded; (out, stats) of the call's nc windows; every byte before and
        after them must still be poison (it is put back behind them)."""
        assert self.din.download(np.uint8, self.sent.nbytes).tobytes() == self.sent.tobytes(), "the input was written"
        res = []
        for buf, per in ((self.dout, self.npair * self.nfine * 16), (self.dst, self.npair * 16)):
            raw = buf.download(np.uint8)
            assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
            assert (raw[GUARD + nc * per:] == POISON).all(), "bytes past the call's windows were written"
            res.append(raw[GUARD:GUARD + nc * per].copy())
            ffi.call("xengMemset", buf.ptr, POISON, buf.nbytes)
        return res[0].view(np.float32).reshape(nc, self.npair, self.nfine, 4), res[1].view(np.int32).reshape(nc, self.npair, 4)

    def check(self, nc, done):
        """Compare the call that has completed with the restatement's; returns (out, stats)."""
        out, st = self.result(nc)
        before = self.ref.nblocks
        eo, es = self.ref.run(self.sent)
        assert bool(done) == (self.ref.nblocks > before)
        if done:
            got = self.tables()
            for name, a, b in zip(("flags", "mu", "V", "R", "gains"), got, self.ref.block):
                assert a.tobytes() == b.tobytes(), "%s of block %d differ at %r" % (name, before, np.argwhere(a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)
                                                                                                             != b.view(np.uint8 if a.dtype == np.uint8 else np.uint32))[:5],)
            self.blocks.append(b"".join(a.tobytes() for a in got))
        assert st.tobytes() == es.tobytes(), "stats differ: %r / %r" % (st[st != es][:8], es[st != es][:8])
        assert out.tobytes() == eo.tobytes(), "out differs at %r" % (np.argwhere(out.view(np.uint32) != eo.view(np.uint32))[:5],)
        return out, st

    def run(self, x):
        done = self.enqueue(x)
        ffi.call("xengRfiSync")
        return self.check(x.shape[0], done)

    def stream(self, x, sizes):
        outs, stats, n = [], [], 0
        for nc in sizes:
            o, s = self.run(x[n:n + nc])
            outs.append(o)
            stats.append(s)
            n += nc
        assert n == x.shape[0]
        return np.concatenate(outs), np.concatenate(stats)

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengRfiCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengRfiDestroy")
        for b in (self.din, self.dout, self.dst):
            b.free()


def _sizes(rng, total, nwin):
    out = []
    while total:
        out.append(min(total, int(rng.integers(1, nwin + 1))))
        total -= out[-1]
    return out


# ---------------------------------------------------------------- 1. the three shapes, word for word
def test_shape_a_fewer_channels_than_chains_and_a_call_that_straddles_two_blocks():
    """nfine 7, one pair, blocks of 4 windows in calls of up to 3: single windows, calls ending on a block's last window, a call that
    takes a block's last window and the next one's first two.  The NaN, the constant channel and the +inf are not live in their
    blocks; the first nstat outputs are +0 with stats {0, 0, 4, 0}."""
    nstat, nwin = 4, 3
    x = rfi_cases.scene(1, 20, 1, 7, nstat)
    rf = RF(1, 7, nwin, nstat)
    rf.control(*rfi_cases.controls(7, min_fraction=0.3))
    out, st = rf.stream(x, [1, 3, 3, 3, 2, 3, 1, 1, 3])
    assert _info() == (20, 5) and len(rf.blocks) == 5
    assert not out[:nstat].view(np.uint32).any() and (st[:nstat].reshape(-1, 4) == [0, 0, 4, 0]).all() and (st[nstat:, :, 2] != 4).all()
    rf.close()


def test_shape_b_chains_of_one_and_two_a_dead_pair_a_masked_channel_and_every_window_code():
    """nfine 300, three pairs, nwin = nstat = 16, three blocks under a mask: pair 2 is dead (count 0, code 1), the spike window has
    code 2 and the window after it, half its band clipped, code 1; masked channels carry bit 0."""
    nstat = nwin = 16
    x = rfi_cases.scene(2, 48, 3, 300, nstat, dead_pair=2)
    mask = np.zeros(300, np.uint8)
    mask[[0, 17, 299]] = 1
    rf = RF(3, 300, nwin, nstat)
    rf.control(*rfi_cases.controls(300))
    rf.mask(mask)
    out, st = rf.stream(x, [16, 7, 9, 16])
    flags = rf.ref.block[0]
    assert (flags[:, [0, 17, 299]] & 1).all() and (flags[2] & 2).all() and (flags[:, 3] & 2).all()
    assert (st[nstat:, 2, 0] == 0).all() and (st[nstat:, 2, 2] == 1).all() and not out[:, 2].view(np.uint32).any()
    assert st[nstat + 8, 0, 2] == 2 and st[nstat + 9, 0, 2] == 1 and st[nstat + 9, 0, 1] >= 140
    rf.close()


def test_shape_c_the_live_channel_count():
    """nfine 3072 (twelve channels a chain), two pairs, blocks of 32 windows in calls of 30 and the rest: two blocks and what can be
    read of them."""
    nstat, nwin = 32, 30
    x = rfi_cases.scene(3, 96, 2, 3072, nstat)
    rf = RF(2, 3072, nwin, nstat)
    rf.control(*rfi_cases.controls(3072))
    out, st = rf.stream(x, [30, 30, 30, 6])
    assert _info() == (96, 3) and (st[nstat:, :, 2] != 4).all() and st[nstat + 16, 0, 2] == 2
    assert rf.blocks[1] != rf.blocks[2]
    rf.close()


# ---------------------------------------------------------------- 2. the tie rule, in integers
def test_integer_scene_with_equal_r_in_many_channels():
    """Small integers with the same statistics in 30 of 40 channels: equal R (ties by index), mad = 0, so the ten channels with
    another R are outliers whatever k_chan is; v = 1 exactly in the kept channels, their gains 1."""
    x = rfi_cases.integer_scene(12, 40)
    rf = RF(1, 40, 3, 4)
    rf.control(*rfi_cases.controls(40))
    out, st = rf.stream(x, [3, 3, 3, 3])
    flags, mu, var, r, g = rf.ref.block
    odd = np.arange(40) % 4 == 1
    assert (flags[0][odd] == 4).all() and (flags[0][~odd] == 0).all() and (st[4:, 0, 3] == 10).all()
    assert (var[0][~odd] == 2.0).all() and (g[0][~odd] == 1.0).all() and (mu[0] == np.where(odd, 20.0, 18.0)).all()
    rf.close()


# ---------------------------------------------------------------- 3. bit identity
def test_bit_identical_across_splits_reset_and_concurrent_kernels():
    """Five blocks of 8 windows and 5 windows more, 2 pairs of 70 channels: calls of one window, of 8 (every call ends on a block's last
    window), of 6 (straddling calls) and a random split.  Each run follows a Reset -- the second one after 11 windows of another
    run, which must leave no trace -- and gives the same out, stats and tables bit for bit; so does a fresh context run while
    X-engine contractions and xengBeamformRun are in flight."""
    nstat, nwin, npair, nfine, total = 8, 8, 2, 70, 45
    rng = np.random.default_rng(17)
    x = rfi_cases.scene(4, total, npair, nfine, nstat)
    splits = [[1] * total, [8] * 5 + [5], [6] * 7 + [3], _sizes(rng, total, nwin)]
    rf = RF(npair, nfine, nwin, nstat)
    rf.control(*rfi_cases.controls(nfine))
    outs = []
    for i, sizes in enumerate(splits):
        if i == 1:
            rf.stream(100 + x[:11][::-1], [8, 3])
        rf.reset()
        rf.blocks = []
        o, s = rf.stream(x, sizes)
        assert _info() == (total, 5)
        outs.append((o.tobytes(), s.tobytes(), list(rf.blocks)))
    rf.close()
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    rf = RF(npair, nfine, nwin, nstat)
    rf.control(*rfi_cases.controls(nfine))
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        o, s, n = [], [], 0
        for nc in splits[2]:
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            done = rf.enqueue(x[n:n + nc])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengRfiSync")
            a, b = rf.check(nc, done)
            o.append(a)
            s.append(b)
            n += nc
        ffi.call("xengXgpuSync")
        outs.append((np.concatenate(o).tobytes(), np.concatenate(s).tobytes(), rf.blocks))
    finally:
        xg.close()
    rf.close()
    ffi.call("xengBeamformDestroy")
    for other in outs[1:]:
        assert other == outs[0]


def test_controls_and_mask_given_mid_block_hold_from_the_next_block_and_zerodm():
    """Blocks of 8 windows, one pair of 64 channels.  SetControl (zerodm off, another clip) and SetMask given after 11 windows, inside
    block 1, leave block 0's windows -- still to come out -- alone and hold from block 1, which the call that takes window 15
    decides.  With zerodm the sum of a window's words over the channels is a rounding error; without it, it is not."""
    nstat, nwin, nfine = 8, 4, 64
    x = rfi_cases.scene(6, 32, 1, nfine, nstat)
    mask = (np.arange(nfine) % 16 == 7).astype(np.uint8)
    rf = RF(1, nfine, nwin, nstat)
    rf.control(*rfi_cases.controls(nfine, min_fraction=0.1))
    o0, s0 = rf.stream(x[:11], [4, 4, 3])
    assert not (rf.ref.block[0] & 1).any()
    rf.control(*rfi_cases.controls(nfine, zerodm=False, min_fraction=0.1))
    rf.mask(mask)
    o1, s1 = rf.stream(x[11:], [1, 4, 4, 4, 4, 4])
    out, st = np.concatenate([o0, o1]), np.concatenate([s0, s1])
    assert (rf.ref.block[0][0][mask == 1] & 1).all() and (st[8:16, 0, 3] < st[16:24, 0, 3]).all()
    ok = st[:, 0, 2] == 0
    z = np.abs(out[:, 0, :, :2].astype(np.float64).sum(axis=(1, 2)))
    assert ok[8:16].sum() >= 4 and z[8:16][ok[8:16]].max() < 1e-3 and ok[16:].sum() >= 8 and z[16:][ok[16:]].max() > 0.5
    rf.close()


# ---------------------------------------------------------------- 4. the ABI
def test_refusals_and_calls_without_a_context():
    bad = ctypes.c_int(-1)
    ffi.call("xengRfiDestroy")
    for name, args in (("xengRfiRun", (16, 1, 16, 16, ctypes.byref(bad))), ("xengRfiReset", ()), ("xengRfiSetMask", (None,)),
                       ("xengRfiSetControl", (1.0, 1.0, 1.0, 1, 1)), ("xengRfiSync", ())):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    for sizes in ((0, 16, 4, 8), (65536, 16, 4, 8), (1, 3, 4, 8), (1, 8193, 4, 8), (1, 16, 0, 8), (1, 16, 9, 8), (1, 16, 1, 1), (1, 16, 4, (1 << 20) + 1),
                  (16, 8192, 1 << 10, 1 << 11)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengRfiInitialize", 0, *sizes)
        assert ei.value.status == INVALID_ARGUMENT, sizes
    rf = RF(1, 16, 4, 8)
    done = ctypes.c_int(-1)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengRfiRun", rf.din.ptr, 1, rf.dout.ptr + GUARD, rf.dst.ptr + GUARD, ctypes.byref(done))
    assert ei.value.status == INVALID_STATE and b"SetControl" in ffi.lib().xengGetLastError()
    for ctl in ((0.0, 1.0, 1.0, 1, 1), (1.0, float('nan'), 1.0, 1, 1), (1.0, 1.0, float('inf'), 1, 1), (1.0, 1.0, -1.0, 1, 1), (1.0, 1.0, 1.0, -1, 1),
                (1.0, 1.0, 1.0, 17, 1), (1.0, 1.0, 1.0, 1, 2)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengRfiSetControl", *ctl)
        assert ei.value.status == INVALID_ARGUMENT, ctl
    rf.control(*rfi_cases.controls(16))
    for args in ((None, 1, rf.dout.ptr, rf.dst.ptr, ctypes.byref(done)), (rf.din.ptr, 1, None, rf.dst.ptr, ctypes.byref(done)),
                 (rf.din.ptr, 1, rf.dout.ptr, None, ctypes.byref(done)), (rf.din.ptr, 1, rf.dout.ptr, rf.dst.ptr, None),
                 (rf.din.ptr + 4, 1, rf.dout.ptr, rf.dst.ptr, ctypes.byref(done)), (rf.din.ptr, 1, rf.dout.ptr + 8, rf.dst.ptr, ctypes.byref(done)),
                 (rf.din.ptr, 1, rf.dout.ptr, rf.dst.ptr + 4, ctypes.byref(done)), (rf.din.ptr, 0, rf.dout.ptr, rf.dst.ptr, ctypes.byref(done)),
                 (rf.din.ptr, 5, rf.dout.ptr, rf.dst.ptr, ctypes.byref(done))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengRfiRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    assert done.value == -1 and _info() == (0, 0)
    with pytest.raises(ffi.XengError) as ei:
        rf.tables()
    assert ei.value.status == INVALID_STATE
    x = rfi_cases.scene(9, 8, 1, 16, 8)
    rf.stream(x, [4, 4])
    assert _info() == (8, 1)
    t = ctypes.c_ulonglong()
    ffi.call("xengRfiMark", ctypes.byref(t))
    ffi.call("xengRfiWait", t.value)
    d = ctypes.c_int()
    ffi.call("xengRfiTicketDone", t.value, ctypes.byref(d))
    assert d.value == 1
    rf.close()


def test_backend_methods():
    from caltech_bifrost_dsp_amd.backend import HipBackend
    from caltech_bifrost_dsp_amd.ndarray import XArray
    be = HipBackend()
    nstat, nwin, npair, nfine = 4, 4, 2, 12
    x = rfi_cases.scene(10, 8, npair, nfine, nstat)
    assert be.rfi_initialize(0, npair, nfine, nwin, nstat) == 0
    ctl = rfi_cases.controls(nfine)
    assert be.rfi_set_control(*ctl) == 0 and be.rfi_set_mask(None) == 0
    ref = rfi_ref.RfiRef(npair, nfine, nstat)
    ref.set_control(*ctl)
    out, st = XArray(shape=(nwin, npair, nfine, 4), dtype=np.float32, space='cuda'), XArray(shape=(nwin, npair, 4), dtype=np.int32, space='cuda')
    for k in range(2):
        rv, done = be.rfi_run(XArray(x[k * nwin:(k + 1) * nwin], space='cuda'), nwin, out, st)
        assert (rv, done) == (0, 1)
        be.rfi_wait(be.rfi_mark())
        eo, es = ref.run(x[k * nwin:(k + 1) * nwin])
        assert out.numpy().tobytes() == eo.tobytes() and st.numpy().tobytes() == es.tobytes()
    assert be.rfi_info() == (8, 2) and all(a.tobytes() == b.tobytes() for a, b in zip(be.rfi_block(npair, nfine), ref.block))
    be.rfi_reset()
    assert be.rfi_info() == (0, 0) and be.rfi_guards_intact()
    be.rfi_sync()
    ffi.call("xengRfiDestroy")


# ---------------------------------------------------------------- 5. the chain on device rings
def test_chain_upchan_sum_beams_rfi_clean_dedisperse_on_device_rings():
    """Source -> Beamform -> UpchanSumBeams -> BeamRfiClean -> BeamDedisperse, 3 windows a gulp, blocks of 6 windows: the cleaner
    writes two spans fewer than it reads, output span j is the restatement's cleaning of the span UpchanSumBeams wrote as its j-th
    byte for byte, under the input's seq0 and time tag, and the dedisperser behind it sums what the cleaner wrote."""
    from tests.test_dedisp_gpu import EPS, _beam_cmds
    nchan, nstand, nbeam, g, N, W, ngulp = 4, 32, 8, 96, 16, 2, 8
    dms = [0.0, 0.5, 1.0]
    nwin, npair, nfine, nstat = g // N // W, nbeam // 2, nchan * N, 6
    ninput = 2 * nstand
    vin = np.random.default_rng(0xc0ffee).integers(0, 256, (ngulp * g, nchan, ninput), dtype=np.uint8)
    r0, r1, r2 = Ring("gpu-input", space="cuda"), Ring("bf-output", space="cuda"), Ring("ub-output", space="cuda")
    r3, r4 = Ring("rc-output", space="cuda"), Ring("dd-output", space="cuda_host")
    bf = Beamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, gpu=0)
    sfreq, bw = 40e6, 23925.78125
    bf.freqs = sfreq + bw * np.arange(nchan)
    bf.process_command_strings(_beam_cmds(nchan, nbeam, ninput, np.random.default_rng(0x5eed))[0])
    ub = UpchanSumBeams(LOG, r1, r2, nchan=nchan, nbeam=nbeam, ntime_gulp=g, nupchan=N, nframe_sum=W, gpu=0)
    rc = BeamRfiClean(LOG, r2, r3, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nstat=nstat, min_fraction=0.25, gpu=0)
    dd = BeamDedisperse(LOG, r3, r4, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, dms=dms, gpu=0)
    span = nwin * npair * nfine * 16
    s_ub, s_rc, s_dd = Sink(r2, span), Sink(r3, span), Sink(r4, nwin * npair * len(dms) * 4)
    run_blocks([bf, ub, rc, dd], Source(r0, [(source_header(nchan, nstand, 2, sfreq=sfreq, chan_bw=bw), vin, g * nchan * ninput)]), [s_ub, s_rc, s_dd])
    (uh, utag, usp), = s_ub.sequences
    (rh, rtag, rsp), = s_rc.sequences
    (dh, dtag, dsp), = s_dd.sequences
    head = nstat // nwin
    assert len(usp) == ngulp and len(rsp) == len(dsp) == ngulp - head
    assert rtag == utag == dtag and rh['seq0'] == uh['seq0'] and rh['rfi_cleaned'] is True and rh['rfi_nstat'] == nstat and rh['rfi_zerodm'] is True
    assert (rh['rfi_nsig_chan'], rh['rfi_nsig_clip'], rh['rfi_nsig_broad'], rh['rfi_min_fraction']) == (5.0, 6.0, 5.0, 0.25)
    ref = rfi_ref.RfiRef(npair, nfine, nstat)
    ref.set_control(*(rfi_controls(nfine=nfine, min_fraction=0.25) + (1,)))
    exp = [ref.run(s.view(np.float32).reshape(nwin, npair, nfine, 4))[0] for s in usp][head:]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rsp, exp)) and any(e.any() for e in exp)
    assert rc.stats['nwindow'] == ngulp * nwin and rc.stats['nblock'] == ngulp * nwin // nstat and 0 <= rc.stats['frac_samples'] < 1
    y = np.concatenate([s.view(np.float32).reshape(nwin, npair, nfine, 4) for s in rsp])
    tsamp = W * N * nchan / uh['bw_hz']
    table = dm_delays(uh['fine_sfreq'] + uh['fine_bw_hz'] * np.arange(nfine), dms, tsamp)
    got = np.concatenate([s.view(np.float32).reshape(nwin, npair, len(dms), 1) for s in dsp]).astype(np.float64)
    want = dedisperse(y, table, None, 1)
    assert (np.abs(got - want) <= (nfine + 2) * EPS * dedisperse(y, table, None, 1, absolute=True)).all()
