"""BeamDedisperse on the MI355X: xengDedisp* against the restatement (tests/dedisp_ref.py).  Word for word on integer data
(both products, S = 0, S beyond a call, a ring wrapped several times, ragged sizes, more windows than a wave has lanes, the live
shape with an injected dispersed pulse); bit identity across splits of a run over calls, after Reset against a fresh context
and beside an X-engine contraction and xengBeamformRun; float data word for word against the contract's summation order in
float32 steps (dedisperse_ordered32); NaN / Inf in zero-weight channels; float data against the a-priori
bound of an fp32 sum and the house bar of 1e-5 of the RMS; guard bands around every output and around the history; the checks
that need a context; and Beamform -> UpchanSumBeams -> BeamDedisperse on device rings beside BeamformSumBeams.  No wall-clock
assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Beamform, BeamDedisperse, BeamformSumBeams, UpchanSumBeams, dm_delays  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import dedisp_cases  # noqa: E402
from tests.dedisp_ref import dedisperse, dedisperse_ordered32  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_blocks_cpu import _beam_cmds  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
EPS = 2.0 ** -24


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    s, n = ctypes.c_int(), ctypes.c_longlong()
    ffi.call("xengDedispGetInfo", ctypes.byref(s), ctypes.byref(n))
    return s.value, n.value


class DD:
    """The xengDedisp context (one per process), an input buffer and an output between two poisoned guard bands."""

    def __init__(self, npair, nfine, nwin, ndm, max_delay, nprod, delays=None, weights=None):
        self.npair, self.nfine, self.nwin, self.ndm, self.nprod = npair, nfine, nwin, ndm, nprod
        ffi.call("xengDedispInitialize", 0, npair, nfine, nwin, ndm, max_delay, nprod)
        self.din = ffi.DeviceBuffer(nwin * npair * nfine * 16)
        self.dout = ffi.DeviceBuffer(2 * GUARD + nwin * npair * ndm * nprod * 4)
        if weights is not None:
            self.set_weights(weights)
        if delays is not None:
            self.set_delays(delays)

    def set_delays(self, s):
        self.s = np.ascontiguousarray(s, np.int32)
        ffi.call("xengDedispSetDelays", _ip(self.s))

    def set_weights(self, w):
        self.w = None if w is None else np.ascontiguousarray(w, np.float32)
        ffi.call("xengDedispSetWeights", _fp(self.w))

    def enqueue(self, x):
        nc = x.shape[0]
        assert x.shape == (nc, self.npair, self.nfine, 4)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        self.din.upload(np.ascontiguousarray(x, np.float32))
        ffi.call("xengDedispRun", self.din.ptr, nc, self.dout.ptr + GUARD)
        return nc

    def result(self, nc):
        """After a sync: the nc windows written; every byte before and after them (the rest of a full-size span included) must
        still be poison."""
        raw = self.dout.download(np.uint8)
        n = nc * self.npair * self.ndm * self.nprod * 4
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + n:] == POISON).all(), "bytes past the output's %d windows were written" % nc
        return raw[GUARD:GUARD + n].view(np.float32).reshape(nc, self.npair, self.ndm, self.nprod).copy()

    def run(self, x):
        nc = self.enqueue(x)
        ffi.call("xengDedispSync")
        return self.result(nc)

    def stream(self, x, sizes):
        """Consecutive calls of the given sizes over the windows of x; the outputs one after the other."""
        outs, n = [], 0
        for nc in sizes:
            outs.append(self.run(x[n:n + nc]))
            n += nc
        assert n == x.shape[0]
        return np.concatenate(outs)

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengDedispCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the history ring were written"
        ffi.call("xengDedispDestroy")


def _sizes(rng, total, nwin):
    out = []
    while total:
        out.append(int(min(total, rng.integers(1, nwin + 1))))
        total -= out[-1]
    return out


def _dm_like_table(ndm, nfine, S):
    """Delays that grow with the trial and towards low channels, 0 at the top channel and at trial 0, S at (ndm-1, 0)."""
    d = np.arange(ndm)[:, None] / max(ndm - 1, 1)
    q = 1.0 - np.arange(nfine)[None, :] / max(nfine - 1, 1)
    s = np.rint(S * d * q * q).astype(np.int32)
    s[-1, 0] = S
    return s


# ---------------------------------------------------------------- exact on integer data
CASES = {
    # npair, nfine, nwin, ndm, S, windows
    "no delay": (2, 70, 5, 5, 0, 23),
    "S beyond a call, ring wrapped": (3, 130, 4, 7, 11, 61),          # L = 17: wrapped three times
    "one trial, fewer channels than segments": (1, 3, 3, 1, 2, 14),
    "deep history": (2, 64, 8, 9, 300, 700),
    "more windows than lanes": (1, 40, 70, 3, 5, 200),
}


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("case", sorted(CASES))
def test_integer_data_match_the_restatement_word_for_word(case, nprod):
    """Random tables (any non-negative delays are a table), integer data and integer weights with zeros, calls of random
    sizes; halfway SetWeights changes the weights, which the history (kept unweighted) takes on at once.  Every sum is below
    2^24, so fp32 is exact and the output equals the int64 restatement."""
    npair, nfine, nwin, ndm, S, total = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case) * 10 + nprod)
    s = rng.integers(0, S + 1, (ndm, nfine)).astype(np.int32)
    s[rng.integers(ndm), rng.integers(nfine)] = S
    x = rng.integers(-5 if nprod == 4 else 0, 10, (total, npair, nfine, 4)).astype(np.float32)
    w0, w1 = (rng.integers(0, 4, nfine).astype(np.float32) for _ in range(2))
    dd = DD(npair, nfine, nwin, ndm, S + 2, nprod, s, w0)
    assert _info() == (S, 0)
    half = total // 2
    got0 = dd.stream(x[:half], _sizes(rng, half, nwin))
    assert _info() == (S, half)
    dd.set_weights(w1)
    assert _info() == (S, half)
    got1 = dd.stream(x[half:], _sizes(rng, total - half, nwin))
    exp0 = dedisperse(x, s, w0, nprod, np.int64)[:half]
    exp1 = dedisperse(x, s, w1, nprod, np.int64)[half:]
    assert np.abs(exp0).max() < 2 ** 24 and np.abs(exp1).max() < 2 ** 24
    assert np.array_equal(got0.astype(np.int64), exp0) and np.array_equal(got1.astype(np.int64), exp1)
    # a new table clears the history and the count: the same windows again, from nothing
    dd.set_delays(s)
    assert _info() == (S, 0)
    n = min(total, 3 * nwin)
    assert np.array_equal(dd.stream(x[:n], _sizes(rng, n, nwin)).astype(np.int64), dedisperse(x[:n], s, w1, nprod, np.int64))
    dd.close()


def test_live_shape_with_an_injected_pulse():
    """16 pairs x 3072 fine channels x 30 windows per call, 256 trials up to DM 30 at 50 MHz with 40 ms windows (S = 107), five
    calls (the ring of 137 windows wraps): word for word the int64 restatement, and a pulse of 1000 in XX dispersed at trial
    200 peaks at (t0 + S, 200) with nfine * amp + the background under it."""
    npair, nchan, N, nwin, ndm, ncall, t0, d0, amp = 16, 96, 32, 30, 256, 5, 20, 200, 1000
    nfine = nchan * N
    bw = 23925.78125
    freqs = 50e6 - bw / 2 + bw / N * np.arange(nfine)
    s = dm_delays(freqs, np.linspace(0, 30, ndm), 30 * N / bw)
    S = int(s.max())
    assert 100 <= S <= 115
    rng = np.random.default_rng(42)
    x = rng.integers(0, 4, (ncall * nwin, npair, nfine, 4)).astype(np.float32)
    q = np.arange(nfine)
    under = (x[t0 + s[d0], :, q, 0] + x[t0 + s[d0], :, q, 1]).sum(axis=0)        # [npair]
    x[t0 + s[d0], :, q, 0] += amp
    dd = DD(npair, nfine, nwin, ndm, S, 1, s)
    got = dd.stream(x, [nwin] * ncall)
    assert np.array_equal(got.astype(np.int64), dedisperse(x, s, None, 1, np.int64))
    for p in range(npair):
        plane = got[:, p, :, 0]
        assert np.unravel_index(plane.argmax(), plane.shape) == (t0 + S, d0)
        assert plane[t0 + S, d0] == nfine * amp + under[p]
    dd.close()


# ---------------------------------------------------------------- bit identity
def _float_case(rng, nwindows, npair, nfine, nprod):
    x = rng.chisquare(4, (nwindows, npair, nfine, 4)).astype(np.float32)
    if nprod == 4:
        x[..., 2:] = rng.standard_normal((nwindows, npair, nfine, 2)).astype(np.float32)
    return x, rng.uniform(0.5, 1.5, nfine).astype(np.float32)


@pytest.mark.parametrize("nprod", [1, 4])
def test_bit_identical_across_splits_reset_and_concurrent_kernels(nprod):
    """90 windows of float data: three calls of 30 equal nine of 10 and ninety of 1 bit for bit (each after a Reset, so the ring
    position differs too), and equal a fresh context run while X-engine contractions and xengBeamformRun are in flight."""
    npair, nfine, nwin, ndm, S, total = 4, 515, 30, 33, 47, 90
    rng = np.random.default_rng(7 + nprod)
    x, w = _float_case(rng, total, npair, nfine, nprod)
    w[rng.integers(0, nfine, 20)] = 0
    s = _dm_like_table(ndm, nfine, S)
    dd = DD(npair, nfine, nwin, ndm, S + 5, nprod, s, w)
    a = dd.stream(x, [30] * 3)
    outs = []
    for step in (10, 1):
        ffi.call("xengDedispReset")
        assert _info() == (S, 0)
        outs.append(dd.stream(x, [step] * (total // step)))
    dd.close()
    # a fresh context beside other work: contractions on their own stream, the beamformer on this one
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    dd = DD(npair, nfine, nwin, ndm, S + 5, nprod, s, w)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        parts = []
        for k in range(3):
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            nc = dd.enqueue(x[30 * k:30 * k + 30])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengDedispSync")
            parts.append(dd.result(nc))
        ffi.call("xengXgpuSync")
        outs.append(np.concatenate(parts))
    finally:
        xg.close()
    dd.close()
    ffi.call("xengBeamformDestroy")
    for o in outs:
        assert np.array_equal(a.view(np.uint32), o.view(np.uint32))
    assert np.isfinite(a).all()


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_float_data_match_the_contracts_summation_order_bit_for_bit(case, nprod):
    """The public summation order on the device: float data (weights in [0.5, 1.5] with an eighth 0, NaN in those channels) in
    the calls of tests/dedisp_cases.py -- (a) nfine 70, Q = 18, ragged tiles, a ring of 16 slots wrapped three times; (b) fewer
    channels than segments; (c) more windows than a wave has lanes -- equal the ordered float32 restatement (four segments, one
    fmaf a channel from +0, ((P0 + P1) + P2) + P3) as uint32 words.  One ascending chain over all channels differs from it in
    most words of case (a) (tests/test_dedisp_cpu.py), and so would a product that is not fused."""
    c = dedisp_cases.CASES[case]
    x, s, w = dedisp_cases.float_case(case, nprod)
    dd = DD(c["npair"], c["nfine"], c["nwin"], c["ndm"], c["S"], nprod, s, w)
    got = dd.stream(x, c["calls"])
    dd.close()
    exp = dedisperse_ordered32(x, s, w, nprod)
    diff = got.view(np.uint32) != exp.view(np.uint32)
    print("dedisp ordered case %s nprod=%d: %d of %d words differ" % (case, nprod, diff.sum(), diff.size))
    assert np.isfinite(got).all() and not diff.any(), "%d of %d words differ, first at %s" % (diff.sum(), diff.size, np.argwhere(diff)[:1])


@pytest.mark.parametrize("nprod", [1, 4])
def test_nan_and_inf_in_zero_weight_channels_never_reach_an_output(nprod):
    npair, nfine, nwin, ndm, S, total = 2, 200, 16, 12, 21, 64
    rng = np.random.default_rng(17 + nprod)
    x, w = _float_case(rng, total, npair, nfine, nprod)
    off = rng.choice(nfine, 30, replace=False)
    w[off] = 0
    s = _dm_like_table(ndm, nfine, S)
    dd = DD(npair, nfine, nwin, ndm, S, nprod, s, w)
    clean = dd.stream(x, [nwin] * (total // nwin))
    bad = x.copy()
    bad[:, :, off[:10]] = np.nan
    bad[::3, :, off[10:20], 0] = np.inf
    bad[1::3, :, off[20:], 1] = -np.inf
    ffi.call("xengDedispReset")
    dirty = dd.stream(bad, [nwin] * (total // nwin))
    dd.close()
    assert np.isfinite(dirty).all() and np.array_equal(clean.view(np.uint32), dirty.view(np.uint32))


# ---------------------------------------------------------------- float data
@pytest.mark.parametrize("nprod", [1, 4])
def test_float_data_within_the_a_priori_bound_and_the_house_bar(nprod):
    """chi^2-like powers, weights in [0.5, 1.5], nfine = 3072, S = 107, 150 windows in calls of 30.  Per output
    |got - ref| <= (nfine + 2) * 2^-24 * sum_q |w x| (an fp32 sum of nfine terms in any order, one rounding for I and one for
    the product); and max |got - ref| <= 1e-5 of the RMS of each product's output plane.  On the MI355X the worst ratios
    measured are recorded in DESIGN.md 4.16."""
    npair, nfine, nwin, ndm, S, total = 2, 3072, 30, 64, 107, 150
    rng = np.random.default_rng(27 + nprod)
    x, w = _float_case(rng, total, npair, nfine, nprod)
    s = _dm_like_table(ndm, nfine, S)
    dd = DD(npair, nfine, nwin, ndm, S, nprod, s, w)
    got = dd.stream(x, [nwin] * (total // nwin)).astype(np.float64)
    dd.close()
    ref = dedisperse(x, s, w, nprod)
    bound = (nfine + 2) * EPS * dedisperse(x, s, w, nprod, absolute=True)
    err = np.abs(got - ref)
    full = bound > 0
    worst_bound = (err[full] / bound[full]).max()
    worst_rms = max(err[..., k].max() / np.sqrt(np.mean(ref[..., k] ** 2)) for k in range(nprod))
    print("dedisp float nprod=%d: worst |err| / a-priori bound = %.3g, worst |err| / RMS = %.3g" % (nprod, worst_bound, worst_rms))
    assert (err <= bound).all(), "worst |err| / bound = %.3g" % worst_bound
    assert worst_rms <= 1e-5, "worst |err| = %.3g of the plane's RMS" % worst_rms


# ---------------------------------------------------------------- what needs a context
def test_argument_checks_with_a_context():
    """Run before SetDelays: INVALID_STATE.  nwin_call outside 1..nwin, misaligned pointers, a negative delay or one above
    max_delay, a non-finite weight: INVALID_ARGUMENT, nothing launched and the state unchanged."""
    dd = DD(2, 16, 4, 3, 9, 1)
    assert _info() == (-1, 0)
    x = np.ones((4, 2, 16, 4), np.float32)
    with pytest.raises(ffi.XengError) as ei:
        dd.enqueue(x)
    assert ei.value.status == INVALID_STATE
    s = np.zeros((3, 16), np.int32)
    for bad in (-1, 10):
        t = s.copy()
        t[1, 5] = bad
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengDedispSetDelays", _ip(t))
        assert ei.value.status == INVALID_ARGUMENT and _info() == (-1, 0)
    s[2, 0] = 9
    dd.set_delays(s)
    assert _info() == (9, 0)
    for args in ((dd.din.ptr, 0, dd.dout.ptr), (dd.din.ptr, 5, dd.dout.ptr), (dd.din.ptr + 4, 1, dd.dout.ptr), (dd.din.ptr, 1, dd.dout.ptr + 8)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengDedispRun", *args)
        assert ei.value.status == INVALID_ARGUMENT and _info() == (9, 0)
    for v in (np.nan, np.inf):
        w = np.ones(16, np.float32)
        w[3] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengDedispSetWeights", _fp(w))
        assert ei.value.status == INVALID_ARGUMENT
    y = dd.run(x)[..., 0]                # (b = 9 everywhere but at channel 0 of trial 2: after 4 windows nothing else has arrived)
    assert (y[:, :, 2] == 2.0).all() and (y[:, :, :2] == 0.0).all()
    assert _info() == (9, 4)
    t = ctypes.c_ulonglong()
    ffi.call("xengDedispMark", ctypes.byref(t))
    ffi.call("xengDedispWait", t.value)
    done = ctypes.c_int()
    ffi.call("xengDedispTicketDone", t.value, ctypes.byref(done))
    assert done.value == 1
    dd.close()


# ---------------------------------------------------------------- the block at the end of the live chain, on device rings
def _chain(with_dedisp, vin, nchan, nstand, nbeam, g, ns, N, W, dms):
    """Source -> Beamform -> {BeamformSumBeams, UpchanSumBeams -> BeamDedisperse (with_dedisp)} on device rings; returns the
    sinks' sequences: BeamformSumBeams' output, and UpchanSumBeams' and BeamDedisperse's (or None)."""
    ninput = 2 * nstand
    rng = np.random.default_rng(0x5eed)
    r0, r1, r2 = Ring("gpu-input", space="cuda"), Ring("bf-output", space="cuda"), Ring("bf-pow-output", space="cuda_host")
    bf = Beamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, gpu=0)
    sb = BeamformSumBeams(LOG, r1, r2, nchan=nchan, ntime_gulp=g, ntime_sum=ns, gpu=0)
    sfreq, bw = 40e6, 23925.78125
    bf.freqs = sfreq + bw * np.arange(nchan)
    bf.process_command_strings(_beam_cmds(nchan, nbeam, ninput, rng)[0])
    blocks, sinks = [bf, sb], [Sink(r2, (nbeam // 2) * (g // ns) * nchan * 16)]
    if with_dedisp:
        nwin = g // N // W
        r3, r4 = Ring("ub-output", space="cuda"), Ring("dd-output", space="cuda_host")
        blocks.append(UpchanSumBeams(LOG, r1, r3, nchan=nchan, nbeam=nbeam, ntime_gulp=g, nupchan=N, nframe_sum=W, gpu=0))
        blocks.append(BeamDedisperse(LOG, r3, r4, npair=nbeam // 2, nchan=nchan, nupchan=N, nwin=nwin, dms=dms, gpu=0))
        sinks += [Sink(r3, nwin * (nbeam // 2) * nchan * N * 16), Sink(r4, nwin * (nbeam // 2) * len(dms) * 4)]
    run_blocks(blocks, Source(r0, [(source_header(nchan, nstand, 2, sfreq=sfreq, chan_bw=bw), vin, g * nchan * ninput)]), sinks)
    return [s.sequences for s in sinks] + ([None, None] if not with_dedisp else [])


def test_block_after_upchan_sum_beams_on_device_rings():
    """8 gulps through Beamform and UpchanSumBeams (3 windows of 2 frames per gulp) into BeamDedisperse, 5 trials up to DM 1 at
    40 MHz: its output equals the restatement applied to the spans UpchanSumBeams wrote, with the table of the formula at the
    header's frequencies, within the a-priori bound and 1e-5 of the RMS; BeamformSumBeams' output beside it is bit for bit what
    it is without the two readers."""
    nchan, nstand, nbeam, g, ns, N, W, ngulp = 4, 32, 8, 96, 24, 16, 2, 8
    dms = [0.0, 0.25, 0.5, 0.75, 1.0]
    nwin, npair, nfine = g // N // W, nbeam // 2, nchan * N
    vin = np.random.default_rng(0xc0ffee).integers(0, 256, (ngulp * g, nchan, 2 * nstand), dtype=np.uint8)
    pow_with, ub, dd = _chain(True, vin, nchan, nstand, nbeam, g, ns, N, W, dms)
    pow_without, _, _ = _chain(False, vin, nchan, nstand, nbeam, g, ns, N, W, dms)
    (uh, _, usp), = ub
    (hd, _, dsp), = dd
    assert len(usp) == len(dsp) == ngulp
    x = np.concatenate([s.view(np.float32).reshape(nwin, npair, nfine, 4) for s in usp])
    tsamp = W * N * nchan / uh['bw_hz']
    table = dm_delays(uh['fine_sfreq'] + uh['fine_bw_hz'] * np.arange(nfine), dms, tsamp)
    S = int(table.max())
    assert 3 < S < ngulp * nwin
    assert hd['ndm'] == len(dms) and hd['dms'] == dms and hd['dedisp_latency'] == S and hd['nprod'] == 1 and hd['tsamp'] == tsamp
    got = np.concatenate([s.view(np.float32).reshape(nwin, npair, len(dms), 1) for s in dsp]).astype(np.float64)
    ref = dedisperse(x, table, None, 1)
    err = np.abs(got - ref)
    assert (err <= (nfine + 2) * EPS * dedisperse(x, table, None, 1, absolute=True)).all()
    assert err.max() <= 1e-5 * np.sqrt(np.mean(ref ** 2))
    (_, _, a), = pow_with
    (_, _, b), = pow_without
    assert len(a) == len(b) == ngulp and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
