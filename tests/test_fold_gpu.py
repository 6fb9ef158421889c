"""BeamFold on the MI355X: xengFold* against the restatement (tests/fold_ref.py).  The accumulation bit for bit on integer and on
float data (calls of 1, 7 and 30 windows; bins revisited within a call, empty bins, many windows per bin, ddphi of either sign, a
pair left out, a SetPhase mid-run); bit identity across splits of a run over calls, after Reset against a fresh context and
beside an X-engine contraction and xengBeamformRun; the dump (nfscr 1, a few channels, nfine; rotations that wrap; normalise;
clear = 0 then more windows against clear = 1; NaN / Inf; weights against the a-priori bound); an injected pulsar; guard bands
around every output and around the profile; the checks that need a context; and Beamform -> UpchanSumBeams -> BeamFold on device
rings beside BeamformSumBeams.  No wall-clock assertions."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Beamform, BeamFold, BeamformSumBeams, UpchanSumBeams, fold_rotations, profile_snr  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.fold_ref import MASK, FoldRef  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_blocks_cpu import _beam_cmds  # noqa: E402
from tests.test_fold_cpu import _subints  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
EPS = 2.0 ** -24


def _info():
    n, f = ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengFoldGetInfo", ctypes.byref(n), ctypes.byref(f))
    return n.value, f.value


def _period_osc(period, phase=0.0, ddphi=0, active=1):
    """(phi0, dphi, ddphi, active) of an oscillator of `period` windows per turn."""
    return (int(phase * 2 ** 64) & MASK, int(round(2 ** 64 / period)) & MASK, ddphi, active)


class FO:
    """The xengFold context (one per process) beside its restatement: every call goes to both.  An input buffer, and an
    output between two poisoned guard bands sized for the full cube."""

    def __init__(self, npair, nfine, nwin, nbin, nprod, mirror=True):
        self.npair, self.nfine, self.nwin, self.nbin, self.nprod = npair, nfine, nwin, nbin, nprod
        ffi.call("xengFoldInitialize", 0, npair, nfine, nwin, nbin, nprod)
        self.din = ffi.DeviceBuffer(nwin * npair * nfine * 16)
        self.dout = ffi.DeviceBuffer(2 * GUARD + npair * nprod * nfine * nbin * 4)
        self.ref = FoldRef(npair, nfine, nbin, nprod) if mirror else None

    def set_phase(self, osc, n_ref):
        a = [np.array([o[k] for o in osc], t) for k, t in enumerate((np.uint64, np.uint64, np.int64, np.uint8))]
        ffi.call("xengFoldSetPhase", a[0].ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), a[1].ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                 a[2].ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), a[3].ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), n_ref)
        if self.ref:
            self.ref.set_phase(*a, n_ref)

    def set_rotations(self, rot):
        r = None if rot is None else np.ascontiguousarray(rot, np.int32)
        ffi.call("xengFoldSetRotations", None if r is None else r.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        if self.ref:
            self.ref.set_rotations(r)

    def set_weights(self, w):
        a = None if w is None else np.ascontiguousarray(w, np.float32)
        ffi.call("xengFoldSetWeights", None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        if self.ref:
            self.ref.set_weights(a)

    def enqueue(self, x):
        nc = x.shape[0]
        assert x.shape == (nc, self.npair, self.nfine, 4)
        ffi.call("xengFoldSync")                    # (the input buffer is reused: the call before has read it)
        self.din.upload(np.ascontiguousarray(x, np.float32))
        ffi.call("xengFoldRun", self.din.ptr, nc)
        if self.ref:
            self.ref.run(x)

    def stream(self, x, sizes):
        n = 0
        for nc in sizes:
            self.enqueue(x[n:n + nc])
            n += nc
        assert n == x.shape[0]

    def dump(self, nfscr, normalise, clear):
        """(out [npair][nprod][nfine/nfscr][nbin], hits) after a sync; every byte before and after the output must still be
        poison.  With a restatement: ((out, hits) of the GPU, (out, hits) of the restatement)."""
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        hits = np.full((self.npair, self.nbin), 0xFFFFFFFF, np.uint32)
        ffi.call("xengFoldDump", self.dout.ptr + GUARD, hits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), nfscr, normalise, clear)
        ffi.call("xengFoldSync")
        raw = self.dout.download(np.uint8)
        n = self.npair * self.nprod * (self.nfine // nfscr) * self.nbin * 4
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + n:] == POISON).all(), "bytes past the output were written"
        assert self.guards_intact(), "bytes outside the profile were written"
        got = raw[GUARD:GUARD + n].view(np.float32).reshape(self.npair, self.nprod, self.nfine // nfscr, self.nbin).copy()
        if self.ref:
            return (got, hits), self.ref.dump(nfscr, normalise, clear)
        return got, hits

    def check(self, nfscr, normalise, clear):
        """A dump that must equal the restatement's bit for bit, hits included; returns it."""
        (got, hits), (exp, ehits) = self.dump(nfscr, normalise, clear)
        assert np.array_equal(hits, ehits)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), "nfscr=%d normalise=%d: %d words differ" % (
            nfscr, normalise, int((got.view(np.uint32) != exp.view(np.uint32)).sum()))
        return got, hits

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengFoldCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the profile were written"
        ffi.call("xengFoldDestroy")


def _data(rng, kind, nwindows, npair, nfine, nprod):
    """Integer values 0..49, or chi^2-like powers (the cross terms normal)."""
    if kind == "int":
        return rng.integers(0, 50, (nwindows, npair, nfine, 4)).astype(np.float32)
    x = rng.chisquare(4, (nwindows, npair, nfine, 4)).astype(np.float32)
    if nprod == 4:
        x[..., 2:] = rng.standard_normal((nwindows, npair, nfine, 2)).astype(np.float32)
    return x


def _group_sizes(nfine):
    """nfscr: the full cube, whole groups sharing a work-group, one group in several chunks with a ragged tail, everything."""
    return sorted({1, 8 if nfine % 8 == 0 else 10, nfine // 2, nfine})


# ---------------------------------------------------------------- word for word
@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("nbin", [1, 7, 64])
@pytest.mark.parametrize("nfine", [40, 130])
@pytest.mark.parametrize("kind", ["int", "float"])
def test_accumulation_and_dump_match_the_restatement_word_for_word(kind, nfine, nbin, nprod):
    """3 pairs: a period of 5.3 windows (bins met again within a call) with ddphi > 0, one of 37 windows (against 64 bins: empty
    bins, hits 0) with ddphi < 0, one of 1000.7 windows (many windows per bin); 75 windows in calls of 30, 7, 1, 30, 7; then a
    SetPhase with n_ref = the count that leaves pair 0 out and swaps the others' periods, and 38 windows more.  With unit
    weights and no rotation the full cube IS the profile (fmaf(1, x, +0) = x), so the accumulation is compared bit for bit, on
    integer and on float data alike; then the other groupings, wrapped rotations and the division by the hits, all bit for bit
    (unit weights: fmaf(1, x, s) = fl(x + s)); clear = 0 changes nothing, clear = 1 leaves +0 and hits 0."""
    npair, nwin = 3, 30
    rng = np.random.default_rng([kind == "int", nfine, nbin, nprod])
    x = _data(rng, kind, 113, npair, nfine, nprod)
    fo = FO(npair, nfine, nwin, nbin, nprod)
    fo.set_rotations(None)
    fo.set_phase([_period_osc(5.3, 0.37, 1 << 46), _period_osc(37, 0.81, -(1 << 40)), _period_osc(1000.7, 0.5)], 0)
    fo.stream(x[:75], [30, 7, 1, 30, 7])
    assert _info() == (75, 75)
    _, hits = fo.check(1, 0, 0)
    assert hits.sum() == 3 * 75 and (nbin < 64 or (hits[1] == 0).sum() >= 20)      # (37 windows a turn step over 27 of 64 bins)
    fo.set_phase([_period_osc(5.3, 0, 0, active=0), _period_osc(1000.7, 0.25, 1 << 40), _period_osc(5.3, 0.9, -(1 << 45))], 75)
    fo.stream(x[75:], [7, 30, 1])
    assert _info() == (113, 113)
    cube, hits = fo.check(1, 0, 0)
    assert hits[0].sum() == 75 and hits[1].sum() == hits[2].sum() == 113 and (cube[0] == 0).all()      # (pair 0 is left out NOW: its plane is +0)
    if kind == "int":
        assert np.array_equal(cube, np.rint(cube)) and cube.max() > 49
    rot = rng.integers(0, nbin, (npair, nfine))
    rot[:, 0], rot[:, -1] = nbin - 1, 0
    fo.set_rotations(rot)
    for nfscr in _group_sizes(nfine):
        for normalise in (0, 1):
            got, _ = fo.check(nfscr, normalise, 0)
            assert np.isfinite(got).all() and not np.signbit(got[got == 0]).any()
    assert _info() == (113, 113)
    fo.check(nfine, 1, 1)
    assert _info() == (113, 0)
    got, hits = fo.check(1, 1, 0)
    assert (got.view(np.uint32) == 0).all() and (hits == 0).all()
    fo.close()


# ---------------------------------------------------------------- bit identity
@pytest.mark.parametrize("nprod", [1, 4])
def test_bit_identical_across_splits_reset_and_concurrent_kernels(nprod):
    """30 windows of float data: one call of 30, three of 10 and thirty of 1 (each after a Reset) give the same cube and hits
    bit for bit, and so does a fresh context run while X-engine contractions and xengBeamformRun are in flight."""
    npair, nfine, nwin, nbin, total = 3, 515, 30, 16, 30
    rng = np.random.default_rng(7 + nprod)
    x = _data(rng, "float", total, npair, nfine, nprod)
    osc = [_period_osc(5.3, 0.2, 1 << 44), _period_osc(37, 0.6), _period_osc(1000.7, 0.1, -(1 << 50))]
    fo = FO(npair, nfine, nwin, nbin, nprod)
    fo.set_rotations(None)
    fo.set_phase(osc, 0)
    fo.stream(x, [30])
    a, ahits = fo.check(1, 0, 0)
    outs = []
    for step in (10, 1):
        ffi.call("xengFoldReset")
        fo.ref.reset()
        assert _info() == (0, 0)
        fo.stream(x, [step] * (total // step))
        outs.append(fo.check(1, 0, 0))
    fo.close()
    # a fresh context beside other work: contractions on their own stream, the beamformer on this one
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    fo = FO(npair, nfine, nwin, nbin, nprod, mirror=False)
    fo.set_rotations(None)
    fo.set_phase(osc, 0)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        for k in range(3):
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            fo.enqueue(x[10 * k:10 * k + 10])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
        outs.append(fo.dump(1, 0, 0))
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    fo.close()
    ffi.call("xengBeamformDestroy")
    for o, h in outs:
        assert np.array_equal(a.view(np.uint32), o.view(np.uint32)) and np.array_equal(ahits, h)
    assert np.isfinite(a).all() and np.abs(a).max() > 0


# ---------------------------------------------------------------- the dump
@pytest.mark.parametrize("nprod", [1, 4])
def test_dump_nan_and_inf_stay_in_their_channel_and_out_of_zero_weight_channels(nprod):
    """NaN and Inf in channels of weight 0 reach no output (bit for bit the dump of clean data); in an ordinary channel they
    reach the outputs of that channel's group only, whatever the rotation."""
    npair, nfine, nwin, nbin, nfscr, total = 2, 40, 16, 7, 8, 48
    rng = np.random.default_rng(17 + nprod)
    x = _data(rng, "float", total, npair, nfine, nprod)
    w = np.ones(nfine, np.float32)
    off = np.array([3, 8, 21, 39])
    w[off] = 0
    osc = [_period_osc(5.3, 0.1), _period_osc(9.1, 0.7)]
    rot = rng.integers(0, nbin, (npair, nfine))
    outs = []
    for dirty in (False, True, "own group"):
        v = x.copy()
        if dirty:
            v[:, :, off[:2]] = np.nan
            v[::3, :, off[2], 0] = np.inf
            v[1::3, :, off[3], 1] = -np.inf
        if dirty == "own group":
            v[5, 0, 17, 0] = np.nan                     # channel 17 is in group 2 of pair 0
            v[9, 1, 30, 1 if nprod == 4 else 0] = np.inf
        fo = FO(npair, nfine, nwin, nbin, nprod)
        fo.set_rotations(rot)
        fo.set_weights(w)
        fo.set_phase(osc, 0)
        fo.stream(v, [nwin] * (total // nwin))
        outs.append([fo.check(nfscr, normalise, 0)[0] for normalise in (0, 1)])
        fo.close()
    for clean, dirty, own in zip(*outs):
        assert np.isfinite(clean).all() and np.array_equal(clean.view(np.uint32), dirty.view(np.uint32))
        bad = ~np.isfinite(own)
        assert bad[0, :, 2].any() and bad[1, :, 3].any()
        bad[0, :, 2] = False
        bad[1, :, 3] = False
        assert not bad.any()
        same = np.ones(own.shape, bool)
        same[0, :, 2] = same[1, :, 3] = False
        assert np.array_equal(own.view(np.uint32)[same], clean.view(np.uint32)[same])


@pytest.mark.parametrize("nprod", [1, 4])
def test_dump_with_weights_is_within_the_a_priori_bound(nprod):
    """Weights in [0.5, 1.5] (and two zeros), float data, nfscr in {1, 8, nfine}, both normalisations: per output
    |got - ref| <= (nfscr + 2) * 2^-24 * sum_q |w x|, with x the fp32 term the contract names (the profile word, divided by the
    hits in fp32 when normalising) and ref the float64 sum of w*x -- nfscr roundings of the chain, as DESIGN.md 4.16 has it.  The
    restatement, whose fmaf is correctly rounded, is met bit for bit as well."""
    npair, nfine, nwin, nbin, total = 3, 40, 30, 7, 90
    rng = np.random.default_rng(27 + nprod)
    x = _data(rng, "float", total, npair, nfine, nprod)
    w = rng.uniform(0.5, 1.5, nfine).astype(np.float32)
    w[[4, 33]] = 0
    fo = FO(npair, nfine, nwin, nbin, nprod)
    rot = rng.integers(0, nbin, (npair, nfine))
    fo.set_rotations(rot)
    fo.set_weights(w)
    fo.set_phase([_period_osc(5.3, 0.3), _period_osc(37, 0.2), _period_osc(1000.7, 0.9)], 0)
    fo.stream(x, [30, 30, 30])
    b = np.arange(nbin)
    for nfscr in (1, 8, nfine):
        for normalise in (0, 1):
            got, hits = fo.check(nfscr, normalise, 0)
            ref = np.zeros(got.shape)
            scale = np.zeros(got.shape)
            for p in range(npair):
                for q in range(nfine):
                    rows = (b + rot[p, q]) % nbin
                    t = fo.ref.prof[p, rows, q, :].T
                    if normalise:
                        h = hits[p, rows].astype(np.float32)
                        with np.errstate(divide='ignore', invalid='ignore'):
                            t = np.where(h > 0, t / h, np.float32(0)).astype(np.float32)
                    ref[p, :, q // nfscr] += float(w[q]) * t.astype(np.float64)
                    scale[p, :, q // nfscr] += np.abs(float(w[q]) * t.astype(np.float64))
            err = np.abs(got.astype(np.float64) - ref)
            bound = (nfscr + 2) * EPS * scale
            print("fold dump nprod=%d nfscr=%d normalise=%d: worst |err| / bound = %.3g" % (nprod, nfscr, normalise, (err[bound > 0] / bound[bound > 0]).max()))
            assert (err <= bound).all()
    fo.close()


# ---------------------------------------------------------------- an injected pulsar
def test_injected_pulsar_is_recovered_exactly():
    """Integer background bg in XX; in channel q, amp more at every window whose bin is (b0 + rot[q]) mod nbin, with rot from
    fold_rotations at a DM that spreads the band over more than one turn.  The dedispersed profile (nfscr = nfine, not
    normalised) holds exactly sum_q hits * (bg + amp) in bin b0 and sum_q hits * bg elsewhere, hits taken at the rotated bin;
    profile_snr finds b0.  Without the rotations the pulse is smeared: no bin reaches half of that."""
    npair, nfine, nwin, nbin, total, bg, amp, b0 = 2, 130, 30, 64, 600, 3, 40, 11
    bw = 23925.78125
    freqs = 40e6 + bw / 32 * np.arange(nfine)
    period = 37.3                                               # windows per turn
    f_spin = 1.0 / (period * 0.04)                              # Hz, with windows of 40 ms
    rot = np.array([fold_rotations(freqs, 200.0, f_spin, nbin), fold_rotations(freqs, 350.0, f_spin, nbin)])
    span = 4.148808e3 * 200.0 * ((freqs[0] * 1e-6) ** -2 - (freqs[-1] * 1e-6) ** -2) * f_spin
    assert span > 1.0 and len(set(rot[0].tolist())) == nbin, "the band spans %.2f turns" % span
    fo = FO(npair, nfine, nwin, nbin, 1)
    osc = [_period_osc(period, 0.123, 1 << 38), _period_osc(period, 0.6)]
    fo.set_phase(osc, 0)
    fo.set_rotations(rot)
    x = np.zeros((total, npair, nfine, 4), np.float32)
    x[..., 0] = bg
    for n0 in range(0, total, nwin):
        bins = fo.ref.bins(nwin)                                # [npair][nwin]: the restatement's oscillator (Python ints)
        for p in range(npair):
            on = bins[p][:, None] == (b0 + rot[p][None, :]) % nbin
            x[n0:n0 + nwin, p, :, 0] += amp * on
        fo.enqueue(x[n0:n0 + nwin])
    got, hits = fo.check(nfine, 0, 0)
    assert hits.sum() == npair * total
    for p in range(npair):
        rows = (np.arange(nbin)[:, None] + rot[p][None, :]) % nbin          # [b][q]
        h = hits[p][rows].astype(np.int64)
        exp = h.sum(axis=1) * bg
        exp[b0] += h[b0].sum() * amp
        assert np.array_equal(got[p, 0, 0].astype(np.int64), exp) and exp.max() < 2 ** 24
        s = profile_snr(got[p, 0, 0])
        assert s['bin'] == b0 and s['peak'] == exp[b0] and s['snr'] > 20
    fo.set_rotations(None)
    (smeared, _), _ = fo.dump(nfine, 0, 1)
    assert ((smeared[:, 0, 0] - smeared[:, 0, 0].min(axis=1, keepdims=True)).max(axis=1) < 0.5 * amp * total / nbin * nfine).all()
    fo.close()


# ---------------------------------------------------------------- what needs a context
def test_argument_checks_with_a_context():
    """Run before SetPhase and Dump before SetRotations: INVALID_STATE.  nwin_call outside 1..nwin, misaligned pointers, n_ref
    out of range, a rotation outside [0, nbin), a non-finite weight, nfscr not dividing nfine: INVALID_ARGUMENT, nothing
    launched and the state unchanged."""
    fo = FO(2, 16, 4, 8, 1)
    x = np.ones((4, 2, 16, 4), np.float32)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengFoldRun", fo.din.ptr, 4)
    assert ei.value.status == INVALID_STATE
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengFoldDump", fo.dout.ptr + GUARD, None, 1, 0, 0)
    assert ei.value.status == INVALID_STATE
    osc = [_period_osc(8, 0.01), _period_osc(8, 0.51)]
    for n_ref in (-1, 1):
        with pytest.raises(ffi.XengError) as ei:
            fo.set_phase(osc, n_ref)
        assert ei.value.status == INVALID_ARGUMENT
    fo.set_phase(osc, 0)
    for bad in (-1, 8):
        r = np.zeros((2, 16), np.int32)
        r[1, 5] = bad
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFoldSetRotations", r.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengFoldDump", fo.dout.ptr + GUARD, None, 1, 0, 0)
    assert ei.value.status == INVALID_STATE                     # (a refused table is no table)
    fo.set_rotations(None)
    for v in (np.nan, np.inf):
        w = np.ones(16, np.float32)
        w[3] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFoldSetWeights", w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((fo.din.ptr, 0), (fo.din.ptr, 5), (fo.din.ptr + 4, 1)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFoldRun", *args)
        assert ei.value.status == INVALID_ARGUMENT and _info() == (0, 0)
    for args in ((fo.dout.ptr + GUARD + 8, None, 1, 0, 0), (fo.dout.ptr + GUARD, None, 3, 0, 0), (fo.dout.ptr + GUARD, None, 0, 0, 0),
                 (fo.dout.ptr + GUARD, None, 32, 0, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFoldDump", *args)
        assert ei.value.status == INVALID_ARGUMENT
    fo.enqueue(x)
    assert _info() == (4, 4)
    got, hits = fo.check(16, 0, 0)          # (period 8: windows 0..3 fall in bins 0..3 of pair 0 and 4..7 of pair 1, 16 channels of I = 2)
    assert hits.tolist() == [[1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 1, 1]] and np.array_equal(got[:, 0, 0], 32.0 * hits)
    fo.set_phase(osc, 4)                    # (n_ref = the count is allowed; one past it is not)
    with pytest.raises(ffi.XengError) as ei:
        fo.set_phase(osc, 5)
    assert ei.value.status == INVALID_ARGUMENT
    t = ctypes.c_ulonglong()
    ffi.call("xengFoldMark", ctypes.byref(t))
    ffi.call("xengFoldWait", t.value)
    done = ctypes.c_int()
    ffi.call("xengFoldTicketDone", t.value, ctypes.byref(done))
    assert done.value == 1
    fo.close()


# ---------------------------------------------------------------- the block at the end of the live chain, on device rings
PULSARS = [dict(f0=3.1, f1=-1e-6, pepoch=0.25, dm=0.4), dict(f0=11.7, f1=0.0, pepoch=0.0, dm=0.05)]


def _chain(with_fold, vin, nchan, nstand, nbeam, g, ns, N, W, nbin, nsub, nfscr):
    """Source -> Beamform -> {BeamformSumBeams, UpchanSumBeams -> BeamFold (with_fold)} on device rings; returns the sinks'
    sequences: BeamformSumBeams' output, and UpchanSumBeams' and BeamFold's (or None)."""
    ninput = 2 * nstand
    rng = np.random.default_rng(0x5eed)
    r0, r1, r2 = Ring("gpu-input", space="cuda"), Ring("bf-output", space="cuda"), Ring("bf-pow-output", space="cuda_host")
    bf = Beamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, gpu=0)
    sb = BeamformSumBeams(LOG, r1, r2, nchan=nchan, ntime_gulp=g, ntime_sum=ns, gpu=0)
    sfreq, bw = 40e6, 23925.78125
    bf.freqs = sfreq + bw * np.arange(nchan)
    bf.process_command_strings(_beam_cmds(nchan, nbeam, ninput, rng)[0])
    blocks, sinks = [bf, sb], [Sink(r2, (nbeam // 2) * (g // ns) * nchan * 16)]
    if with_fold:
        nwin, npair, nfine = g // N // W, nbeam // 2, nchan * N
        r3, r4 = Ring("ub-output", space="cuda"), Ring("fold-output", space="cuda_host")
        blocks.append(UpchanSumBeams(LOG, r1, r3, nchan=nchan, nbeam=nbeam, ntime_gulp=g, nupchan=N, nframe_sum=W, gpu=0))
        blocks.append(BeamFold(LOG, r3, r4, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nbin=nbin, pulsars=PULSARS, nsub=nsub, nfscr=nfscr, gpu=0))
        sinks += [Sink(r3, nwin * npair * nfine * 16), Sink(r4, npair * (nfine // nfscr) * nbin * 4)]
    run_blocks(blocks, Source(r0, [(source_header(nchan, nstand, 2, sfreq=sfreq, chan_bw=bw), vin, g * nchan * ninput)]), sinks)
    return [s.sequences for s in sinks] + ([None, None] if not with_fold else [])


def test_block_after_upchan_sum_beams_on_device_rings():
    """8 gulps through Beamform and UpchanSumBeams (3 windows of 2 frames per gulp) into BeamFold, 2 pairs, 16 bins, nsub = 2:
    each of the 4 sub-integrations equals, bit for bit, the restatement applied to the spans UpchanSumBeams wrote, driven with
    fold_phase at each span's own time and fold_rotations at the header's frequencies; BeamformSumBeams' output beside it is
    bit for bit what it is without the two readers."""
    nchan, nstand, nbeam, g, ns, N, W, ngulp, nbin, nsub, nfscr = 4, 32, 4, 96, 24, 16, 2, 8, 16, 2, 16
    nwin, npair, nfine = g // N // W, nbeam // 2, nchan * N
    vin = np.random.default_rng(0xc0ffee).integers(0, 256, (ngulp * g, nchan, 2 * nstand), dtype=np.uint8)
    pow_with, ub, fold = _chain(True, vin, nchan, nstand, nbeam, g, ns, N, W, nbin, nsub, nfscr)
    pow_without, _, _ = _chain(False, vin, nchan, nstand, nbeam, g, ns, N, W, nbin, nsub, nfscr)
    (uh, _, usp), = ub
    assert len(usp) == ngulp and len(fold) == ngulp // nsub
    x = np.concatenate([s.view(np.float32).reshape(nwin, npair, nfine, 4) for s in usp])
    exp = _subints(uh, x, range(ngulp), nchan, N, W, nwin, nbin, 1, nsub, nfscr, True, PULSARS)
    shape = (npair, 1, nfine // nfscr, nbin)
    for (hd, tag, spans), (start, out, hits) in zip(fold, exp):
        assert tag == start == hd['subint_start'] and len(spans) == 1 and hd['hits'] == hits.tolist() and hits.sum() == npair * nsub * nwin
        assert (hd['nbin'], hd['nfscr'], hd['nprod'], hd['nsub'], hd['tsamp']) == (nbin, nfscr, 1, nsub, W * N * nchan / uh['bw_hz'])
        got = spans[0].view(np.float32).reshape(shape)
        assert np.array_equal(got.view(np.uint32), out.view(np.uint32)) and np.abs(got).max() > 0
    (_, _, a), = pow_with
    (_, _, b), = pow_without
    assert len(a) == len(b) == ngulp and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
