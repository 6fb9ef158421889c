"""xengFlag* and UpchanFlag on the GPU (include/xeng.h, "Outlier flags from the fine-channel visibilities"; csrc/flag_kernels.h).

1. R and A against the float64 restatement (tests/flag_ref.py), per (channel, pol) as max_s |x - ref| / rms_s ref, within five times
   the gap of the float32 restatement (the contract's sum taken term by term in float32) to float64 on the test's own inputs; A, a
   copy of an input word, exact.  Measured on the MI355X, worst error / bar: see MEASURED.
2. mask and chan equal the float32 restatement of steps 2 and 3 applied to the device's own stats table, bit for bit, for every
   combination of the controls.
3. Injections are found: the expected mask is written down from the injections (tests/test_flag_cpu.py detection_case).
4. stats and the bits 0, 1, 3, 4 do not change by a bit with a channel subset, a fresh context, other kernels beside, the upper
   triangle and the cross hands overwritten with NaN, a SetControl back and forth.
5. A NaN in a word that is read sets bit 3 on its two stands in its (channel, pol) and changes nothing else.
6. The ABI: sizes, guards, tickets, every rejection of the header, with and without a context.
7. TbfSource -> Copy -> UpchanCorr -> UpchanFlag on device rings; flags() -> flag_factors -> UpchanCalApply.set_factors."""
import ctypes
import json
import os
import struct
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Copy, TbfSource, UpchanCalApply, UpchanCorr, UpchanFlag, flag_factors  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import flag_ref as fr  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.image_ref import random_array  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_flag_cpu import detection_case  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
SHAPES = [(22, 3), (35, 2), (64, 2), (70, 5)]       # (nstand, nfine): one ragged tile; two; two full ones; three, the last ragged
# worst error of R / bar per shape, measured on the MI355X (the emulated kernels give the same words: tests/test_flag_emul_cpu.py)
MEASURED = {22: 0.20, 35: 0.25, 64: 0.20, 70: 0.17}


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _info():
    m, s, c, l = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
    ffi.call("xengFlagGetInfo", ctypes.byref(m), ctypes.byref(s), ctypes.byref(c), ctypes.byref(l))
    return m.value, s.value, c.value, l.value


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


class FL:
    """The xengFlag context (one per process), an input buffer and the three outputs of one call, each between poisoned guard bands."""

    def __init__(self, nstand, nfine, w=None, control=None):
        self.nstand, self.nfine = nstand, nfine
        ffi.call("xengFlagInitialize", 0, nstand, nfine)
        if w is not None:
            self.set_weights(w)
        if control is not None:
            self.set_control(*control)
        n = nfine * 2 * nstand
        self.sizes = (n, 8 * n, 32 * nfine)
        self.offs = [GUARD, 2 * GUARD + ((n + 15) & ~15)]
        self.offs.append(self.offs[1] + 8 * n + GUARD)
        self.din = ffi.DeviceBuffer(nfine * (2 * nstand) ** 2 * 8)
        self.dout = ffi.DeviceBuffer(self.offs[2] + 32 * nfine + GUARD)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)

    def set_weights(self, w):
        ffi.call("xengFlagSetWeights", _fp(np.ascontiguousarray(w, np.float32)))

    def set_control(self, a, b, c, wchan):
        ffi.call("xengFlagSetControl", float(a), float(b), float(c), int(wchan))

    def upload(self, V):
        assert V.shape == (self.nfine, self.nstand, 2, self.nstand, 2) and V.dtype == np.complex64
        self.din.upload(np.ascontiguousarray(V))

    def enqueue(self):
        ffi.call("xengFlagRun", self.din.ptr, *[self.dout.ptr + o for o in self.offs])

    def result(self):
        """After a sync: (mask, stats, chan) (the poison is put back); every byte between and around them must still be poison."""
        raw = self.dout.download(np.uint8)
        keep = np.zeros(raw.size, bool)
        for o, n in zip(self.offs, self.sizes):
            keep[o:o + n] = True
        assert (raw[~keep] == POISON).all(), "bytes outside the outputs were written"
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        m, s, c = (raw[o:o + n].copy() for o, n in zip(self.offs, self.sizes))
        return m.reshape(self.nfine, 2, self.nstand), s.view(np.float32).reshape(self.nfine, 2, self.nstand, 2), c.view(np.float32).reshape(self.nfine, 2, 4)

    def run(self, V):
        self.upload(V)
        self.enqueue()
        ffi.call("xengFlagSync")
        return self.result()

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengFlagCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengFlagDestroy")
        self.din.free()
        self.dout.free()


def _case(nstand, nfine, seed=None):
    """A case with stand 3 of weight 0 and full of non-finite words, the upper triangle and the cross hands NaN, stand 7 eight times
    too loud in channel 1: (the clean V, what the device gets, w)"""
    V = fr.case(nstand, nfine, seed)
    fr.scale_stand(V, 1, 7, 8)
    w = np.ones(nstand, np.float32)
    w[3] = 0
    bad = fr.upper_and_cross_nan(V)
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    return V, bad, w


# ---------------------------------------------------------------- 1. the statistics
@pytest.mark.parametrize("nstand,nfine", SHAPES)
def test_statistics_against_the_float64_restatement(nstand, nfine):
    """R within five float gaps of the float64 restatement per (channel, pol), A exact, +0 for both at the stand of weight 0; the
    words are those of the restatement in the kernel's summation order, bit for bit; mask and chan follow from the device's table.
    Measured on the MI355X, worst error / bar: 0.20 (22 stands), 0.25 (35), 0.20 (64), 0.17 (70)."""
    V, bad, w = _case(nstand, nfine)
    fl = FL(nstand, nfine, w)
    mask, stats, chan = fl.run(bad)
    fl.close()
    ref = fr.statistics(V, w)
    gap = fr.float_gap(V, w, ref)
    err = fr.stat_error(stats[..., 0], ref[0], w)
    print("%d stands: R's float32 gap %.2e, device %.2e, worst error / bar %.2f" % (nstand, gap[0].max(), err.max(), (err / (5 * gap[0])).max()))
    assert np.isfinite(stats).all() and (err <= 5 * gap[0]).all()
    assert _same(stats[..., 1], ref[1].astype(np.float32)) and (stats[:, :, 3].view(np.uint32) == 0).all()
    R, _ = fr.statistics_kernel_order(V, w)
    assert _same(stats[..., 0], R)
    emask, echan = fr.flags(stats, w, *fr.thresholds(), 0)
    assert _same(mask, emask) and _same(chan, echan)
    assert (mask[1, :, 7] & 3 == 3).all() and (mask[:, :, 3] & 16 == 16).all()


# ---------------------------------------------------------------- 2. exact flags
CONTROLS = [(6, 6, 6, 0), (0, 6, 6, 0), (6, 0, 6, 0), (6, 6, 0, 0), (0, 0, 0, 0), (6, 6, 6, 1), (6, 6, 6, 3), (2, 1.5, 1, 3), (1, 1, 1, 0), (3, 3, 2.5, 1)]


def test_mask_and_chan_are_the_restatement_on_the_device_table_for_every_control():
    """35 stands, 12 channels: stand 7 loud in channel 1, channel 4 loud, stand 11's autos low, (9, pol 1) without a y (NaN words leave
    3 finite stands), two stands that share every word (ties).  For each control combination -- the defaults, each test off, all off,
    wchan 0, 1, 3, thresholds low enough to flag many cells -- mask and chan are the float32 restatement on the device's own table."""
    nstand, nfine = 35, 12
    V, bad, w = _case(nstand, nfine, seed=5)
    for X in (V, bad):
        fr.scale_channel(X, 4, 5)
        fr.scale_auto(X, 11, 0.01)
        X[:, 21] = X[:, 20]
        X[:, :, :, 21] = X[:, :, :, 20]
    bad[9, 6:, 1, 0, 1] = np.nan                # stand 0 and every stand from 6 on; 3 has weight 0
    bad[9, 5, 1, 4, 1] = np.nan                 # 5 and 4: 1 and 2 stay
    fl = FL(nstand, nfine, w)
    seen = set()
    for control in CONTROLS:
        fl.set_control(*control)
        mask, stats, chan = fl.run(bad)
        emask, echan = fr.flags(stats, w, *fr.thresholds(*control[:3]), control[3])
        assert _same(mask, emask) and _same(chan, echan), control
        assert chan[9, 1, 3] == 2 and (mask[9, 1] & 4 == 4).all()
        seen.add(mask.tobytes())
    fl.close()
    assert len(seen) >= 6                       # (the controls do change the mask)


# ---------------------------------------------------------------- 3. detection
def test_injections_are_found():
    """tests/test_flag_cpu.py detection_case: 70 stands, 12 channels, the five injections; the expected mask is written down there.
    First, on the CPU restatement, every d of every test taken is at least 1 % away from its threshold, so that no cell is marginal;
    then the device's mask is the expected one, every cell of it."""
    V, w, expect = detection_case()
    detail = []
    fr.flags(np.stack(fr.statistics_kernel_order(V, w), axis=-1), w, *fr.thresholds(), 0, detail)
    print("detection: the nearest d is %.3f of its threshold away from it" % fr.margin(detail))
    assert fr.margin(detail) >= 0.01
    fl = FL(expect.shape[2], expect.shape[0], w)
    mask, stats, chan = fl.run(V)
    fl.close()
    assert np.array_equal(mask, expect)


# ---------------------------------------------------------------- 4. bit identity
def test_a_channel_subset_fresh_context_other_kernels_nan_elsewhere_and_controls_change_no_bit():
    """35 stands, 3 channels.  stats and the bits 0, 1, 3, 4 of the full run are those of: the middle channel alone in a context of its
    own; a fresh context; the input with the upper triangle and all cross hands NaN; a run after SetControl to other values and
    back (all of the mask then); a fresh context while X-engine contractions run on their streams and xengBeamformRun on this one."""
    nstand, nfine = 35, 3
    V, bad, w = _case(nstand, nfine, seed=41)
    clean = V.copy()
    clean[:, 3] = 0
    clean[:, :, :, 3] = 0
    fl = FL(nstand, nfine, w)
    mask, stats, chan = fl.run(clean)
    m2, s2, c2 = fl.run(bad)
    fl.set_control(1, 1, 1, 1)
    m3, s3, _ = fl.run(clean)
    fl.set_control(6, 6, 6, 0)
    m4, s4, c4 = fl.run(clean)
    fl.close()
    assert _same(s2, stats) and _same(m2, mask) and _same(c2, chan)
    assert _same(s3, stats) and not _same(m3, mask) and _same(s4, stats) and _same(m4, mask) and _same(c4, chan)
    fl = FL(nstand, 1, w)
    m1, s1, _ = fl.run(np.ascontiguousarray(clean[1:2]))
    fl.close()
    assert _same(s1, stats[1:2]) and _same(m1 & 0x1b, mask[1:2] & 0x1b)
    bstand, bchan, btime, nbeam = 96, 8, 96, 4
    rng = np.random.default_rng(3)
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, bstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * bstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * bstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    fl = FL(nstand, nfine, w)
    fl.upload(clean)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        got = []
        for k in range(3):
            for q in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + q * xg.gulp_bytes, xg.out.ptr, int(q == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            fl.enqueue()
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengFlagSync")
            got.append(fl.result())
        ffi.call("xengXgpuSync")
    finally:
        xg.close()
    fl.close()
    ffi.call("xengBeamformDestroy")
    assert all(_same(m, mask) and _same(s, stats) and _same(c, chan) for m, s, c in got)


# ---------------------------------------------------------------- 5. non-finite visibilities
def test_a_nan_word_marks_its_two_stands_in_its_channel_and_pol_only():
    """A NaN in V[1][20 1][9 1] (a word of the lower triangle, between two tiles) and an Inf in V[2][5 0][5 0] (an auto): bit 3 on the
    stands 20 and 9 of (1, pol 1) and on stand 5 of (2, pol 0), their R (or A) non-finite; every other word of stats is that of the
    clean run, as is every other cell of the bits 0, 1, 3, 4 whose (channel, pol) was not touched; the cells that share a (channel,
    pol) with a non-finite stand, and bit 2 and chan everywhere, are the restatement's on the device's own table (the median moves
    when a stand leaves).  A NaN above the diagonal and one in a cross hand change nothing at all."""
    nstand, nfine = 35, 4
    V = fr.case(nstand, nfine, seed=61)
    w = np.ones(nstand, np.float32)
    bad, other = V.copy(), V.copy()
    bad[1, 20, 1, 9, 1] = np.nan
    bad[2, 5, 0, 5, 0] = np.inf
    other[1, 9, 1, 20, 1] = np.nan
    other[1, 20, 1, 9, 0] = np.nan
    fl = FL(nstand, nfine, w)
    (m0, s0, c0), (m1, s1, c1), (m2, s2, c2) = fl.run(V), fl.run(bad), fl.run(other)
    fl.close()
    assert _same(m2, m0) and _same(s2, s0) and _same(c2, c0) and np.isfinite(s0).all() and not (m0 & 8).any()
    hit = np.zeros(s0.shape, bool)
    hit[1, 1, [20, 9], 0] = True
    hit[2, 0, 5, 1] = True
    assert not np.isfinite(s1[hit]).any() and _same(s1[~hit], s0[~hit])
    b3 = np.zeros(m0.shape, bool)
    b3[1, 1, [20, 9]] = b3[2, 0, 5] = True
    assert np.array_equal((m1 & 8) != 0, b3)
    touched = np.zeros(m0.shape, bool)
    touched[1, 1] = touched[2, 0] = True
    assert _same((m1 & 0x1b)[~touched], (m0 & 0x1b)[~touched])
    emask, echan = fr.flags(s1, w, *fr.thresholds(), 0)
    assert _same(m1, emask) and _same(c1, echan)
    assert _same(c1[[0, 3]][:, :, [0, 1, 3]], c0[[0, 3]][:, :, [0, 1, 3]]) and c1[1, 1, 3] == nstand - 2 and c1[2, 0, 3] == nstand - 1


# ---------------------------------------------------------------- 6. the ABI
def test_info_tickets_and_argument_checks_with_and_without_a_context():
    """GetInfo's sizes; SetWeights refuses NULL, a negative or non-finite weight and weights that leave 3 stands; SetControl a
    negative or non-finite nsig and a wchan outside [0, 64]; they change nothing; tickets count from 1 after Initialize and every one
    is done after Sync; every INVALID_ARGUMENT of Initialize leaves a live context alone; Run refuses NULL and misaligned pointers
    and writes nothing; after Destroy every call that needs a context is INVALID_STATE."""
    nstand, nfine = 38, 2
    V, bad, w = _case(nstand, nfine, seed=81)
    fl = FL(nstand, nfine, w)
    n = nfine * 2 * nstand
    assert _info() == (n, 8 * n, 32 * nfine, 8192 * 5 + 8)
    a, b, c, wc = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int(-1)
    ffi.call("xengFlagGetControl", ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(wc))
    assert (a.value, b.value, c.value, wc.value) == (6.0, 6.0, 6.0, 0)
    first = fl.run(bad)
    for bw in (np.where(np.arange(nstand) == 2, np.nan, w), np.where(np.arange(nstand) == 7, -1, w), np.where(np.arange(nstand) == 7, np.inf, w),
               np.where(np.arange(nstand) < 3, 1, 0)):
        with pytest.raises(ffi.XengError) as ei:
            fl.set_weights(bw)
        assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengFlagSetWeights", None)
    assert ei.value.status == INVALID_ARGUMENT
    for bc in ((-1, 6, 6, 0), (6, np.nan, 6, 0), (6, 6, np.inf, 0), (6, 6, 1e39, 0), (6, 6, 6, -1), (6, 6, 6, 65)):
        with pytest.raises(ffi.XengError) as ei:
            fl.set_control(*bc)
        assert ei.value.status == INVALID_ARGUMENT, bc
    assert all(_same(x, y) for x, y in zip(fl.run(bad), first))
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    ffi.call("xengFlagMark", ctypes.byref(t))
    assert t.value == 1
    fl.enqueue()
    ffi.call("xengFlagMark", ctypes.byref(t))
    assert t.value == 2
    ffi.call("xengFlagWait", 2)
    ffi.call("xengFlagSync")
    fl.result()
    for k in (1, 2):
        ffi.call("xengFlagTicketDone", k, ctypes.byref(d))
        assert d.value == 1
    for k in (0, 3):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFlagWait", k)
        assert ei.value.status == INVALID_ARGUMENT
    for args in ((0, 0, nfine), (0, 3, nfine), (0, 513, nfine), (0, nstand, 0), (0, nstand, 8193)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFlagInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    assert _info()[0] == n
    o = [fl.dout.ptr + x for x in fl.offs]
    for args in ((None, o[0], o[1], o[2]), (fl.din.ptr, None, o[1], o[2]), (fl.din.ptr, o[0], None, o[2]), (fl.din.ptr, o[0], o[1], None),
                 (fl.din.ptr + 8, o[0], o[1], o[2]), (fl.din.ptr, o[0], o[1] + 2, o[2]), (fl.din.ptr, o[0], o[1], o[2] + 1)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengFlagRun", *args)
        assert ei.value.status == INVALID_ARGUMENT
    s = ctypes.c_int()
    ll = ctypes.c_longlong()
    for name, args in (("xengFlagGetInfo", (None, ctypes.byref(ll), ctypes.byref(ll), ctypes.byref(s))), ("xengFlagCheckGuards", (None,)),
                       ("xengFlagGetControl", (ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None)), ("xengFlagMark", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, name
    ffi.call("xengFlagSync")
    fl.result()                                 # (nothing was written)
    fl.close()
    for name, args in (("xengFlagRun", (4096, 4096, 4096, 4096)), ("xengFlagSetWeights", (_fp(w),)), ("xengFlagSetControl", (6.0, 6.0, 6.0, 0)),
                       ("xengFlagGetControl", (ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(wc))),
                       ("xengFlagGetInfo", (ctypes.byref(ll), ctypes.byref(ll), ctypes.byref(ll), ctypes.byref(s))),
                       ("xengFlagMark", (ctypes.byref(t),)), ("xengFlagWait", (1,)), ("xengFlagTicketDone", (1, ctypes.byref(d))), ("xengFlagSync", ()),
                       ("xengFlagCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    for name, args in (("xengFlagSetWeights", (None,)), ("xengFlagSetControl", (-1.0, 6.0, 6.0, 0)), ("xengFlagRun", (None, 4096, 4096, 4096))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, name
    ffi.call("xengFlagDestroy")


# ---------------------------------------------------------------- 7. the chain on device rings
def _vis(span, nfine, nstand):
    return np.ascontiguousarray(span).view(np.uint8).reshape(-1).view(np.complex64).reshape(nfine, nstand, 2, nstand, 2)


def test_tbf_file_to_upchan_corr_to_upchan_flag_and_its_mask_into_upchan_calapply(tmp_path):
    """TbfSource (host ring) -> Copy (device ring) -> UpchanCorr (44 inputs, 2 coarse channels, nupchan 2) -> UpchanFlag on device
    rings, two integrations of four gulps each, input (stand 5, pol 0) dead: every flag span is the restatement on its own stats table, which is that of
    UpchanCorr's span in the kernel's order, bit for bit; the dead input is an auto outlier in every channel; flags() is the last
    span.  Then flags() -> flag_factors -> UpchanCalApply.set_factors on UpchanCorr's spans: the rows and columns of every flagged
    (channel, pol, stand) are +0 and every other word is that of the run without flags, bit for bit."""
    nstand, nchan, g, N, seq0, nint, ngulp = 22, 2, 64, 2, 6400, 2, 4
    ninput, nfine = 2 * nstand, nchan * N
    rng = np.random.default_rng(91)
    vin = rng.integers(0, 256, (nint * ngulp * g, nchan, ninput), dtype=np.uint8)
    vin[:, :, 2 * 5] = 0            # (256 samples per fine channel and integration: the autos scatter by 6 %, a dead input stands out)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=55e6)
    hdr['seq'] = seq0
    path = os.path.join(str(tmp_path), "lwa-dump-1.00.tbf.0")
    hjson = json.dumps(hdr).encode()
    with open(path, "wb") as fh:
        assert len(hjson) <= 1024 - 8
        fh.write(struct.pack('<II', len(hjson), 1024) + hjson)
        fh.write(b"\0" * (1024 - 8 - len(hjson)))
        fh.write(vin.tobytes())
    rh, rd, ru, rf = Ring("tbf", space="system"), Ring("tbf-gpu", space="cuda"), Ring("uc-output", space="cuda"), Ring("flag-output", space="cuda")
    src = TbfSource(LOG, rh, [path], ntime_gulp=g)
    cp = Copy(LOG, rh, rd, ntime_gulp=g, nbyte_per_time=nchan * ninput)
    uc = UpchanCorr(LOG, rd, ru, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=ngulp * g // N, gpu=0)
    fl = UpchanFlag(LOG, ru, rf, nstand, gpu=0)
    span = nfine * ninput * ninput * 8
    stats_offset, chan_offset, ospan = fl.layout(nfine)
    mid, out = Sink(ru, span), Sink(rf, ospan)
    ths = [threading.Thread(target=b.main, daemon=True) for b in (src, cp, uc, fl)]
    for s in (mid, out):
        s.start()
    for t in ths[::-1]:
        t.start()
    for t in ths + [mid, out]:
        t.join(60)
        assert not t.is_alive()
    ok = ctypes.c_int()
    ffi.call("xengFlagCheckGuards", ctypes.byref(ok))
    ffi.call("xengFlagDestroy")
    ffi.call("xengUpchanCorrDestroy")
    assert ok.value == 1
    (vh, _, vspans), = mid.sequences
    (fh_, ftag, fspans), = out.sequences
    assert len(vspans) == len(fspans) == nint and ftag == fh_['seq0'] == seq0 and fl.stats['nflag'] == nint and fl.stats['ngap'] == 0
    assert fh_['flagged'] is True and (fh_['stats_offset'], fh_['chan_offset'], fh_['nfine'], fh_['wchan']) == (stats_offset, chan_offset, nfine, 0)
    w = np.ones(nstand, np.float32)
    n = nfine * 2 * nstand
    for k in range(nint):
        raw = np.ascontiguousarray(fspans[k]).view(np.uint8).reshape(-1)
        mask, stats = raw[:n].reshape(nfine, 2, nstand), raw[stats_offset:chan_offset].view(np.float32).reshape(nfine, 2, nstand, 2)
        chan = raw[chan_offset:ospan].view(np.float32).reshape(nfine, 2, 4)
        V = _vis(vspans[k], nfine, nstand)
        R, A = fr.statistics_kernel_order(V, w)
        assert _same(stats[..., 0], R) and _same(stats[..., 1], A)
        emask, echan = fr.flags(stats, w, *fr.thresholds(), 0)
        assert _same(mask, emask) and _same(chan, echan)
        assert (mask[:, 0, 5] & 2 == 2).all() and (stats[:, 0, 5] == 0).all()
    seq, fmask, fstats, fchan = fl.flags()
    assert seq == seq0 + (nint - 1) * vh['acc_len'] and _same(fmask, mask) and _same(fstats, stats) and _same(fchan, chan)
    # the mask into UpchanCalApply
    pos = random_array(rng, nstand, 1200.0, 5.0)
    h = flag_factors(np.ones((nfine, 2, nstand), np.complex64), fmask)
    outs = []
    for factors in (None, h):
        r1, r2 = Ring("uc-again", space="cuda"), Ring("calapply-output", space="cuda")
        cal = UpchanCalApply(LOG, r1, r2, pos, gpu=0)
        if factors is not None:
            cal.set_factors(factors)
        sink = Sink(r2, span)
        run_blocks([cal], Source(r1, [(vh, np.concatenate([np.ascontiguousarray(s).view(np.uint8).reshape(-1) for s in vspans]), span)]), [sink])
        ffi.call("xengCalapplyDestroy")
        (_, _, cspans), = sink.sequences
        outs.append([_vis(s, nfine, nstand) for s in cspans])
    gone = ((fmask & 0x0f) != 0).transpose(0, 2, 1).reshape(nfine, ninput)
    gone = (gone[:, :, None] | gone[:, None, :]).reshape(nfine, nstand, 2, nstand, 2)
    assert gone.any() and not gone.all()
    for plain, flagged in zip(*outs):
        assert (flagged[gone].view(np.uint32) == 0).all() and _same(flagged[~gone], plain[~gone])
