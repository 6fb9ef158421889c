"""The PFB front end of xengUpchan* / xengUpchanCorr* on the MI355X: the kernels against the float64 restatement
(tests/upchan_pfb_ref.py; the whole output and every row of it) over consecutive gulps with random asymmetric coefficients
(so that a reversed tap or sample index cannot pass), bit identity (parts, repeats, nstage, Reset, SetPfb(1, NULL), Prime),
bytes past the output untouched, the leakage of a quantised tone, the argument checks that need a context, and both blocks
on device rings with a gap and two sequences.  No wall-clock assertions."""
import ctypes
import json
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import UpchanBeamform, UpchanCorr  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.pfb import pfb_coeffs  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.pipeline_util import LOG, Sink, source_header  # noqa: E402
from tests.upchan_local_ref import check_rows  # noqa: E402
from tests.upchan_pfb_ref import pfb_fine_select, upchan_beamform_pfb, upchan_corr_pfb  # noqa: E402

POISON = 0xA5
GUARD = 4096
INVALID_ARGUMENT = 1


def _fp(h):
    return None if h is None else np.ascontiguousarray(h, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def set_pfb(name, ntap, h):
    h = None if h is None else np.ascontiguousarray(h, np.float32)
    ffi.call(name, ntap, _fp(h))


def check(got, exp):
    """Within 1e-5 of the output's RMS, and every row within 1e-5 of its own (tests/upchan_local_ref.py check_rows)."""
    rms = np.sqrt(np.mean(np.abs(exp) ** 2))
    err = np.max(np.abs(got.astype(exp.dtype) - exp))
    assert rms > 0 and err <= 1e-5 * rms, "max |err| %.3g = %.3g of RMS %.3g" % (err, err / rms, rms)
    check_rows(got, exp)


class UP:
    """The xengUpchan context (one per process: each test makes one at a time), a gulp buffer and a poisoned output."""

    def __init__(self, ninput, nchan, ntime, N, nbeam, nframe_sum=0, dual=False, ntap=None, h=None):
        self.ninput, self.nchan, self.ntime, self.N = ninput, nchan, ntime, N
        ffi.call("xengUpchanInitializeDualPol" if dual else "xengUpchanInitialize", 0, ninput, nchan, ntime, N, nbeam, nframe_sum)
        if ntap is not None:
            set_pfb("xengUpchanSetPfb", ntap, h)
        nf = ntime // N
        if dual:
            self.shape, self.dtype = (nf // nframe_sum, nbeam // 2, nchan, N, 4), np.float32
        elif nframe_sum:
            self.shape, self.dtype = (nf // nframe_sum, nbeam, nchan, N), np.float32
        else:
            self.shape, self.dtype = (nf, nbeam, nchan, N), np.complex64
        self.nout = int(np.prod(self.shape)) * np.dtype(self.dtype).itemsize
        self.din = ffi.DeviceBuffer(ntime * nchan * ninput)
        self.dw = ffi.DeviceBuffer(nchan * N * nbeam * ninput * 8)
        self.dout = ffi.DeviceBuffer(self.nout + GUARD)

    def run(self, vin, w=None, split=None):
        self.din.upload(np.ascontiguousarray(vin).reshape(-1))
        if w is not None:
            self.dw.upload(w)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.nout + GUARD)
        if split is None:
            ffi.call("xengUpchanRun", self.din.ptr, self.dout.ptr, self.dw.ptr, 1)
        else:
            ffi.call("xengUpchanRunParts", self.din.ptr, split, self.din.ptr + split * self.nchan * self.ninput, self.dout.ptr, self.dw.ptr, 1)
        ffi.call("xengUpchanSync")
        raw = self.dout.download(np.uint8)
        assert (raw[self.nout:] == POISON).all(), "bytes past the output were written"
        return raw[:self.nout].view(self.dtype).reshape(self.shape).copy()


@pytest.fixture
def up():
    yield UP
    ffi.call("xengUpchanDestroy")


def rand_w(rng, nchan, N, nbeam, ninput):
    return (rng.standard_normal((nchan, N, nbeam, ninput)) + 1j * rng.standard_normal((nchan, N, nbeam, ninput))).astype(np.complex64)


# ---------------------------------------------------------------- UpchanBeamform kernel
@pytest.mark.parametrize("N", [8, 16, 32, 64])
@pytest.mark.parametrize("P", [2, 4, 8])
def test_beamform_kernel_against_restatement(up, N, P):
    """Three consecutive gulps of 8 frames (the history carries P-1 frames across each boundary; at P = 8 nearly a whole gulp),
    random asymmetric coefficients, voltage / power / dual-pol; within 1e-5 of the output's RMS."""
    ninput, nchan, ntime = 8, 2, 8 * N
    rng = np.random.default_rng(N * 10 + P)
    stream = rng.integers(0, 256, (3 * ntime, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32)
    assert not np.array_equal(h, h[::-1])
    for nbeam, nframe_sum, dual in ((3, 0, False), (3, 4, False), (4, 2, True)):
        w = rand_w(rng, nchan, N, nbeam, ninput)
        u = up(ninput, nchan, ntime, N, nbeam, nframe_sum, dual, P, h)
        for k in range(3):
            got = u.run(stream[k * ntime:(k + 1) * ntime], w if k == 0 else None)
            check(got, upchan_beamform_pfb(stream, w, N, nbeam, h, k * ntime, ntime, nframe_sum, dual_pol=dual))


def test_beamform_bit_identity(up):
    """Whole gulps against two-part gulps (splits inside the history span and before it), repeats after Reset, Reset against a
    fresh context's first gulp, and SetPfb(1, NULL) against a context that never called SetPfb."""
    ninput, nchan, N, P, nbeam = 16, 3, 32, 4, 5
    ntime = 6 * N
    rng = np.random.default_rng(7)
    stream = rng.integers(0, 256, (3 * ntime, nchan, ninput), dtype=np.uint8)
    h = rng.standard_normal(P * N).astype(np.float32)
    w = rand_w(rng, nchan, N, nbeam, ninput)
    gulps = [stream[k * ntime:(k + 1) * ntime] for k in range(3)]
    u = up(ninput, nchan, ntime, N, nbeam, 0, False, P, h)
    whole = [u.run(g, w) for g in gulps]
    for split in (N, ntime - 2 * N, ntime - N):
        ffi.call("xengUpchanReset")
        parts = [u.run(g, split=split) for g in gulps]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, parts)), split
    ffi.call("xengUpchanReset")
    again = [u.run(g) for g in gulps]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
    ffi.call("xengUpchanReset")
    after_reset = u.run(gulps[2])
    u = up(ninput, nchan, ntime, N, nbeam, 0, False, P, h)
    fresh = u.run(gulps[2], w)
    assert after_reset.tobytes() == fresh.tobytes()
    check(fresh, upchan_beamform_pfb(gulps[2], w, N, nbeam, h, 0, ntime))
    u = up(ninput, nchan, ntime, N, nbeam, 3)
    plain = [u.run(g, w) for g in gulps]
    u = up(ninput, nchan, ntime, N, nbeam, 3, False, 1, None)
    assert all(a.tobytes() == u.run(g, w).tobytes() for a, g in zip(plain, gulps))


def _tone(N, offset, nframe, amp=6.5, ninput=4):
    """A complex tone at fine-channel offset `offset` from channel j = N/4 (k = 3N/4), 4+4-bit quantised, on input 0 only."""
    t = np.arange(nframe * N)
    x = amp * np.exp(2j * np.pi * (3 * N // 4 + offset) * t / N)
    re = np.clip(np.round(x.real), -8, 7).astype(np.int64)
    im = np.clip(np.round(x.imag), -8, 7).astype(np.int64)
    v = np.zeros((nframe * N, 1, ninput), np.uint8)
    v[:, 0, 0] = ((re & 0xF) << 4) | (im & 0xF)
    return v


@pytest.mark.parametrize("offset", [0.25, 0.5])
def test_tone_leakage_through_the_default_filter(up, offset):
    """A quantised tone (amplitude 6.5) between fine channels, one input, unit weights, power over 80-frame windows, three
    gulps (240 frames): through the default 4-tap filter the largest channel >= 2 away from the tone's channel is <= -20 dB of
    the peak (the float64 model: -27 to -32); through the plain FFT it is >= -18 dB (the model: -9.5 to -17)."""
    N, nf, ninput = 32, 80, 4
    stream = _tone(N, offset, 3 * nf, ninput=ninput)
    w = np.ones((1, N, 1, ninput), np.complex64)
    j0 = N // 4                             # (k = 3N/4 -> j = (k + N/2) mod N = N/4)
    far = np.minimum((np.arange(N) - j0) % N, (j0 - np.arange(N)) % N) >= 2
    res = {}
    for ntap in (4, 1):
        u = up(ninput, 1, nf * N, N, 1, nf, False, ntap if ntap > 1 else None, pfb_coeffs(ntap, N) if ntap > 1 else None)
        for k in range(3):
            p = u.run(stream[k * nf * N:(k + 1) * nf * N], w if k == 0 else None)[0, 0, 0]
        assert np.argmax(p) in (j0, j0 + 1)
        res[ntap] = 10 * np.log10(p[far].max() / p.max())
    assert res[4] <= -20 and res[1] >= -18, res


def test_set_pfb_checks_that_need_the_context(up):
    """Non-finite coefficients and a gulp shorter than the history are refused (INVALID_ARGUMENT) and leave the context as it
    was; ntap outside 1..8 and NULL coefficients with ntap > 1 too."""
    ninput, nchan, N, ntime = 8, 1, 16, 64
    rng = np.random.default_rng(3)
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    w = rand_w(rng, nchan, N, 2, ninput)
    u = up(ninput, nchan, ntime, N, 2)
    before = u.run(vin, w)
    h = np.ones(8 * N, np.float32)
    for name in ("xengUpchanSetPfb", "xengUpchanCorrSetPfb"):
        if name == "xengUpchanCorrSetPfb":
            ffi.call("xengUpchanCorrInitialize", 0, ninput, nchan, ntime, N, 0, N, 0)
        for ntap, coeffs in ((2, np.r_[np.ones(2 * N - 1), np.nan]), (1, np.r_[np.inf, np.ones(N - 1)]), (6, h[:6 * N]), (0, h), (9, h), (2, None)):
            with pytest.raises(ffi.XengError) as ei:
                set_pfb(name, ntap, coeffs)
            assert ei.value.status == INVALID_ARGUMENT, (name, ntap)
    ffi.call("xengUpchanCorrDestroy")
    assert u.run(vin).tobytes() == before.tobytes()


# ---------------------------------------------------------------- UpchanCorr
class UCP:
    def __init__(self, ninput, nchan, ntime, N, fine_lo, fine_hi, nstage=0, ntap=None, h=None):
        self.ninput, self.nchan, self.ntime, self.N = ninput, nchan, ntime, N
        ffi.call("xengUpchanCorrInitialize", 0, ninput, nchan, ntime, N, fine_lo, fine_hi, nstage)
        if ntap is not None:
            set_pfb("xengUpchanCorrSetPfb", ntap, h)
        self.nfine = fine_hi - fine_lo
        self.row = nchan * ninput
        self.din = ffi.DeviceBuffer(ntime * self.row)
        self.nout = self.nfine * ninput * ninput * 8
        self.dout = ffi.DeviceBuffer(self.nout + GUARD)

    def put(self, gulp, split=None, prime=False):
        self.din.upload(np.ascontiguousarray(gulp).reshape(-1))
        p = self.din.ptr
        if split is None:
            ffi.call("xengUpchanCorrPrime" if prime else "xengUpchanCorrAccumulate", p)
        else:
            ffi.call("xengUpchanCorrPrimeParts" if prime else "xengUpchanCorrAccumulateParts", p, split, p + split * self.row)
        ffi.call("xengUpchanCorrSync")          # (the next gulp is uploaded into the same buffer)

    def dump(self):
        ffi.call("xengMemset", self.dout.ptr, POISON, self.nout + GUARD)
        ffi.call("xengUpchanCorrDump", self.dout.ptr)
        ffi.call("xengUpchanCorrSync")
        raw = self.dout.download(np.uint8)
        assert (raw[self.nout:] == POISON).all(), "bytes past the output were written"
        return raw[:self.nout].view(np.complex64).reshape(self.nfine, self.ninput, self.ninput).copy()


@pytest.fixture
def ucp():
    yield UCP
    ffi.call("xengUpchanCorrDestroy")


def _corr_check(v, stream, N, h, gulps, ntime, lo, hi, first=0):
    X = np.concatenate([pfb_fine_select(stream, N, h, k * ntime, ntime, lo, hi, first) for k in gulps])
    exp, scale = upchan_corr_pfb(X)
    err = np.abs(v.astype(np.complex128) - exp)
    assert (err <= 1e-6 * scale).all(), "worst |err| / sum|X_i||X_j| = %.3g" % np.max(err / np.maximum(scale, 1e-30))


@pytest.mark.parametrize("N", [2, 8, 32])
@pytest.mark.parametrize("P", [2, 4])
def test_corr_against_restatement(ucp, N, P):
    """Two integrations of two gulps, a fine-channel selection, 40 inputs (padded to 64), asymmetric coefficients: within 1e-6
    of sum |X_i||X_j|; the second integration sees the first's tail."""
    ninput, nchan, ntime = 40, 3, 4 * N
    lo, hi = 1, 3 * N - 1
    rng = np.random.default_rng(N * 10 + P)
    stream = rng.integers(0, 256, (4 * ntime, nchan, ninput), dtype=np.uint8)
    h = (pfb_coeffs(P, N) * (1 + 0.3 * rng.standard_normal(P * N))).astype(np.float32)
    u = ucp(ninput, nchan, ntime, N, lo, hi, 0, P, h)
    for i in range(2):
        for k in (2 * i, 2 * i + 1):
            u.put(stream[k * ntime:(k + 1) * ntime])
        _corr_check(u.dump(), stream, N, h, (2 * i, 2 * i + 1), ntime, lo, hi)


def test_corr_bit_identity(ucp):
    """Against the reference run (default nstage, whole gulps): two-part gulps split inside the history span, nstage 1, a
    repeat after Reset; and a Prime followed by an integration against the same integration in a context that accumulated and
    dumped the primed gulp first (Dump leaves the history alone)."""
    ninput, nchan, N, P = 36, 2, 8, 4
    ntime = 4 * N
    lo, hi = 3, 13
    rng = np.random.default_rng(5)
    stream = rng.integers(0, 256, (4 * ntime, nchan, ninput), dtype=np.uint8)
    g = [stream[k * ntime:(k + 1) * ntime] for k in range(4)]
    h = rng.standard_normal(P * N).astype(np.float32)

    def two(u, split=None):
        out = []
        for i in range(2):
            u.put(g[2 * i], split)
            u.put(g[2 * i + 1], split)
            out.append(u.dump())
        return out
    u = ucp(ninput, nchan, ntime, N, lo, hi, 0, P, h)
    ref = two(u)
    _corr_check(ref[1], stream, N, h, (2, 3), ntime, lo, hi)
    ffi.call("xengUpchanCorrReset")
    for a, b in zip(ref, two(u, split=2 * N)):       # (the 24-sample tail straddles the split at 16)
        assert a.tobytes() == b.tobytes()
    ffi.call("xengUpchanCorrReset")
    for a, b in zip(ref, two(u)):
        assert a.tobytes() == b.tobytes()
    u = ucp(ninput, nchan, ntime, N, lo, hi, 1, P, h)
    for a, b in zip(ref, two(u)):
        assert a.tobytes() == b.tobytes()
    u = ucp(ninput, nchan, ntime, N, lo, hi, 0, P, h)
    u.put(g[1])
    u.dump()
    u.put(g[2])
    u.put(g[3])
    dumped = u.dump()
    u = ucp(ninput, nchan, ntime, N, lo, hi, 0, P, h)
    u.put(g[1], split=N, prime=True)
    u.put(g[2])
    u.put(g[3])
    primed = u.dump()
    assert dumped.tobytes() == primed.tobytes() == ref[1].tobytes()


# ---------------------------------------------------------------- the blocks on device rings
class _Span:
    def __init__(self, buf, nbytes):
        self.buf, self.ptr, self.nbytes = buf, buf.ptr, nbytes


class _DevSeq:
    """An input sequence of device spans whose reader saw only some gulps (ispan.offset tells where each one was)."""

    def __init__(self, hdr, gulps, igulp, split_bytes=None):
        self.header = types.SimpleNamespace(tostring=lambda: json.dumps(hdr).encode())
        self.time_tag = hdr['seq0']
        self.spans = []
        for k, a in gulps:
            b = ffi.DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a).reshape(-1))
            parts = None
            if split_bytes is not None:
                b1 = ffi.DeviceBuffer(a.nbytes - split_bytes).upload(np.ascontiguousarray(a).reshape(-1)[split_bytes:])
                parts = [_Span(b, split_bytes), _Span(b1, a.nbytes - split_bytes)]
            self.spans.append(types.SimpleNamespace(size=a.nbytes, offset=k * igulp, data=_Span(b, a.nbytes), parts=parts))

    def read(self, n):
        return iter(self.spans)


class _DevRing:
    span_memory_outlives_release = False
    name = "fake-device-input"

    def __init__(self, seqs):
        self.seqs = seqs

    def read(self, guarantee=True):
        return iter(self.seqs)


def test_blocks_on_device_rings_with_a_gap_and_two_sequences():
    """UpchanBeamform and UpchanCorr at pfb_ntap=4: sequence 1 misses gulp 4 of 8 (two-part gulps), sequence 2 starts fresh;
    each output equals the restatement with the samples before the sequence's start or the gap taken as zero (UpchanCorr's
    integration after the gap primed with the gulp before its boundary)."""
    nchan, nstand, nbeam, N, P, g = 2, 4, 2, 16, 4, 64
    ninput = 2 * nstand
    rng = np.random.default_rng(9)
    s1 = rng.integers(0, 256, (8 * g, nchan, ninput), dtype=np.uint8)
    s2 = rng.integers(0, 256, (2 * g, nchan, ninput), dtype=np.uint8)
    h1, h2 = source_header(nchan, nstand, 2, seq0=0, sfreq=40e6), source_header(nchan, nstand, 2, seq0=20000, sfreq=40e6)
    seen1 = [(k, s1[k * g:(k + 1) * g]) for k in range(8) if k != 4]
    seen2 = [(k, s2[k * g:(k + 1) * g]) for k in range(2)]
    igulp = g * nchan * ninput
    h = pfb_coeffs(P, N)

    def ring_in(split):
        return _DevRing([_DevSeq(h1, seen1, igulp, split), _DevSeq(h2, seen2, igulp)])

    ru = Ring("up-output", space="cuda")
    upb = UpchanBeamform(LOG, ring_in(48 * nchan * ninput), ru, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, pfb_ntap=P)
    w = rand_w(rng, nchan, N, nbeam, ninput)
    upb.weights_cpu[...] = w
    sink = Sink(ru, (g // N) * nbeam * nchan * N * 8)
    sink.start()
    try:
        upb.main()
    finally:
        sink.join(30)
        ffi.call("xengUpchanDestroy")
    assert [hd['pfb_ntap'] for hd, _, _ in sink.sequences] == [P, P]
    for (hd, _, spans), stream, seen in zip(sink.sequences, (s1, s2), (seen1, seen2)):
        assert len(spans) == len(seen)
        for (k, _), s in zip(seen, spans):
            exp = upchan_beamform_pfb(stream, w, N, nbeam, h, k * g, g, first=5 * g if stream is s1 and k >= 5 else 0)
            check(s.view(np.complex64).reshape(exp.shape), exp)

    rc = Ring("uc-output", space="cuda")
    ucb = UpchanCorr(LOG, ring_in(None), rc, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=2 * g // N,
                     fine_lo=2, fine_hi=29, pfb_ntap=P)
    sink = Sink(rc, 27 * ninput * ninput * 8)
    sink.start()
    try:
        ucb.main()
    finally:
        sink.join(30)
        ffi.call("xengUpchanCorrDestroy")
    spans = [(hd['seq0'], s) for hd, _, ss in sink.sequences for s in ss]
    # sequence 1: [0, 1], [2, 3]; gulp 4 missing loses [4, 5]; gulp 5 waits for the boundary and primes; [6, 7] sees its tail
    expect = [(s1, 0, 0), (s1, 2, 0), (s1, 6, 5 * g), (s2, 0, 0)]
    assert [sq for sq, _ in spans] == [0, 0, 6 * g, 20000]
    for (stream, k, first), (_, s) in zip(expect, spans):
        _corr_check(s.view(np.complex64).reshape(27, ninput, ninput), stream, N, h, (k, k + 1), g, 2, 29, first)
