"""UpchanCorr on CPU rings (no GPU), both ring implementations: the float64 restatement of the reference's upchannelised
imaging chain (tests/upchan_corr_ref.py) against golden_corr and the golden file at N = 1 and an int64 restatement at N = 2
and 4; the block's output header, fine-channel selection, integrations aligned to seq0, two-part gulps, a short final gulp,
a skipped gulp, constructor rejections; and the C entry points' argument checks.  The kernel calls go to the oracle backend
below (the restatement, on system-space spans)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanCorr
from caltech_bifrost_dsp_amd.ring import Ring
from oracle import xeng_oracle as orc
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.upchan_corr_ref import fine_freqs, upchan_corr, upchan_corr_int

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_64t_32a_8c_32s_2p_deadbeef.npz")


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


class UpchanCorrOracleBackend(OracleBackend):
    """The oracle backend plus xengUpchanCorr* served by the float64 restatement (results cast to cf32)."""

    def __init__(self):
        super().__init__()
        self.uc = None
        self.gulps = []
        self.calls = []                 # 'run' | 'parts' | 'dump' | 'reset'

    def upchan_corr_initialize(self, gpu, ninput, nchan, ntime, nupchan, fine_lo, fine_hi, nstage=0):
        self.uc = dict(ninput=ninput, nchan=nchan, ntime=ntime, nupchan=nupchan, fine_lo=fine_lo, fine_hi=fine_hi)
        return 0

    def upchan_corr_accumulate(self, in_arr):
        u = self.uc
        self.gulps.append(in_arr.numpy().reshape(-1).view(np.uint8).reshape(u['ntime'], u['nchan'], u['ninput']).copy())
        self.calls.append('run')
        return 0

    def upchan_corr_accumulate_parts(self, part0, ntime0, part1):
        u = self.uc
        row = u['nchan'] * u['ninput']
        assert part0.nbytes == ntime0 * row and ntime0 % u['nupchan'] == 0
        v = np.concatenate([part0.numpy().reshape(-1), part1.numpy().reshape(-1)]).view(np.uint8)
        self.gulps.append(v.reshape(u['ntime'], u['nchan'], u['ninput']).copy())
        self.calls.append('parts')
        return 0

    def upchan_corr_dump(self, out_arr):
        u = self.uc
        v = upchan_corr(np.concatenate(self.gulps), u['nupchan'], u['fine_lo'], u['fine_hi'])
        out_arr.numpy().reshape(-1).view(np.complex64)[...] = v.reshape(-1)
        self.gulps = []
        self.calls.append('dump')
        return 0

    def upchan_corr_reset(self):
        self.gulps = []
        self.calls.append('reset')

    def upchan_corr_mark(self):
        return self.beam_mark()

    def upchan_corr_wait(self, ticket):
        self.beam_wait(ticket)

    def upchan_corr_sync(self):
        pass


# ---------------------------------------------------------------- the restatement itself
def test_restatement_at_n1_is_golden_corr_and_the_golden_file():
    """N = 1 is the coarse-channel correlator: the restatement equals golden_corr (make_golden_inputs.py:150-158) and both
    32-sample integrations stored in the golden file, exactly."""
    d = np.load(GOLDEN)
    vin = d['vin']                                              # [64][8][32][2]
    ntime, nchan, nstand, npol = vin.shape
    for k in range(2):
        part = vin[32 * k:32 * (k + 1)]
        v = upchan_corr(part.reshape(32, nchan, nstand * npol), 1).reshape(nchan, nstand, npol, nstand, npol)
        v = v.transpose(0, 1, 3, 2, 4)                          # -> [c][s0][s1][p0][p1]
        rr, ii = orc.golden_corr(part)
        assert np.array_equal(v.real, rr) and np.array_equal(v.imag, ii)
        assert np.array_equal(v.real, d['corr_re'][k]) and np.array_equal(v.imag, d['corr_im'][k])


@pytest.mark.parametrize("nupchan", [2, 4])
def test_restatement_at_n2_n4_is_the_int64_restatement(nupchan):
    rng = np.random.default_rng(nupchan)
    vin = rng.integers(0, 256, (12 * nupchan, 3, 10), dtype=np.uint8)
    vin.reshape(-1)[:256] = np.arange(256)
    v = upchan_corr(vin, nupchan, 1, 3 * nupchan - 1)
    re, im = upchan_corr_int(vin, nupchan, 1, 3 * nupchan - 1)
    assert np.array_equal(v.real, re) and np.array_equal(v.imag, im)


def test_restatement_fine_channels_and_tone():
    """A tone of 4-bit-exact samples 7 i^n (k = N/4) on input 2 of coarse channel 1 lands in merged fine channel N + 3N/4:
    its autocorrelation there is (7 N)^2 per frame, zero in every other fine channel."""
    N, nchan, ninput, nframe = 8, 2, 4, 3
    vin = np.zeros((nframe * N, nchan, ninput), np.uint8)
    for n in range(nframe * N):
        v = 7 * 1j ** n
        vin[n, 1, 2] = ((int(round(v.real)) & 0xF) << 4) | (int(round(v.imag)) & 0xF)
    auto = upchan_corr(vin, N)[:, 2, 2]
    m = N + 3 * N // 4
    assert np.allclose(auto[m], nframe * (7 * N) ** 2) and np.abs(np.delete(auto, m)).max() < 1e-9
    f = fine_freqs(30e6, 2e5, nchan, N)
    assert f[m] == pytest.approx(30e6 + 1e5 + (3 * N // 4 - N // 2) * 1e5 / N)


# ---------------------------------------------------------------- the block
def _run(vin, g, N, nfpi, nchan, nstand, fine_lo=0, fine_hi=None, span=None, seq0=1000, sfreq=40e6, chan_bw=25e3):
    ninput = 2 * nstand
    hdr = source_header(nchan, nstand, 2, seq0=seq0, chan0=64, sfreq=sfreq, chan_bw=chan_bw)
    r0, r1 = Ring("gpu-input"), Ring("uc-output")
    if span is not None:
        r0.resize(span * nchan * ninput, 8 * g * nchan * ninput)
    be = UpchanCorrOracleBackend()
    uc = UpchanCorr(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=nfpi,
                    fine_lo=fine_lo, fine_hi=fine_hi, backend=be)
    nfine = (fine_hi if fine_hi is not None else nchan * N) - fine_lo
    sink = Sink(r1, nfine * ninput * ninput * 8)
    run_blocks([uc], Source(r0, [(hdr, vin, (span or g) * nchan * ninput)]), [sink])
    return uc, be, sink, hdr


def test_integrations_aligned_to_seq0_with_header_and_short_final_gulp():
    """7.5 gulps, 2 gulps per integration: three integrations, the 7th gulp's integration never completes (not written), the
    half gulp at the end is skipped.  Each span is the restatement over its two gulps; the header describes the fine axis."""
    nchan, nstand, N, g = 3, 2, 4, 16
    ninput = 2 * nstand
    rng = np.random.default_rng(3)
    vin = rng.integers(0, 256, (7 * g + g // 2, nchan, ninput), dtype=np.uint8)
    uc, be, sink, hdr = _run(vin, g, N, nfpi=2 * g // N, nchan=nchan, nstand=nstand)
    assert len(sink.sequences) == 1
    ohdr, tag, spans = sink.sequences[0]
    assert len(spans) == 3
    for k in range(3):
        exp = upchan_corr(vin[2 * k * g:(2 * k + 2) * g], N)
        assert np.allclose(spans[k].view(np.complex64).reshape(exp.shape), exp, rtol=1e-6)
    assert be.calls.count('run') == 7 and be.calls.count('dump') == 3 and be.calls[-1] == 'reset'
    assert uc.stats['nintegration'] == 3 and uc.stats['ndropped'] == 0
    for key in ('nchan', 'chan0', 'sfreq', 'bw_hz', 'nstand', 'npol', 'system_nchan'):
        assert ohdr[key] == hdr[key]
    assert (ohdr['seq0'], tag) == (1000, 1000)
    assert (ohdr['nupchan'], ohdr['fine_lo'], ohdr['nfine'], ohdr['nbit'], ohdr['complex']) == (N, 0, nchan * N, 32, True)
    assert (ohdr['nframe_per_integration'], ohdr['acc_len']) == (2 * g // N, 2 * g)
    assert ohdr['fine_bw_hz'] == pytest.approx(25e3 / N)
    assert ohdr['fine_sfreq'] == pytest.approx(fine_freqs(40e6, 25e3 * nchan, nchan, N)[0]) == pytest.approx(40e6 - 12.5e3)


def test_fine_channel_selection():
    """[fine_lo, fine_hi) across a coarse-channel boundary: the span holds those fine channels only, fine_sfreq is the centre
    of fine_lo."""
    nchan, nstand, N, g = 3, 2, 8, 16
    rng = np.random.default_rng(4)
    vin = rng.integers(0, 256, (2 * g, nchan, 2 * nstand), dtype=np.uint8)
    lo, hi = 5, 19
    uc, be, sink, hdr = _run(vin, g, N, nfpi=g // N, nchan=nchan, nstand=nstand, fine_lo=lo, fine_hi=hi)
    ohdr, _, spans = sink.sequences[0]
    assert len(spans) == 2 and ohdr['nfine'] == hi - lo and ohdr['fine_lo'] == lo
    full = upchan_corr(vin[:g], N)
    assert np.allclose(spans[0].view(np.complex64).reshape(hi - lo, 4, 4), full[lo:hi], rtol=1e-6)
    assert ohdr['fine_sfreq'] == pytest.approx(fine_freqs(40e6, 25e3 * nchan, nchan, N, lo, hi)[0])


def test_two_part_gulps_equal_one_span_gulps():
    nchan, nstand, N, g = 2, 2, 8, 32
    rng = np.random.default_rng(5)
    vin = rng.integers(0, 256, (4 * g, nchan, 2 * nstand), dtype=np.uint8)
    out = {}
    for span in (g, g // 2):
        uc, be, sink, hdr = _run(vin, g, N, nfpi=2 * g // N, nchan=nchan, nstand=nstand, span=span)
        out[span] = (b''.join(s.tobytes() for s in sink.sequences[0][2]), [c for c in be.calls if c in ('run', 'parts')])
    assert out[g][1] == ['run'] * 4 and out[g // 2][1] == ['parts'] * 4
    assert out[g][0] == out[g // 2][0] and len(out[g][0]) == 2 * nchan * N * 16 * 8


class _Data:
    def __init__(self, a):
        self.a = a
        self.nbytes = a.nbytes

    def numpy(self):
        return self.a


class _FakeSeq:
    """An input sequence whose reader saw only some gulps (ispan.offset tells where each one was)."""

    def __init__(self, hdr, gulps, igulp):
        self.header = types.SimpleNamespace(tostring=lambda: json.dumps(hdr).encode())
        self.gulps, self.igulp = gulps, igulp

    def read(self, n):
        for k, a in self.gulps:
            yield types.SimpleNamespace(size=a.nbytes, offset=k * self.igulp, data=_Data(a.reshape(-1)), parts=None)


class _FakeRing:
    span_memory_outlives_release = False
    name = "fake-input"

    def __init__(self, seqs):
        self.seqs = seqs

    def read(self, guarantee=True):
        return iter(self.seqs)


@pytest.mark.parametrize("missing,ndropped", [((3,), 1), ((2,), 1), ((3, 4, 5), 2)])
def test_skipped_gulps_drop_their_integrations(missing, ndropped):
    """2 gulps per integration, gulps `missing` never read: each integration they touch is dropped (Reset when one was in
    progress) and counted; the output realigns to the next boundary in a new sequence whose seq0 is its start."""
    nchan, nstand, N, g, ngulp, seq0 = 1, 2, 4, 8, 10, 500
    ninput = 2 * nstand
    rng = np.random.default_rng(6)
    vin = rng.integers(0, 256, (ngulp, g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=seq0, sfreq=1e6)
    seen = [(k, vin[k]) for k in range(ngulp) if k not in missing]
    r1 = Ring("uc-output")
    be = UpchanCorrOracleBackend()
    uc = UpchanCorr(LOG, _FakeRing([_FakeSeq(hdr, seen, g * nchan * ninput)]), r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N,
                    nframe_per_integration=2 * g // N, backend=be)
    sink = Sink(r1, nchan * N * ninput * ninput * 8)
    sink.start()
    uc.main()
    sink.join(20)
    assert uc.stats['ndropped'] == ndropped
    assert be.calls.count('reset') == (1 if 3 in missing else 0)
    done = [k for k in range(0, ngulp, 2) if k not in missing and k + 1 not in missing]
    starts = [h['seq0'] for h, _, _ in sink.sequences]
    assert starts == [seq0, seq0 + (max(missing) // 2 + 1) * 2 * g]
    spans = [s for _, _, ss in sink.sequences for s in ss]
    assert len(spans) == len(done) == uc.stats['nintegration']
    for k, s in zip(done, spans):
        exp = upchan_corr(vin[k:k + 2].reshape(2 * g, nchan, ninput), N)
        assert np.allclose(s.view(np.complex64).reshape(exp.shape), exp, rtol=1e-6)


def test_a_failing_gulp_lets_go_of_the_calls_in_flight_only_after_their_kernels():
    """The third gulp's call fails with two integrations in flight: the block raises, and every span a call in flight holds
    (its input, its uncommitted output) was still alive when that call's ticket was waited for (the sequence's own exit
    retires them) or the stream synchronised; let go under a running kernel, their memory would go back to the ring."""
    import weakref

    class Failing(UpchanCorrOracleBackend):
        def __init__(self):
            super().__init__()
            self.held, self.by_ticket, self.alive = [], {}, []

        def upchan_corr_accumulate(self, in_arr):
            if len(self.by_ticket) == 2:
                return 3
            self.held.append(weakref.ref(in_arr))
            return super().upchan_corr_accumulate(in_arr)

        def upchan_corr_dump(self, out_arr):
            self.held.append(weakref.ref(out_arr))
            return super().upchan_corr_dump(out_arr)

        def upchan_corr_mark(self):
            t = super().upchan_corr_mark()
            self.by_ticket[t], self.held = self.held, []
            return t

        def upchan_corr_wait(self, ticket):
            self.alive.append(all(r() is not None for r in self.by_ticket.pop(ticket)))
            super().upchan_corr_wait(ticket)

        def upchan_corr_sync(self):
            self.alive.extend(all(r() is not None for r in refs) for refs in self.by_ticket.values())
            self.by_ticket.clear()

    nchan, nstand, N, g = 2, 2, 4, 16
    ninput = 2 * nstand
    vin = np.random.default_rng(6).integers(0, 256, (6 * g, nchan, ninput), dtype=np.uint8)
    r0, r1 = Ring("gpu-input"), Ring("uc-output")
    be = Failing()
    uc = UpchanCorr(LOG, r0, r1, nchan=nchan, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_per_integration=g // N, backend=be)
    sink = Sink(r1, nchan * N * ninput * ninput * 8)
    src = Source(r0, [(source_header(nchan, nstand, 2), vin, g * nchan * ninput)], wait_readers=1)
    sink.start()
    src.start()
    with pytest.raises(RuntimeError, match="xengUpchanCorrAccumulate returned 3"):
        uc.main()
    assert be.alive == [True, True] and not be.by_ticket


def test_constructor_rejections():
    be = UpchanCorrOracleBackend()
    ok = dict(nchan=2, ninput=4, ntime_gulp=32, nupchan=8, nframe_per_integration=8)
    for bad in (dict(nupchan=3), dict(nupchan=128), dict(ntime_gulp=36), dict(nframe_per_integration=6), dict(nframe_per_integration=0),
                dict(fine_lo=-1), dict(fine_lo=4, fine_hi=4), dict(fine_hi=17), dict(fine_lo=16)):
        with pytest.raises(ValueError):
            UpchanCorr(LOG, Ring("a"), Ring("b"), backend=be, **dict(ok, **bad))
    uc = UpchanCorr(LOG, Ring("a"), Ring("b"), backend=be, fine_lo=3, **ok)
    assert (uc.nfine, uc.gulps_per_integration, uc.acc_len) == (13, 2, 64)
    assert be.uc['fine_lo'] == 3 and be.uc['fine_hi'] == 16


# ---------------------------------------------------------------- the C entry points without a GPU
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_point_argument_checks_need_no_gpu():
    """Bad sizes and pointers are refused with INVALID_ARGUMENT before any device is touched (nothing launched); good
    arguments without a live context with INVALID_STATE."""
    ok = dict(gpu=0, ninput=8, nchan=2, ntime=64, nupchan=32, fine_lo=0, fine_hi=64, nstage=0)
    bad = [dict(ninput=0), dict(ninput=-4), dict(nchan=0), dict(ntime=0), dict(nstage=-1), dict(nupchan=3), dict(nupchan=0),
           dict(nupchan=128), dict(ntime=48), dict(fine_lo=-1), dict(fine_hi=65), dict(fine_lo=10, fine_hi=10),
           dict(fine_lo=10, fine_hi=9), dict(nupchan=1, fine_hi=3)]
    for b in bad:
        a = dict(ok, **b)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanCorrInitialize", *a.values())
        assert ei.value.status == INVALID_ARGUMENT and "UpchanCorr" in str(ei.value), b
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanCorrAccumulate", None)
    assert ei.value.status == INVALID_ARGUMENT
    for in0, ntime0, in1 in ((0, 32, 4096), (4096, 0, 4096), (4096, -32, 4096), (4096, 32, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanCorrAccumulateParts", in0, ntime0, in1)
        assert ei.value.status == INVALID_ARGUMENT, (in0, ntime0, in1)
    for out in (0, 8200):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanCorrDump", out)
        assert ei.value.status == INVALID_ARGUMENT, out
    for name, args in (("xengUpchanCorrMark", (None,)), ("xengUpchanCorrTicketDone", (1, None)), ("xengUpchanCorrGetInfo", (None, None))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, name
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_upchan_corr_gpu.py covers the rest)
    ffi.call("xengUpchanCorrDestroy")   # (no context: nothing to do)
    t, d, n = ctypes.c_ulonglong(), ctypes.c_int(-1), ctypes.c_int(-1)
    for name, args in (("xengUpchanCorrAccumulate", (4096,)), ("xengUpchanCorrAccumulateParts", (4096, 32, 4096)), ("xengUpchanCorrDump", (8192,)),
                       ("xengUpchanCorrReset", ()), ("xengUpchanCorrMark", (ctypes.byref(t),)), ("xengUpchanCorrWait", (1,)),
                       ("xengUpchanCorrTicketDone", (1, ctypes.byref(d))), ("xengUpchanCorrSync", ()),
                       ("xengUpchanCorrGetInfo", (ctypes.byref(n), ctypes.byref(n)))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    assert d.value == -1 and n.value == -1
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanCorrInitialize", *ok.values())  # (valid sizes: the device is what fails here)
    assert ei.value.status not in (0, INVALID_ARGUMENT)
