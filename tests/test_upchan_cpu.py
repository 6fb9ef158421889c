"""UpchanBeamform and TbfSource on CPU rings (no GPU), both ring implementations: the float64 restatement of the reference's
upchannelising chain (tests/upchan_ref.py) checked against a direct DFT, the block's commands -> weights (Beamform's formula at
fine frequencies, fine-resolution `calgains`, timed `load_sample`), its output header, two-part gulps, a short final gulp,
gulp times after skipped gulps; .tbf files through TbfSource; and the C entry points' argument checks.  The kernel call goes
to the oracle backend below (the restatement, on system-space spans)."""
import ctypes
import json
import os
import struct
import threading

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import TbfSource, UpchanBeamform
from caltech_bifrost_dsp_amd.ring import Ring
from oracle import xeng_oracle as orc
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, GatedSource, Sink, Source, run_blocks, source_header, wait_for
from tests.test_blocks_cpu import cmd
from tests.upchan_ref import channelise, fine_freqs, upchan_beamform, upchan_weights

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


class UpchanOracleBackend(OracleBackend):
    """The oracle backend plus xengUpchan* served by the float64 restatement (results cast to the kernel's fp32 types)."""

    def __init__(self):
        super().__init__()
        self.up = None
        self.runs = []                  # ('run' | 'parts', weights version, the block's curr_sample at the call)
        self.block = None
        self.before_run = None

    def upchan_initialize(self, gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum):
        self.up = dict(ninput=ninput, nchan=nchan, ntime=ntime, nupchan=nupchan, nbeam=nbeam, nframe_sum=nframe_sum)
        return 0

    def _run(self, vin, out_arr, weights, version, kind):
        if self.before_run is not None:
            self.before_run()
        u = self.up
        vin = vin.reshape(u['ntime'], u['nchan'], u['ninput'])
        w = weights.numpy().reshape(u['nchan'], u['nupchan'], u['nbeam'], u['ninput'])
        r = upchan_beamform(vin, w, u['nupchan'], u['nbeam'], u['nframe_sum'])
        out = out_arr.numpy().reshape(-1).view(np.float32 if u['nframe_sum'] else np.complex64)
        out[...] = r.reshape(-1)
        self.runs.append((kind, version, self.block.stats.get('curr_sample') if self.block is not None else None))
        return 0

    def upchan_run(self, in_arr, out_arr, weights, version=0):
        return self._run(in_arr.numpy().reshape(-1).view(np.uint8), out_arr, weights, version, 'run')

    def upchan_run_parts(self, part0, ntime0, part1, out_arr, weights, version=0):
        row = self.up['nchan'] * self.up['ninput']
        assert part0.nbytes == ntime0 * row and ntime0 % self.up['nupchan'] == 0
        vin = np.concatenate([part0.numpy().reshape(-1), part1.numpy().reshape(-1)]).view(np.uint8)
        return self._run(vin, out_arr, weights, version, 'parts')

    def upchan_mark(self):
        return self.beam_mark()

    def upchan_wait(self, ticket):
        self.beam_wait(ticket)

    def upchan_sync(self):
        pass


# ---------------------------------------------------------------- the restatement itself
def test_restatement_is_the_dft_of_each_frame():
    """channelise() against a direct double-loop DFT with the fftshift written out: X[f,c,i,j] = sum_n x[fN+n,c,i]
    exp(-2 pi i k n / N), k = (j + N/2) mod N; and a 4-bit-exact tone at k = N/4 lands in j = 3N/4 only."""
    rng = np.random.default_rng(1)
    N, nframe, nchan, ninput = 8, 3, 2, 4
    vin = rng.integers(0, 256, (nframe * N, nchan, ninput), dtype=np.uint8)
    re, im = orc.decode(vin)
    x = re + 1j * im
    X = channelise(vin, N)
    for f in range(nframe):
        for j in range(N):
            k = (j + N // 2) % N
            d = sum(x[f * N + n] * np.exp(-2j * np.pi * k * n / N) for n in range(N))
            assert np.allclose(X[f, :, :, j], d, atol=1e-9)
    tone = np.zeros((2 * N, 1, 1), np.uint8)
    for n in range(2 * N):
        v = 7 * 1j ** n                                     # exp(2 pi i n / 4): k = N/4
        tone[n, 0, 0] = ((int(round(v.real)) & 0xF) << 4) | (int(round(v.imag)) & 0xF)
    p = np.abs(channelise(tone, N)[:, 0, 0, :]) ** 2
    assert np.allclose(p[:, 3 * N // 4], (7 * N) ** 2) and np.delete(p, 3 * N // 4, axis=1).max() < 1e-12


def test_power_mode_is_the_sum_of_voltage_powers():
    rng = np.random.default_rng(2)
    N, nframe, nchan, ninput, nbeam = 16, 6, 2, 8, 3
    vin = rng.integers(0, 256, (nframe * N, nchan, ninput), dtype=np.uint8)
    w = rng.standard_normal((nchan, N, nbeam, ninput)) + 1j * rng.standard_normal((nchan, N, nbeam, ninput))
    v = upchan_beamform(vin, w, N, nbeam)
    assert v.shape == (nframe, nbeam, nchan, N)
    assert np.allclose(upchan_beamform(vin, w, N, nbeam, 3), (np.abs(v) ** 2).reshape(2, 3, nbeam, nchan, N).sum(1))


# ---------------------------------------------------------------- the block
def _cal_cmds(nchan, N, nbeam, ninput, rng, start=0):
    cmds, cal = [], np.ones((nchan, N, nbeam, ninput), np.complex128)
    k = start
    for b in range(nbeam):
        for i in range(ninput):
            g = rng.uniform(-1, 1, 2 * nchan * N)
            cal[:, :, b, i] = (g[0::2] + 1j * g[1::2]).reshape(nchan, N)
            cmds.append(cmd(k, coeffs={'type': 'calgains', 'input_id': i, 'beam_id': b, 'data': g.tolist()}))
            k += 1
    return cmds, cal


def _coeff_cmds(nbeam, ninput, rng, load_sample=None, start=10000):
    cmds, delays, amps = [], {}, {}
    for b in range(nbeam):
        delays[b], amps[b] = rng.uniform(0, 12, ninput), rng.uniform(0.5, 2, ninput)
        c = {'type': 'beamcoeffs', 'beam_id': b, 'data': {'delays': delays[b].tolist(), 'amps': amps[b].tolist()}}
        if load_sample is not None:
            c['load_sample'] = load_sample
        cmds.append(cmd(start + b, coeffs=c))
    return cmds, delays, amps


def _expected_weights(freqs, cal, delays, amps, nbeam):
    w = np.zeros(cal.shape, np.complex128)
    for b in range(nbeam):
        w[:, :, b, :] = upchan_weights(freqs, delays[b], amps[b], cal[:, :, b, :])
    return w


@pytest.mark.parametrize("nframe_sum", [0, 2])
def test_commands_weights_header_and_timed_load(nframe_sum):
    """calgains at fine resolution and beamcoeffs give amps * exp(2 pi i f_cj tau 1e-9) * cal at the fine frequencies of the
    header; the weights take effect from the gulp whose first sample reaches load_sample (gulps before it see the zero
    weights); output spans equal the restatement; a short final gulp is skipped; the header carries the fine-channel axis."""
    nchan, nstand, nbeam, N, g = 3, 2, 2, 8, 32
    ninput = 2 * nstand
    rng = np.random.default_rng(3 + nframe_sum)
    vin = rng.integers(0, 256, (4 * g + g // 2, nchan, ninput), dtype=np.uint8)
    seq0, sfreq, chan_bw = 4800, 45e6, 23925.78125
    hdr = source_header(nchan, nstand, 2, seq0=seq0, chan0=96, sfreq=sfreq, chan_bw=chan_bw)
    r0, r1 = Ring("gpu-input"), Ring("up-output")
    be = UpchanOracleBackend()
    up = UpchanBeamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=nframe_sum, backend=be)
    be.block = up
    freqs = fine_freqs(sfreq, chan_bw * nchan, nchan, N)
    up.freqs = freqs
    cal_cmds, cal = _cal_cmds(nchan, N, nbeam, ninput, rng)
    co_cmds, delays, amps = _coeff_cmds(nbeam, ninput, rng, load_sample=seq0 + 2 * g)
    up.process_command_strings(cal_cmds + co_cmds)
    w = _expected_weights(freqs, cal, delays, amps, nbeam)
    assert np.allclose(up.weights_new, w, rtol=1e-6, atol=1e-6)
    nout = (g // N // (nframe_sum or 1)) * nbeam * nchan * N * (4 if nframe_sum else 8)
    sink = Sink(r1, nout)
    run_blocks([up], Source(r0, [(hdr, vin, g * nchan * ninput)]), [sink])
    ohdr, _, spans = sink.sequences[0]
    assert len(spans) == 4 and len(be.runs) == 4                # (the half gulp at the end is skipped)
    assert [r[2] for r in be.runs] == [seq0 + k * g for k in range(4)]
    assert [r[1] for r in be.runs] == [1, 1, 2, 2]              # one upload at the start, one at the load sample
    for k in range(4):
        wk = w if k >= 2 else np.zeros_like(w)
        exp = upchan_beamform(vin[k * g:(k + 1) * g], wk.astype(np.complex64), N, nbeam, nframe_sum)
        got = spans[k].view(np.float32 if nframe_sum else np.complex64).reshape(exp.shape)
        assert np.allclose(got, exp, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(exp).max()))
    for key in ('nchan', 'chan0', 'sfreq', 'bw_hz', 'seq0', 'system_nchan'):
        assert ohdr[key] == hdr[key]
    assert (ohdr['nbeam'], ohdr['nupchan'], ohdr['nframe_sum'], ohdr['nbit'], ohdr['npol']) == (nbeam, N, nframe_sum, 32, 1)
    assert ohdr.get('complex', False) is (nframe_sum == 0)
    assert ohdr['fine_bw_hz'] == pytest.approx(chan_bw / N)
    assert ohdr['fine_sfreq'] == pytest.approx(freqs[0, 0]) and freqs[0, 0] == pytest.approx(sfreq - chan_bw / 2)


def test_two_part_gulps_equal_one_span_gulps():
    """A writer whose spans are half a gulp: the gulps come as two parts (read_parts -> upchan_run_parts, no gathered copy),
    and the output equals the one-span run."""
    nchan, nstand, nbeam, N, g = 2, 2, 3, 16, 64
    ninput = 2 * nstand
    rng = np.random.default_rng(4)
    vin = rng.integers(0, 256, (3 * g, nchan, ninput), dtype=np.uint8)
    hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=30e6)
    outs = {}
    for span in (g, g // 2):
        r0, r1 = Ring("gpu-input"), Ring("up-output")
        r0.resize(span, 8 * g * nchan * ninput)
        be = UpchanOracleBackend()
        up = UpchanBeamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, backend=be)
        up.weights_cpu[...] = (rng.standard_normal(up.weights_cpu.shape) if span == g else outs['w'])
        outs.setdefault('w', up.weights_cpu.copy())
        sink = Sink(r1, (g // N) * nbeam * nchan * N * 8)
        run_blocks([up], Source(r0, [(hdr, vin, span * nchan * ninput)]), [sink])
        outs[span] = (b''.join(s.tobytes() for s in sink.sequences[0][2]), [r[0] for r in be.runs])
    assert outs[g][1] == ['run'] * 3 and outs[g // 2][1] == ['parts'] * 3
    assert outs[g][0] == outs[g // 2][0] and len(outs[g][0]) == 3 * (g // N) * nbeam * nchan * N * 8


def test_gulp_times_follow_the_span_position_after_skipped_gulps():
    """A reader that is not guaranteed and falls behind skips gulps; every gulp it does process is timed by its place in the
    sequence (the gulp index is written into the data, so each run can be matched to the gulp it read)."""
    nchan, nstand, nbeam, N, g, ngulp = 1, 2, 1, 8, 16, 12
    ninput = 2 * nstand
    gulp = g * nchan * ninput
    vin = np.zeros((ngulp, g, nchan, ninput), np.uint8)
    vin[...] = (np.arange(ngulp, dtype=np.uint8) << 4)[:, None, None, None]      # gulp k: every sample k + 0i (k < 8)
    vin[8:] = 0x10
    vin[8:, 0, 0, 0] = np.arange(8, ngulp, dtype=np.uint8)                       # (and a marker for k >= 8)
    r0, r1 = Ring("gpu-input"), Ring("up-output")
    r0.resize(gulp, 2 * gulp)
    be = UpchanOracleBackend()
    seen = []
    src = GatedSource(r0, source_header(nchan, nstand, 2, seq0=1000, sfreq=1e6), vin, gulp, {})

    def before():
        if not seen:
            wait_for(lambda: src.written == ngulp, "the source to have written every gulp")
        seen.append(1)
    be.before_run = before
    up = UpchanBeamform(LOG, r0, r1, guarantee=False, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, backend=be)
    be.block = up
    up.weights_cpu[...] = 1
    sink = Sink(r1, (g // N) * nbeam * nchan * N * 8)
    run_blocks([up], src, [sink])
    spans = sink.sequences[0][2]
    assert 0 < len(spans) < ngulp, "no gulp was skipped"
    times = [r[2] for r in be.runs]
    for t, s in zip(times, spans):
        k = (t - 1000) // g
        exp = upchan_beamform(vin[k].reshape(g, nchan, ninput), np.ones((nchan, N, nbeam, ninput), np.complex64), N, nbeam)
        assert np.allclose(s.view(np.complex64).reshape(exp.shape), exp)
    assert times == sorted(times) and times[-1] == 1000 + (ngulp - 1) * g


def test_a_failing_gulp_waits_for_the_stream_before_the_gulps_in_flight_let_go():
    """The third run fails with two gulps in flight: the block raises, and it has waited for the stream (upchan_sync) while
    the spans of those gulps -- inputs and uncommitted outputs -- were still held; let go under a running kernel, their
    memory would go back to the ring.  Nothing in flight is committed."""
    import weakref

    class Failing(UpchanOracleBackend):
        def __init__(self):
            super().__init__()
            self.held, self.syncs = [], []          # (input, output) of every run that succeeded; at each sync, which are alive

        def upchan_run(self, in_arr, out_arr, weights, version=0):
            if len(self.held) == 2:
                return 3
            self.held.append((weakref.ref(in_arr), weakref.ref(out_arr)))
            return super().upchan_run(in_arr, out_arr, weights, version)

        def upchan_sync(self):
            self.syncs.append([i() is not None and o() is not None for i, o in self.held])

    nchan, nstand, nbeam, N, g = 2, 2, 2, 8, 16
    ninput = 2 * nstand
    vin = np.random.default_rng(6).integers(0, 256, (6 * g, nchan, ninput), dtype=np.uint8)
    r0, r1 = Ring("gpu-input"), Ring("up-output")
    be = Failing()
    up = UpchanBeamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, backend=be)
    sink = Sink(r1, (g // N) * nbeam * nchan * N * 8)
    src = Source(r0, [(source_header(nchan, nstand, 2), vin, g * nchan * ninput)], wait_readers=1)
    sink.start()
    src.start()
    with pytest.raises(RuntimeError, match="xengUpchanRun returned 3"):
        up.main()
    assert len(be.held) == 2 and be.syncs == [[True, True]]
    assert not getattr(be, "waits", [])                             # (nothing was retired: neither gulp was committed)


def test_bad_gulp_shape_is_refused():
    with pytest.raises(ValueError):
        UpchanBeamform(LOG, Ring("a"), Ring("b"), nchan=1, nbeam=1, ninput=4, ntime_gulp=30, nupchan=8, backend=UpchanOracleBackend())
    with pytest.raises(ValueError):
        UpchanBeamform(LOG, Ring("a"), Ring("b"), nchan=1, nbeam=1, ninput=4, ntime_gulp=32, nupchan=8, nframe_sum=3,
                       backend=UpchanOracleBackend())


# ---------------------------------------------------------------- TbfSource
def write_tbf(path, hdr, data, hblock_size=1024):
    """triggered_dump_block.py:133-140: <I hsize, <I hblock_size, JSON header, data from hblock_size."""
    h = json.dumps(hdr).encode()
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<II', len(h), hblock_size) + h)
        fh.write(b'\0' * (hblock_size - 8 - len(h)))
        fh.write(np.ascontiguousarray(data).tobytes())


def test_tbf_round_trip_with_a_gap(tmp_path):
    """Three files: .0 and .1 contiguous (one sequence, a gulp across the file boundary), .2 after a gap (a new sequence with
    its own seq0).  The gulps come back as the same bytes; each sequence's trailing partial gulp is dropped."""
    nchan, nstand, g = 3, 2, 10
    bpt = nchan * nstand * 2
    rng = np.random.default_rng(6)
    d = [rng.integers(0, 256, (n, nchan, nstand, 2), dtype=np.uint8) for n in (25, 18, 27)]
    seqs = [7000, 7025, 9000]
    paths = []
    for k in range(3):
        hdr = source_header(nchan, nstand, 2, seq0=0, sfreq=40e6)
        hdr['seq'] = seqs[k]
        p = os.path.join(str(tmp_path), "lwa-dump-1607434049.77.tbf.%d" % k)
        write_tbf(p, hdr, d[k], hblock_size=512 + 64 * k)
        paths.append(p)
    r = Ring("tbf")
    src = TbfSource(LOG, r, paths, ntime_gulp=g)
    sink = Sink(r, g * bpt)
    th = threading.Thread(target=src.main, daemon=True)
    sink.start()
    th.start()
    th.join(20)
    sink.join(20)
    assert not th.is_alive() and not sink.is_alive()
    assert len(sink.sequences) == 2
    (h0, t0, s0), (h1, t1, s1) = sink.sequences
    assert (h0['seq0'], h1['seq0'], t0, t1) == (7000, 9000, 7000, 9000)
    a = np.concatenate([d[0], d[1]]).reshape(-1)
    assert len(s0) == 4 and b''.join(x.tobytes() for x in s0) == a[:4 * g * bpt].tobytes()
    assert len(s1) == 2 and b''.join(x.tobytes() for x in s1) == d[2].reshape(-1)[:2 * g * bpt].tobytes()
    assert h0['nchan'] == nchan and h0['sfreq'] == 40e6


# ---------------------------------------------------------------- the C entry points without a GPU
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_point_argument_checks_need_no_gpu():
    """Bad sizes and pointers are refused with INVALID_ARGUMENT before any device is touched (nothing launched); good
    arguments without a live context with INVALID_STATE."""
    ok = dict(gpu=0, ninput=8, nchan=2, ntime=64, nupchan=32, nbeam=2, nframe_sum=0)
    bad = [dict(ninput=0), dict(ninput=6), dict(nchan=0), dict(ntime=0), dict(nbeam=0), dict(nframe_sum=-1), dict(nupchan=4),
           dict(nupchan=24), dict(nupchan=128), dict(ntime=48), dict(nframe_sum=3, ntime=64), dict(nbeam=33, nupchan=32),
           dict(nbeam=17, nupchan=64)]
    for b in bad:
        a = dict(ok, **b)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanInitialize", *a.values())
        assert ei.value.status == INVALID_ARGUMENT and "Upchan" in str(ei.value), b
    run_ok = dict(i=4096, o=8192, w=16384, v=1)
    for b in (dict(i=0), dict(o=0), dict(w=0), dict(o=8200), dict(w=16392)):
        a = dict(run_ok, **b)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanRun", a['i'], a['o'], a['w'], a['v'])
        assert ei.value.status == INVALID_ARGUMENT, b
    for ntime0, in1 in ((0, 4096), (-32, 4096), (32, 0)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanRunParts", 4096, ntime0, in1, 8192, 16384, 1)
        assert ei.value.status == INVALID_ARGUMENT, (ntime0, in1)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanMark", None)
    assert ei.value.status == INVALID_ARGUMENT
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanTicketDone", 1, None)
    assert ei.value.status == INVALID_ARGUMENT
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_upchan_gpu.py covers the rest)
    ffi.call("xengUpchanDestroy")   # (no context: nothing to do)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanRun", 4096, 8192, 16384, 1)
    assert ei.value.status == INVALID_STATE
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanRunParts", 4096, 32, 4096, 8192, 16384, 1)
    assert ei.value.status == INVALID_STATE
    t, d = ctypes.c_ulonglong(), ctypes.c_int(-1)
    for name, args in (("xengUpchanMark", (ctypes.byref(t),)), ("xengUpchanWait", (1,)), ("xengUpchanTicketDone", (1, ctypes.byref(d))),
                       ("xengUpchanSync", ())):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    assert d.value == -1
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanInitialize", *ok.values())  # (valid sizes: the device is what fails here)
    assert ei.value.status not in (0, INVALID_ARGUMENT)
