"""BeamformVlbiOutput on CPU rings (no GPU), both ring implementations: the packets against a numpy restatement of the
reference's (beamform_vlbi_output_block.py:257-276: `idata[:, 0:nsel, :].transpose(2, 0, 1)` and one header per sample),
commands, the throttle, sample numbering after skipped gulps, and the C entry point's argument checks.  The packetiser call
goes to the oracle backend below; no packet is sent anywhere but to a sink (or a fake socket)."""
import ctypes
import struct
import threading

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import Beamform, BeamformVlbiOutput
from caltech_bifrost_dsp_amd.blocks import beamform_vlbi_output_block as vlbi_mod
from caltech_bifrost_dsp_amd.ring import Ring
from oracle import xeng_oracle as orc
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, GatedSource, Source, run_blocks, source_header, wait_for
from tests.test_blocks_cpu import _beam_cmds, cmd

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


class VlbiOracleBackend(OracleBackend):
    """The oracle backend plus the VLBI packetiser (xengBeamformPacketizeVoltages restated in numpy) and an immediate copy
    'stream', so that the block's in-flight path runs on system-space rings."""

    def __init__(self):
        super().__init__()
        self.packetize_calls = []
        self.copies = 0

    def beam_packetize_voltages(self, in_arr, out_arr, nchan, nbeam, ntime, beam0, nbeam_pkt, pkt_stride, server, gbe, nbeam_hdr,
                                nserver, chan0, seq0):
        self.packetize_calls.append(seq0)
        x = in_arr.numpy().view(np.uint64).reshape(nchan, nbeam, ntime)          # (bits, not values)
        out = out_arr.numpy()
        pay = np.ascontiguousarray(x[:, beam0:beam0 + nbeam_pkt, :].transpose(2, 0, 1)).view(np.uint8).reshape(ntime, -1)
        for t in range(ntime):
            s = t * pkt_stride
            out[s + 1:s + 16] = np.frombuffer(struct.pack('>5BHQ', server, gbe, nchan, nbeam_hdr, nserver, chan0, seq0 + t), np.uint8)
            out[s + 16:s + 16 + pay.shape[1]] = pay[t]
        return 0

    def copy_async(self, dst, src):
        self.copies += 1
        dst.numpy()[...] = src.numpy()
        return self.copies

    def copy_done(self, stamp):
        return True

    def copy_wait(self, stamp):
        pass


def ref_packets(idata, nsel, server, nbeam_send, nserver, chan0, seq):
    """The reference's packets of one gulp: idata cf32 [nchan][nrow][ntime] -> [bytes] per sample."""
    nchan, _, ntime = idata.shape
    pay = np.ascontiguousarray(idata[:, 0:nsel, :].transpose(2, 0, 1))
    return [struct.pack('>5BHQ', server, 1, nchan, nbeam_send, nserver, chan0, seq + t) + pay[t].tobytes() for t in range(ntime)]


def vlbi_header(nchan, nbeam, npol, seq0=0, chan0=0, system_nchan=None):
    return {'nchan': nchan, 'nbeam': nbeam, 'npol': npol, 'nbit': 32, 'complex': True, 'seq0': seq0, 'chan0': chan0,
            'system_nchan': system_nchan or 4 * nchan, 'nstand': nbeam}


def random_bits(rng, shape):
    """cf32 words with every kind of bit pattern: NaN (with payloads), +-Inf, -0.0, denormals among random words."""
    w = rng.integers(0, 2 ** 32, size=shape + (2,), dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    special = np.array([0x7FC00001, 0xFFA12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000], np.uint32)
    flat[rng.choice(flat.size, size=min(flat.size, 64), replace=False)] = np.resize(special, min(flat.size, 64))
    return w.view(np.complex64).reshape(shape)


@pytest.mark.parametrize("streaming", [True, False])
@pytest.mark.parametrize("nbeam_send", [1, 2])
def test_beamform_to_vlbi_packets(nbeam_send, streaming):
    """Beamform -> BeamformVlbiOutput: three gulps (and a short tail Beamform drops), one packet per sample, header fields,
    seq, and payload bytes = the restatement of the reference's packets = the oracle's beams.  `streaming` False: a ring
    without span_memory_outlives_release (a bifrost ring) takes the synchronous form."""
    nchan, nstand, nbeam, g = 3, 6, 4, 8
    ninput = nstand * 2
    rng = np.random.default_rng(11 + nbeam_send)
    vin = rng.integers(0, 256, (3 * g + g // 2, nchan, ninput), dtype=np.uint8)
    sfreq, chan_bw = 50e6, 23925.78125
    r0, r1 = Ring("gpu-input"), Ring("bf-output")
    if not streaming:
        r1.span_memory_outlives_release = False
    be = VlbiOracleBackend()
    bf = Beamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, backend=be)
    pk = []
    vl = BeamformVlbiOutput(LOG, r1, ntime_gulp=g, pipeline_idx=3, nbeam_send=nbeam_send, backend=be, sink=pk.append)
    vl._sleep = lambda s: None
    cmds, _, _, _ = _beam_cmds(nchan, nbeam, ninput, rng)
    hdr = source_header(nchan, nstand, 2, seq0=960, chan0=nchan * 2, sfreq=sfreq, chan_bw=chan_bw)
    hdr['system_nchan'] = nchan * 8
    bf.freqs = sfreq + chan_bw * np.arange(nchan)
    bf.process_command_strings(cmds)
    run_blocks([bf, vl], Source(r0, [(hdr, vin, g * nchan * ninput)], wait_readers=1), [])
    assert vl._streaming is streaming
    assert len(pk) == 3 * g and be.packetize_calls == [960, 960 + g, 960 + 2 * g]
    nsel = 2 * nbeam_send
    for k in range(3):
        beams = orc.beamform(vin[k * g:(k + 1) * g], bf.gains_cpu, g, nchan, ninput, nbeam)       # [nchan][nbeam][g]
        exp = ref_packets(beams, nsel, 3, nbeam_send, 8, nchan * 2, 960 + k * g)
        for t in range(g):
            p = pk[k * g + t]
            assert len(p) == 15 + nchan * nsel * 8
            assert struct.unpack('>5BHQ', p[:15]) == (3, 1, nchan, nbeam_send, 8, nchan * 2, 960 + k * g + t)
            assert p == exp[t]
            assert np.array_equal(np.frombuffer(p[15:], np.complex64).reshape(nchan, nsel), beams[:, :nsel, t])
    assert vl.stats['last_end_sample'] == 960 + 2 * g and vl.stats['curr_sample'] == 960 + 2 * g


@pytest.mark.parametrize("npol,nbeam_send", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_packets_bit_exact_by_header_npol(npol, nbeam_send):
    """Voltage spans written straight into the ring (header npol 1 or 2; the gulp is cf32 [nchan][nbeam*npol][ntime] as the
    reference sizes it): (2 // npol) * nbeam_send rows are sent, every bit pattern arrives unchanged, a short tail is ignored."""
    nchan, nbeam, g = 5, 5, 8
    rng = np.random.default_rng(npol * 10 + nbeam_send)
    nrow = nbeam * npol
    data = random_bits(rng, (4, nchan, nrow, g))
    raw = np.concatenate([data.reshape(-1).view(np.uint8), np.zeros(nchan * nrow * 8 * 3, np.uint8)])    # + a short tail
    r1 = Ring("bf-output")
    be = VlbiOracleBackend()
    pk = []
    vl = BeamformVlbiOutput(LOG, r1, ntime_gulp=g, pipeline_idx=2, nbeam_send=nbeam_send, backend=be, sink=pk.append)
    vl._sleep = lambda s: None
    hdr = vlbi_header(nchan, nbeam, npol, seq0=12345678901, chan0=300, system_nchan=nchan * 16)
    run_blocks([vl], Source(r1, [(hdr, raw, g * nchan * nrow * 8)]), [])
    nsel = (2 // npol) * nbeam_send
    assert len(pk) == 4 * g
    for k in range(4):
        exp = ref_packets(data[k], nsel, 2, nbeam_send, 16, 300, 12345678901 + k * g)
        assert pk[k * g:(k + 1) * g] == exp


def test_no_work_without_destination_and_retargeting(monkeypatch):
    """dest_ip "0.0.0.0" and no sink: no packetiser call, nothing sent.  A dest_ip / dest_port command that arrives between
    two gulps re-targets from the next gulp on (:238-254; a fake socket records what would have gone out)."""
    sent = []

    class FakeSocket:
        def __init__(self, *a):
            self.peer = None
            self.closed = False

        def connect(self, addr):
            self.peer = addr

        def send(self, b):
            sent.append((self.peer, bytes(b)))

        def close(self):
            self.closed = True
    monkeypatch.setattr(vlbi_mod.socket, "socket", FakeSocket)
    nchan, nbeam, g = 2, 2, 4
    data = random_bits(np.random.default_rng(3), (4, nchan, nbeam, g))
    r1 = Ring("bf-output")
    be = VlbiOracleBackend()
    vl = BeamformVlbiOutput(LOG, r1, ntime_gulp=g, backend=be, dest_port=4001)
    vl._sleep = lambda s: None
    gate = threading.Event()
    src = GatedSource(r1, vlbi_header(nchan, nbeam, 1), data, g * nchan * nbeam * 8, {2: gate})

    def command():
        wait_for(lambda: vl.stats.get('curr_sample') == g, "gulp 1 to be read")
        wait_for(lambda: vl.stats.get('last_end_sample') == g, "gulp 1 to be done")
        vl.process_command_strings(cmd(1, dest_ip='10.11.12.13', dest_port=4002))
        gate.set()
    th = threading.Thread(target=command, daemon=True)
    th.start()
    run_blocks([vl], src, [])
    th.join(10)
    assert be.packetize_calls == [2 * g, 3 * g] and be.copies == 2          # gulps 0 and 1: no kernel, no copy
    assert len(sent) == 2 * g and {peer for peer, _ in sent} == {('10.11.12.13', 4002)}
    for k in (2, 3):
        assert [p for _, p in sent[(k - 2) * g:(k - 1) * g]] == ref_packets(data[k], 2, 1, 1, 4, 0, k * g)
    assert vl.stats['dest_ip'] == '10.11.12.13' and vl.stats['dest_port'] == 4002
    # an unchanged command keeps the socket; back to "0.0.0.0" drops it
    vl.sock = FakeSocket()
    kept = vl.sock
    vl.process_command_strings(cmd(2, dest_ip='10.11.12.13'))
    vl._update_destination()
    assert vl.sock is kept and not kept.closed
    vl.process_command_strings(cmd(3, dest_ip='0.0.0.0'))
    vl._update_destination()
    assert vl.sock is None and kept.closed


def test_no_sink_and_no_destination_sends_nothing():
    nchan, nbeam, g = 2, 2, 4
    data = random_bits(np.random.default_rng(4), (3, nchan, nbeam, g))
    r1 = Ring("bf-output")
    be = VlbiOracleBackend()
    vl = BeamformVlbiOutput(LOG, r1, ntime_gulp=g, backend=be)
    run_blocks([vl], Source(r1, [(vlbi_header(nchan, nbeam, 1, seq0=40), data, g * nchan * nbeam * 8)]), [])
    assert be.packetize_calls == [] and be.copies == 0 and vl.sock is None
    assert vl.stats['last_end_sample'] == 40 + 2 * g


def test_throttle_requests_the_reference_sleep():
    """Bursts of 32 packets; after each, sleep burst_bits / 0.6e9 less the burst's own time (:262-274), with burst_bits
    = 32 * nchan * nsel * 2 * 32 for the last, short burst too.  The clock is injected: it advances 1 us per reading, except
    that the second burst 'takes' a whole second (no sleep after it)."""
    nchan, nbeam, g = 4, 2, 80
    data = random_bits(np.random.default_rng(5), (1, nchan, nbeam, g))
    r1 = Ring("bf-output")
    be = VlbiOracleBackend()
    pk, sleeps, now = [], [], [0.0]

    def clock():
        now[0] += 1e-6
        return now[0]

    def sink(p):
        pk.append(p)
        if len(pk) == 40:
            now[0] += 1.0               # (the second burst takes a second)
    vl = BeamformVlbiOutput(LOG, r1, ntime_gulp=g, backend=be, sink=sink)
    vl._clock, vl._sleep = clock, sleeps.append
    run_blocks([vl], Source(r1, [(vlbi_header(nchan, nbeam, 1), data, g * nchan * nbeam * 8)]), [])
    assert len(pk) == g
    burst = 32 * nchan * 2 * 2 * 32 / 0.6e9
    assert len(sleeps) == 2
    assert sleeps[0] == pytest.approx(burst - 1e-6, rel=1e-9) and sleeps[1] == pytest.approx(burst - 1e-6, rel=1e-9)


def test_skipped_gulps_are_numbered_by_position():
    """A reader that is not guaranteed and falls behind skips gulps (ring.py); the next gulp it sends is numbered by its
    place in the sequence (the reference's running count would be off by the gulps skipped).  Every packet's seq must match
    the data it carries."""
    nchan, nbeam, g, ngulp = 2, 2, 4, 12
    gulp = g * nchan * nbeam * 8
    data = np.zeros((ngulp, nchan, nbeam, g), np.complex64)
    data.real[...] = np.arange(ngulp)[:, None, None, None]                  # gulp index in every sample
    r1 = Ring("bf-output")
    r1.resize(gulp, 2 * gulp)
    be = VlbiOracleBackend()
    pk = []
    src = GatedSource(r1, vlbi_header(nchan, nbeam, 1, seq0=1000), data, gulp, {})

    def sink(p):
        if not pk:
            wait_for(lambda: src.written == ngulp, "the source to have written every gulp")
        pk.append(p)
    vl = BeamformVlbiOutput(LOG, r1, guarantee=False, ntime_gulp=g, backend=be, sink=sink)
    vl._sleep = lambda s: None
    run_blocks([vl], src, [])
    seqs = [struct.unpack('>Q', p[7:15])[0] for p in pk]
    gulps = [int(np.frombuffer(p[15:], np.complex64)[0].real) for p in pk]
    assert len(pk) < ngulp * g, "no gulp was skipped"
    assert len(pk) % g == 0 and pk
    for s, k in zip(seqs, gulps):
        assert (s - 1000) // g == k
    assert seqs == sorted(seqs) and seqs[-1] == 1000 + ngulp * g - 1


def test_reference_call_site_constructs():
    """pipeline/scripts/lwa352-pipeline.py:292-294 as written, with the ring and core names supplied."""
    log = LOG
    bf_output_ring = Ring("bf-output")
    GPU_NGULP, GSIZE, pipeline_idx, cores, etcd_client = 2, 480, 1, [3, 4], None
    op = BeamformVlbiOutput(log, iring=bf_output_ring, ntime_gulp=GPU_NGULP*GSIZE,
                                      pipeline_idx=pipeline_idx, core=cores.pop(0),
                                      guarantee=True, etcd_client=etcd_client)
    assert op.ntime_gulp == 960 and op.nbeam_send == 1 and op.dest_ip == '0.0.0.0' and op.dest_port == 10000 and op.core == 3


def test_entry_point_argument_checks_need_no_gpu():
    """Bad arguments are refused with INVALID_ARGUMENT before the context is looked at (nothing is launched); good ones
    without a live context with INVALID_STATE."""
    ok = dict(in_dev=4096, out_dev=8192, nchan=4, nbeam=4, ntime=8, beam0=0, nbeam_pkt=2, pkt_stride=80, server=1, gbe=1, nbeam_hdr=1,
              nserver=4, chan0=0, seq0=0)
    bad = [dict(in_dev=0), dict(out_dev=0), dict(in_dev=4100), dict(out_dev=8200), dict(beam0=-1), dict(beam0=3), dict(nbeam_pkt=5),
           dict(nbeam_pkt=0), dict(nchan=256, nbeam_pkt=1, pkt_stride=2064), dict(nbeam_hdr=256), dict(nserver=256), dict(server=256),
           dict(gbe=256), dict(chan0=65536), dict(chan0=-1), dict(pkt_stride=64), dict(pkt_stride=88), dict(ntime=0)]
    for b in bad:
        a = dict(ok, **b)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengBeamformPacketizeVoltages", *a.values())
        assert ei.value.status == INVALID_ARGUMENT and "PacketizeVoltages" in str(ei.value), b
    n = ctypes.c_int(-1)
    if ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0:
        return                      # (a GPU: a context may be live in this process; tests/test_vlbi_output_gpu.py covers it)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengBeamformPacketizeVoltages", *ok.values())
    assert ei.value.status == INVALID_STATE
