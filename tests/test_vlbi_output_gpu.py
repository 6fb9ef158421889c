"""xengBeamformPacketizeVoltages and BeamformVlbiOutput on the MI355X: the kernel's packet buffer byte for byte against the
numpy restatement of the reference's packets (beamform_vlbi_output_block.py:257-276), bytes outside the packets included;
and the block on device rings beside BeamformSumBeams, its payloads bit-identical to the beamformer's own output."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import Beamform, BeamformSumBeams, BeamformVlbiOutput  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from oracle import xeng_oracle as orc  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header  # noqa: E402
from tests.test_blocks_cpu import _beam_cmds  # noqa: E402
from tests.test_vlbi_output_cpu import INVALID_ARGUMENT, INVALID_STATE, random_bits  # noqa: E402

POISON = 0xA5


def expected_buffer(x, beam0, nsel, stride, nbytes, hdr, seq0):
    """The packet buffer the kernel must leave: poison everywhere except bytes [1, 16 + payload) of each slot."""
    nchan, _, ntime = x.shape
    exp = np.full(nbytes, POISON, np.uint8)
    pay = np.ascontiguousarray(x[:, beam0:beam0 + nsel, :].transpose(2, 0, 1)).view(np.uint8).reshape(ntime, -1)
    server, gbe, nbeam_hdr, nserver, chan0 = hdr
    for t in range(ntime):
        s = t * stride
        exp[s + 1:s + 16] = np.frombuffer(struct.pack('>5BHQ', server, gbe, nchan, nbeam_hdr, nserver, chan0, seq0 + t), np.uint8)
        exp[s + 16:s + 16 + pay.shape[1]] = pay[t]
    return exp


@pytest.fixture
def context():
    ffi.call("xengBeamformInitialize", 0, 64, 4, 96, 8, 0)      # (any live context: the call takes its sizes from its arguments)
    yield
    ffi.call("xengBeamformDestroy")


@pytest.mark.parametrize("nchan,nbeam,ntime", [(96, 32, 960), (3, 5, 37), (3, 5, 38)])
@pytest.mark.parametrize("sel", ["first2", "all", "last2"])
@pytest.mark.parametrize("pad", [0, 48])
def test_kernel_bytes_against_restatement(context, nchan, nbeam, ntime, sel, pad):
    beam0, nsel = {"first2": (0, 2), "all": (0, nbeam), "last2": (nbeam - 2, 2)}[sel]
    rng = np.random.default_rng(nchan * 1000 + nbeam * 10 + ntime + beam0 + pad)
    x = random_bits(rng, (nchan, nbeam, ntime))
    stride = -(-(16 + 8 * nchan * nsel) // 16) * 16 + pad
    nbytes = ntime * stride + 256                                # (+ a guard the kernel must not touch either)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    dout = ffi.DeviceBuffer(nbytes)
    ffi.call("xengMemset", dout.ptr, POISON, nbytes)
    hdr, seq0 = (7, 1, nsel // 2 or 1, 16, 65535), (1 << 62) + 12345
    ffi.call("xengBeamformPacketizeVoltages", din.ptr, dout.ptr, nchan, nbeam, ntime, beam0, nsel, stride, hdr[0], hdr[1], hdr[2], hdr[3],
             hdr[4], seq0)
    ffi.call("xengBeamformSync")
    got = dout.download(np.uint8)
    exp = expected_buffer(x, beam0, nsel, stride, nbytes, hdr, seq0)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, "first differing bytes at %s" % bad[:8]
    assert np.array_equal(din.download(np.uint32), x.view(np.uint32).reshape(-1))        # the input is never written


def test_bad_arguments_and_missing_context_are_refused():
    din, dout = ffi.DeviceBuffer(4 * 4 * 8 * 8), ffi.DeviceBuffer(8 * 96)
    ok = dict(in_dev=din.ptr, out_dev=dout.ptr, nchan=4, nbeam=4, ntime=8, beam0=0, nbeam_pkt=2, pkt_stride=96, server=1, gbe=1,
              nbeam_hdr=1, nserver=4, chan0=0, seq0=0)
    ffi.call("xengBeamformInitialize", 0, 64, 4, 96, 8, 0)
    try:
        ffi.call("xengMemset", dout.ptr, POISON, dout.nbytes)
        for b in (dict(in_dev=din.ptr + 4), dict(out_dev=dout.ptr + 8), dict(beam0=3), dict(nbeam_pkt=5), dict(nchan=256), dict(nbeam_hdr=256),
                  dict(nserver=300), dict(server=256), dict(gbe=256), dict(chan0=65536), dict(pkt_stride=64), dict(pkt_stride=104)):
            with pytest.raises(ffi.XengError) as ei:
                ffi.call("xengBeamformPacketizeVoltages", *dict(ok, **b).values())
            assert ei.value.status == INVALID_ARGUMENT, b
        ffi.call("xengBeamformSync")
        assert np.all(dout.download(np.uint8) == POISON)                                 # nothing was launched
    finally:
        ffi.call("xengBeamformDestroy")
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengBeamformPacketizeVoltages", *ok.values())
    assert ei.value.status == INVALID_STATE


def test_vlbi_beside_sumbeams_on_device_rings():
    """Beamform -> {BeamformSumBeams, BeamformVlbiOutput} from one device ring four gulps deep, twelve gulps (spans are reused
    while VLBI gulps are in flight): every VLBI payload is bit-identical to what xengBeamformRunVersioned gives for that gulp and
    those weights, run here directly; the power sums still equal their expectation."""
    nchan, nstand, nbeam, g, ns, ngulp, nbeam_send = 4, 32, 8, 96, 24, 12, 2
    ninput = nstand * 2
    rng = np.random.default_rng(0x7b1)
    vin = rng.integers(0, 256, (ngulp * g, nchan, ninput), dtype=np.uint8)
    r0, r1, r2 = Ring("gpu-input", space="cuda"), Ring("bf-output", space="cuda"), Ring("bf-pow-output", space="cuda_host")
    bf = Beamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, gpu=0)
    sb = BeamformSumBeams(LOG, r1, r2, nchan=nchan, ntime_gulp=g, ntime_sum=ns, gpu=0)
    pk = []
    vl = BeamformVlbiOutput(LOG, r1, ntime_gulp=g, pipeline_idx=2, nbeam_send=nbeam_send, gpu=0, sink=pk.append)
    vl._sleep = lambda s: None
    sfreq, bw = 40e6, 23925.78125
    bf.freqs = sfreq + bw * np.arange(nchan)
    cmds, _, _, _ = _beam_cmds(nchan, nbeam, ninput, rng)
    bf.process_command_strings(cmds)
    s2 = Sink(r2, (nbeam // 2) * (g // ns) * nchan * 16)
    hdr = source_header(nchan, nstand, 2, seq0=4800, chan0=8, sfreq=sfreq, chan_bw=bw)
    run_blocks([bf, sb, vl], Source(r0, [(hdr, vin, g * nchan * ninput)], wait_readers=1), [s2])
    assert vl._streaming
    nsel = 2 * nbeam_send
    assert len(pk) == ngulp * g
    (_, _, sp2), = s2.sequences
    assert len(sp2) == ngulp
    din, dout = ffi.DeviceBuffer(g * nchan * ninput), ffi.DeviceBuffer(nchan * nbeam * g * 8)
    dw = ffi.DeviceBuffer(bf.gains_cpu.nbytes).upload(bf.gains_cpu)
    for k in range(ngulp):
        din.upload(vin[k * g:(k + 1) * g])
        ffi.call("xengBeamformRunVersioned", din.ptr, dout.ptr, dw.ptr, 0)
        ffi.call("xengBeamformSync")
        beams = dout.download(np.complex64).reshape(nchan, nbeam, g)
        exp = np.ascontiguousarray(beams[:, :nsel, :].transpose(2, 0, 1)).view(np.uint32)
        for t in range(g):
            p = pk[k * g + t]
            assert struct.unpack('>5BHQ', p[:15]) == (2, 1, nchan, nbeam_send, 32, 8, 4800 + k * g + t)
            assert np.array_equal(np.frombuffer(p[15:], np.uint32).reshape(nchan, nsel * 2), exp[t].reshape(nchan, nsel * 2)), (k, t)
        pexp = orc.beamform_integrate(beams, ns)
        pgot = sp2[k].view(np.float32).reshape(pexp.shape)
        assert np.all(np.isclose(pgot, pexp, rtol=1e-5, atol=1e-5 * np.abs(pexp).max())), k
    ffi.call("xengBeamformDestroy")
