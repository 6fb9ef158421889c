"""UpchanBeamform's dual-pol mode without a GPU: the float64 restatement (tests/upchan_pol_ref.py) against the C oracle of the
live power beams (orc.beamform_integrate, BeamformSumBeams's convention); xengUpchanInitializeDualPol's argument checks; and
the block with dual_pol=True on the oracle backend (header, span size, timed weights, refusals), both ring implementations."""
import ctypes

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanBeamform
from caltech_bifrost_dsp_amd.ring import Ring
from oracle import xeng_oracle as orc
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_cpu import UpchanOracleBackend, _cal_cmds, _coeff_cmds, _expected_weights
from tests.upchan_pol_ref import upchan_dual_pol
from tests.upchan_ref import fine_freqs, upchan_beamform

INVALID_ARGUMENT = 1            # include/xeng.h XENG_STATUS_*


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


class DualPolOracleBackend(UpchanOracleBackend):
    """UpchanOracleBackend plus the dual-pol initialise, its runs served by the float64 restatement (cast to fp32)."""

    def __init__(self):
        super().__init__()
        self.inits = []

    def upchan_initialize(self, *args):
        self.inits.append('power')
        return super().upchan_initialize(*args)

    def upchan_initialize_dual_pol(self, gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum):
        self.inits.append('dual')
        rv = super().upchan_initialize(gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum)
        self.up['dual'] = True
        return rv

    def _run(self, vin, out_arr, weights, version, kind):
        u = self.up
        if not u.get('dual'):
            return super()._run(vin, out_arr, weights, version, kind)
        vin = vin.reshape(u['ntime'], u['nchan'], u['ninput'])
        w = weights.numpy().reshape(u['nchan'], u['nupchan'], u['nbeam'], u['ninput'])
        out_arr.numpy().reshape(-1).view(np.float32)[...] = upchan_dual_pol(vin, w, u['nupchan'], u['nbeam'], u['nframe_sum']).reshape(-1)
        self.runs.append((kind, version, self.block.stats.get('curr_sample') if self.block is not None else None))
        return 0


# ---------------------------------------------------------------- the restatement against the live product's oracle
@pytest.mark.parametrize("nupchan,nframe,nframe_sum,nbeam", [(8, 10, 5, 2), (16, 12, 12, 6), (32, 9, 1, 4), (64, 6, 3, 2)])
def test_restatement_matches_the_beamform_sum_oracle(nupchan, nframe, nframe_sum, nbeam):
    """The same voltages, laid out as the live beams are ([nchan*N][nbeam][nframe]: one fine channel per 'channel', one frame
    per 'sample'), through orc.beamform_integrate with ntime_sum = nframe_sum give the restatement's four products."""
    ninput, nchan = 8, 3
    rng = np.random.default_rng(nupchan + nframe + nbeam)
    vin = rng.integers(0, 256, (nframe * nupchan, nchan, ninput), dtype=np.uint8)
    w = rng.standard_normal((nchan, nupchan, nbeam, ninput)) + 1j * rng.standard_normal((nchan, nupchan, nbeam, ninput))
    got = upchan_dual_pol(vin, w, nupchan, nbeam, nframe_sum)
    assert got.shape == (nframe // nframe_sum, nbeam // 2, nchan, nupchan, 4)
    v = upchan_beamform(vin, w, nupchan, nbeam, 0)                              # [f][b][c][j]
    live = v.transpose(2, 3, 1, 0).reshape(nchan * nupchan, nbeam, nframe)
    exp = orc.beamform_integrate(live, nframe_sum)                              # [nbeam/2][nwin][nchan*N][4]
    exp = exp.transpose(1, 0, 2, 3).reshape(got.shape)
    rms = np.sqrt(np.mean(exp.astype(np.float64) ** 2))
    assert rms > 0 and np.max(np.abs(got - exp)) <= 1e-5 * rms
    assert np.allclose(got[..., 0], upchan_beamform(vin, w, nupchan, nbeam, nframe_sum)[:, 0::2])     # XX / YY: the power mode
    assert np.allclose(got[..., 1], upchan_beamform(vin, w, nupchan, nbeam, nframe_sum)[:, 1::2])


# ---------------------------------------------------------------- the C entry point without a GPU
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_dual_pol_argument_checks_need_no_gpu():
    """Odd nbeam, nframe_sum = 0 and every size xengUpchanInitialize refuses are refused with INVALID_ARGUMENT before any
    device is touched; valid sizes without a GPU fail on the device."""
    ok = dict(gpu=0, ninput=8, nchan=2, ntime=64, nupchan=32, nbeam=2, nframe_sum=2)
    bad = [dict(nbeam=1), dict(nbeam=3), dict(nbeam=31, nupchan=8), dict(nframe_sum=0), dict(nframe_sum=0, nbeam=3),
           dict(ninput=0), dict(ninput=6), dict(nchan=0), dict(ntime=0), dict(nbeam=0), dict(nframe_sum=-1), dict(nupchan=4),
           dict(nupchan=24), dict(nupchan=128), dict(ntime=48), dict(nframe_sum=3, ntime=64), dict(nbeam=34, nupchan=32),
           dict(nbeam=18, nupchan=64)]
    for b in bad:
        a = dict(ok, **b)
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengUpchanInitializeDualPol", *a.values())
        assert ei.value.status == INVALID_ARGUMENT and "Upchan" in str(ei.value), b
    if _gpu_present():
        return                      # (tests/test_upchan_pol_gpu.py covers valid sizes)
    with pytest.raises(ffi.XengError) as ei:
        ffi.call("xengUpchanInitializeDualPol", *ok.values())      # (valid sizes: the device is what fails here)
    assert ei.value.status not in (0, INVALID_ARGUMENT)


# ---------------------------------------------------------------- the block
def test_dual_pol_header_span_and_timed_load():
    """dual_pol=True: the block initialises the dual-pol context; each span is nwin * nbeam/2 * nchan * N * 16 bytes and equals
    the restatement under the weights active at its gulp (zero before the load sample, the commanded ones from it on); the
    header carries the fine-channel keys and the live power beams' keys."""
    nchan, nstand, nbeam, N, g, ns = 3, 2, 4, 8, 32, 2
    ninput = 2 * nstand
    rng = np.random.default_rng(11)
    vin = rng.integers(0, 256, (4 * g, nchan, ninput), dtype=np.uint8)
    seq0, sfreq, chan_bw = 9600, 52e6, 23925.78125
    hdr = source_header(nchan, nstand, 2, seq0=seq0, chan0=100, sfreq=sfreq, chan_bw=chan_bw)
    r0, r1 = Ring("gpu-input"), Ring("up-output")
    be = DualPolOracleBackend()
    up = UpchanBeamform(LOG, r0, r1, nchan=nchan, nbeam=nbeam, ninput=ninput, ntime_gulp=g, nupchan=N, nframe_sum=ns, backend=be,
                        dual_pol=True)
    be.block = up
    assert be.inits == ['dual'] and be.up['nbeam'] == nbeam
    freqs = fine_freqs(sfreq, chan_bw * nchan, nchan, N)
    up.freqs = freqs
    cal_cmds, cal = _cal_cmds(nchan, N, nbeam, ninput, rng)
    co_cmds, delays, amps = _coeff_cmds(nbeam, ninput, rng, load_sample=seq0 + 2 * g)
    up.process_command_strings(cal_cmds + co_cmds)
    w = _expected_weights(freqs, cal, delays, amps, nbeam)
    nwin = g // N // ns
    nout = nwin * (nbeam // 2) * nchan * N * 16
    sink = Sink(r1, nout)
    run_blocks([up], Source(r0, [(hdr, vin, g * nchan * ninput)]), [sink])
    ohdr, _, spans = sink.sequences[0]
    assert len(spans) == 4 and all(s.nbytes == nout for s in spans)
    assert [r[2] for r in be.runs] == [seq0 + k * g for k in range(4)]
    assert [r[1] for r in be.runs] == [1, 1, 2, 2]
    for k in range(4):
        wk = w if k >= 2 else np.zeros_like(w)
        exp = upchan_dual_pol(vin[k * g:(k + 1) * g], wk.astype(np.complex64), N, nbeam, ns)
        got = spans[k].view(np.float32).reshape(exp.shape)
        assert (k >= 2) == bool(np.abs(exp).max() > 0)
        assert np.allclose(got, exp, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(exp).max()))
    for key in ('nchan', 'chan0', 'sfreq', 'bw_hz', 'seq0', 'system_nchan'):
        assert ohdr[key] == hdr[key]
    assert (ohdr['nbeam'], ohdr['nstand'], ohdr['npol'], ohdr['nbit'], ohdr['complex']) == (nbeam // 2, nbeam // 2, 2, 32, True)
    assert (ohdr['nupchan'], ohdr['nframe_sum']) == (N, ns)
    assert ohdr['fine_bw_hz'] == pytest.approx(chan_bw / N)
    assert ohdr['fine_sfreq'] == pytest.approx(freqs[0, 0])


def test_single_pol_modes_keep_their_backend_calls():
    """dual_pol=False (the default) initialises as before, on a fake that has no dual-pol method."""
    be = UpchanOracleBackend()
    assert not hasattr(be, 'upchan_initialize_dual_pol')
    up = UpchanBeamform(LOG, Ring("a"), Ring("b"), nchan=1, nbeam=3, ninput=4, ntime_gulp=32, nupchan=8, nframe_sum=2, backend=be)
    assert be.up == dict(ninput=4, nchan=1, ntime=32, nupchan=8, nbeam=3, nframe_sum=2) and not up.dual_pol
    be = DualPolOracleBackend()
    UpchanBeamform(LOG, Ring("a"), Ring("b"), nchan=1, nbeam=2, ninput=4, ntime_gulp=32, nupchan=8, nframe_sum=2, backend=be, dual_pol=False)
    assert be.inits == ['power']


class _NoCalls:
    """A backend that records every attribute asked of it, and has none."""

    def __init__(self):
        self.asked = []

    def __getattr__(self, name):
        self.asked.append(name)
        raise AttributeError(name)


@pytest.mark.parametrize("nbeam,nframe_sum", [(3, 2), (1, 2), (2, 0), (5, 0)])
def test_dual_pol_refuses_odd_beams_and_voltage_mode(nbeam, nframe_sum):
    """ValueError before any backend call (gpu=0: a later check would have set the device first)."""
    be = _NoCalls()
    with pytest.raises(ValueError, match="dual_pol"):
        UpchanBeamform(LOG, Ring("a"), Ring("b"), nchan=1, nbeam=nbeam, ninput=4, ntime_gulp=32, nupchan=8, nframe_sum=nframe_sum,
                       gpu=0, backend=be, dual_pol=True)
    assert be.asked == []
