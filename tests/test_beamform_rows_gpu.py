"""The beamformer per (channel, beam) row: every row of every case within 1e-5 of its OWN RMS against a float64 reference
(tests/beam_route_ref.py), on rows of very different scales, on both sides of every threshold of the int8x3 route's
precision control (route totals against the rule's numpy restatement), on heavy-tailed ensembles, with dominant weights on
most of the inputs, and for the power sums per (pair, block, channel).  All three Run kernels."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from tests import beam_route_cases as cases
from tests import beam_route_ref as ref

pytestmark = pytest.mark.gpu

MODES = ["int8x3", "bf16x3", "f32"]


@pytest.fixture(scope="module")
def gpu():
    from tests import gpu_util
    assert gpu_util.ffi.device_count() >= 1
    return gpu_util


_cache = {}


def case(key, make):
    """(vin, w, float64 reference, ...) of a case, built once for the three routes.  The case itself must leave the bar
    reachable: an input-by-input complex64 accumulation stays within a third of it on every row."""
    if key not in _cache:
        made = make()
        vin, w = made[0], made[1]
        exp = ref.beams_f64(vin, w)
        ref.check_beams_rows(ref.beams_c64(vin, w), exp, ref.BEAM_RTOL / 3)
        exp.setflags(write=False)
        _cache[key] = (vin, w, exp) + tuple(made[2:])
    return _cache[key]


@contextlib.contextmanager
def beam_context(gpu, mode, ntime, nchan, ninput, nbeam, nblk=0):
    """A beamformer context on kernel route `mode` (XENG_BEAM is read by Initialize; set and restored)."""
    old = os.environ.get("XENG_BEAM")
    os.environ["XENG_BEAM"] = mode
    try:
        gpu.ffi.call("xengBeamformInitialize", 0, ninput, nchan, ntime, nbeam, nblk)
    finally:
        del os.environ["XENG_BEAM"]
        if old is not None:
            os.environ["XENG_BEAM"] = old
    try:
        yield
    finally:
        gpu.ffi.call("xengBeamformDestroy")


@contextlib.contextmanager
def device_buffers(gpu, *sizes):
    """Device buffers of these sizes, freed on every way out."""
    bufs = []
    try:
        for n in sizes:
            bufs.append(gpu.ffi.DeviceBuffer(n))
        yield bufs
    finally:
        for d in bufs:
            d.free()


def run(gpu, vin, w, do, dtype, shape, versioned=0):
    """One Run into the device buffer `do` (poisoned first) -> host copy."""
    ffi = gpu.ffi
    with device_buffers(gpu, vin.size, w.nbytes) as (di, dw):
        di.upload(vin)
        dw.upload(np.ascontiguousarray(w, dtype=np.complex64))
        ffi.call("xengMemset", do.ptr, 0x7F, do.nbytes)
        if versioned:
            ffi.call("xengBeamformRunVersioned", di.ptr, do.ptr, dw.ptr, versioned)
        else:
            ffi.call("xengBeamformRun", di.ptr, do.ptr, dw.ptr)
        ffi.call("xengBeamformSync")
        return do.download(dtype).reshape(shape)


def beams(gpu, mode, vin, w, totals=False):
    """Voltage beams complex64 [nchan][nbeam][ntime] on route `mode` (and the route totals of the weights)."""
    ntime, nchan, ninput = vin.shape
    nbeam = w.shape[1]
    with beam_context(gpu, mode, ntime, nchan, ninput, nbeam), device_buffers(gpu, nchan * nbeam * ntime * 8) as (do,):
        out = run(gpu, vin, w, do, np.complex64, (nchan, nbeam, ntime))
        if not totals:
            return out
        tot, nbf, nout = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        gpu.ffi.call("xengBeamformGetRouteInfo", ctypes.byref(tot), ctypes.byref(nbf), ctypes.byref(nout))
        return out, (tot.value, nbf.value, nout.value)


def check_totals(mode, totals, w, single=None):
    """The device's routing against the restatement's (the other two routes have no precision control: all zero)."""
    r = ref.route(w)
    if mode != "int8x3":
        assert totals == (r.tiles_total, 0, 0)
        return
    assert totals == (r.tiles_total, r.tiles_bf16, r.outlier_inputs), (totals, r.routed, [len(u) for t in r.union for u in t])
    if single is not None:
        assert totals[1:] == single


# ---- a. uneven rows -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,ninput", [(n, cases.NINPUT) for n in cases.UNEVEN] + [("per_beam", 48), ("zero_rows", 48)])
def test_uneven_rows(gpu, name, ninput, mode):
    """Rows scaled per beam and per channel over twelve decades, a 1e8 checkerboard, all-zero rows and rows whose weights
    sit on dead inputs only (exact zeros out, with the wsum offset of the int8x3 route in play)."""
    vin, w, exp = case(("uneven", name, ninput), lambda: cases.uneven_case(name, ninput))
    got = beams(gpu, mode, vin, w)
    worst, where = ref.check_beams_rows(got, exp)
    print("%s uneven %s/%d worst row %.2e at %s" % (mode, name, ninput, worst, where))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,k", [(5, 7), (33, -3)])
def test_scaling_one_row_by_a_power_of_two(gpu, b, k, mode):
    """Row b alone times 2^k: row b changes by exactly that factor and no other row by a bit."""
    vin, w, _ = case(("uneven", "per_beam", cases.NINPUT), lambda: cases.uneven_case("per_beam"))
    got = beams(gpu, mode, vin, w)
    w2 = w.copy()
    w2[:, b] *= np.float32(2.0 ** k)
    got2 = beams(gpu, mode, vin, w2)
    assert np.array_equal(got2[:, b], got[:, b] * np.float32(2.0 ** k))
    others = np.arange(w.shape[1]) != b
    assert np.array_equal(got2[:, others].view(np.uint32), got[:, others].view(np.uint32))


# ---- b. the thresholds of the rule ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("member", [0, 1])
@pytest.mark.parametrize("name", list(cases.THRESHOLDS))
def test_thresholds(gpu, name, member, multi, mode):
    """One step either side of BI_ROW_OUT, BI_TILE_OUT, BI_GAP_BINADES, BI_GUARD_BINADES, BI_SPREAD_BINADES and the 7/8 share
    of the lower-eighth entry, in a single-tile context (the totals identify the tile) and in a three-channel, two-tile one."""
    vin, w, exp, single = case(("thr", name, member, multi), lambda: cases.threshold_case(name, member, multi))
    got, totals = beams(gpu, mode, vin, w, totals=True)
    check_totals(mode, totals, w, single)
    worst, where = ref.check_beams_rows(got, exp)
    print("%s threshold %s/%d%s totals %s worst row %.2e at %s" % (mode, name, member, "/multi" if multi else "", totals, worst, where))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", cases.EXTRAS)
def test_outlier_table_edges(gpu, name, mode):
    """An input listed by some rows of a tile only, the last input, the padded part of a ragged chunk, exponent field 0."""
    vin, w, exp, single = case(("extra", name), lambda: cases.extra_case(name))
    got, totals = beams(gpu, mode, vin, w, totals=True)
    check_totals(mode, totals, w, single)
    worst, where = ref.check_beams_rows(got, exp)
    print("%s extra %s totals %s worst row %.2e at %s" % (mode, name, totals, worst, where))


# ---- c. heavy-tailed ensembles ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", range(cases.TAIL_SEEDS + cases.MIXED_SEEDS))
def test_heavy_tailed_rows(gpu, seed, mode):
    """24 ensembles of one sigma (0.5, 2, 4) and eight of mixed rows: digits with outliers beside routed tiles."""
    vin, w, exp = case(("tail", seed), lambda: cases.heavy_tail_case(seed))
    got, totals = beams(gpu, mode, vin, w, totals=True)
    check_totals(mode, totals, w)
    worst, where = ref.check_beams_rows(got, exp)
    print("%s tail seed %d totals %s worst row %.2e at %s" % (mode, seed, totals, worst, where))


# ---- d. dominant weights on most of the inputs ------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ninput,share,gain", cases.MAJORITY)
def test_majority_of_dominant_dead_weights(gpu, ninput, share, gain, mode):
    """52 % and 80 % of the inputs dead with gains x64 and x1e3: the ordinary minority alone makes the output.  (With the
    guard measured against the row's median this case stayed on the int8 digits: 1.9e-5 and 3.1e-4 of the row RMS.)"""
    vin, w, exp = case(("major", ninput, share, gain), lambda: cases.majority_case(ninput, share, gain))
    got, totals = beams(gpu, mode, vin, w, totals=True)
    worst = ref.row_errors(got, exp).max()
    print("%s majority %d/%.2f/x%g totals %s worst row %.2e" % (mode, ninput, share, gain, totals, worst))
    check_totals(mode, totals, w)
    ref.check_beams_rows(got, exp)


# ---- e. power -----------------------------------------------------------------------------------------------------------

def power_case(ntime, nchan, ninput, nbeam):
    rng = np.random.default_rng(ntime + nbeam)
    w = cases.block_weights(nchan, nbeam, ninput)
    w *= np.repeat(10.0 ** rng.uniform(-4, 4, nbeam // 2), 2).astype(np.float32)[None, :, None]
    return cases.voltages(rng, ntime, nchan, ninput), w


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ntime,nchan,ninput,nbeam,nblk", [(200, 3, 48, 4, 8), (384, 2, 64, 6, 3)])
def test_power_rows(gpu, ntime, nchan, ninput, nbeam, nblk, mode):
    """Beam pairs eight decades apart: xengBeamformIntegrate / IntegrateSingleBeam on the device's own voltages (summation
    bound), the integrated mode and its fused epilogue against the float64 power of the float64 voltages (summation +
    propagated voltage bar); time blocks inside, equal to and straddling a 128-sample work-group."""
    ffi = gpu.ffi
    vin, w, exp = case(("power", ntime, nbeam), lambda: power_case(ntime, nchan, ninput, nbeam))
    ns, npair = ntime // nblk, nbeam // 2
    npow = npair * nblk * nchan * 16
    with beam_context(gpu, mode, ntime, nchan, ninput, nbeam), \
            device_buffers(gpu, nchan * nbeam * ntime * 8, npow, nblk * nchan * 16) as (dout, dp, ds):
        got = run(gpu, vin, w, dout, np.complex64, (nchan, nbeam, ntime))
        ref.check_beams_rows(got, exp)
        ffi.call("xengBeamformIntegrate", dout.ptr, dp.ptr, ns)
        ffi.call("xengBeamformSync")
        gp = dp.download(np.float32).reshape(npair, nblk, nchan, 4)
        fig = [ref.check_power_rows(gp, got, ns, 0.0), ref.check_power_rows(gp, exp, ns, ref.BEAM_RTOL)]
        for p in range(npair):
            ffi.call("xengMemset", ds.ptr, 0x7F, ds.nbytes)
            ffi.call("xengBeamformIntegrateSingleBeam", dout.ptr, ds.ptr, ns, p)
            ffi.call("xengBeamformSync")
            gs = ds.download(np.float32).reshape(1, nblk, nchan, 4)
            fig.append(ref.check_power_rows(gs, got[:, 2 * p:2 * p + 2], ns, 0.0))
    with beam_context(gpu, mode, ntime, nchan, ninput, nbeam, nblk), device_buffers(gpu, npow) as (do,):
        tm, cn = (ctypes.c_double * 2)(), (ctypes.c_int * 2)()
        ffi.call("xengBeamformSetProfiling", 1)
        ffi.call("xengBeamformGetTimes", tm, cn)
        for version in (0, 5):
            out = run(gpu, vin, w, do, np.float32, (npair, nblk, nchan, 4), versioned=version)
            fig.append(ref.check_power_rows(out, exp, ns, ref.BEAM_RTOL))
        ffi.call("xengBeamformGetTimes", tm, cn)
        ffi.call("xengBeamformSetProfiling", 0)
        assert (cn[0], cn[1]) == ((2, 0) if mode == "int8x3" else (2, 2))     # the fused epilogue ran / Run -> Integrate
    print("%s power %s worst err / bound: Integrate %.2f (vs float64 %.2f), single %.2f, integrated %.2f, versioned %.2f" % (
        mode, (ntime, nchan, ninput, nbeam, nblk), fig[0], fig[1], max(fig[2:2 + npair]), fig[-2], fig[-1]))
