"""The restatement of the beamformer's precision control (tests/beam_route_ref.py) against a one-row-at-a-time statement
of the same rule, on the constructed threshold cases and on random rows; the CPU emulation of the int8x3 arithmetic on
those cases (the error of the RULE, apart from any kernel); and the check that ordinary weights route nowhere.  No GPU."""
import struct

import numpy as np
import pytest

from tests import beam_route_cases as cases
from tests import beam_route_ref as ref


def fexp(x):
    return (struct.unpack("<I", struct.pack("<f", float(x)))[0] >> 23) & 0xFF


def brute_row(row, spread_guard=True):
    """One row, one entry at a time -> (E, outlier inputs, m, guard verdict)."""
    a = [max(abs(np.float32(z.real)), abs(np.float32(z.imag))) for z in row]
    ex = [fexp(v) for v in a]
    exa = np.array(ex)
    for E in range(256):
        if (exa > E).sum() <= ref.ROW_OUT and not ((exa > E) & (exa <= E + ref.GAP_BINADES)).any():
            break
    outs = [i for i, e in enumerate(ex) if e > E]
    m = max([a[i] for i in range(len(a)) if ex[i] <= E], default=np.float32(0))
    nz = sorted((e for e in ex if e >= 1), reverse=True)
    guard = False
    if nz:
        med = nz[-(-len(nz) // 2) - 1]               # ceil(n / 2) entries lie at or above the median's bucket,
        low = nz[-(-ref.LOW_NUM * len(nz) // ref.LOW_DEN) - 1]      # ceil(7 n / 8) at or above the lower-eighth entry's
        guard = bool(fexp(m) - med > ref.GUARD_BINADES or (spread_guard and med - low > ref.SPREAD_BINADES))
    return E, outs, np.float32(m), guard


def brute(w, spread_guard=True):
    nchan, nbeam, ninput = w.shape
    nbf = nout = 0
    rows = {}
    for c in range(nchan):
        for t in range((nbeam + 31) // 32):
            union, routed = set(), False
            for b in range(32 * t, min(32 * t + 32, nbeam)):
                rows[c, b] = brute_row(w[c, b], spread_guard)
                union |= set(rows[c, b][1])
                routed |= rows[c, b][3]
            routed |= len(union) > ref.TILE_OUT
            nbf += routed
            nout += 0 if routed else len(union)
    return rows, nbf, nout


def assert_same(w, spread_guard=True):
    r = ref.route(w, spread_guard)
    rows, nbf, nout = brute(w, spread_guard)
    for (c, b), (E, outs, m, guard) in rows.items():
        assert r.E[c, b] == E and list(np.flatnonzero(r.is_out[c, b])) == outs, (c, b)
        assert r.m[c, b] == m and bool(r.guard[c, b]) == guard, (c, b)
    assert (r.tiles_bf16, r.outlier_inputs) == (nbf, nout)
    return r


@pytest.mark.parametrize("name", list(cases.THRESHOLDS))
@pytest.mark.parametrize("member", [0, 1])
def test_threshold_cases(name, member):
    """One step either side of each threshold: the expected totals, the brute-force rule, and the emulated int8x3
    arithmetic per row against the float64 reference."""
    vin, w, tot = cases.threshold_case(name, member)
    r = assert_same(w)
    assert (r.tiles_bf16, r.outlier_inputs) == tot
    exp = ref.beams_f64(vin, w)
    ref.check_beams_rows(ref.beams_c64(vin, w), exp, ref.BEAM_RTOL / 3)
    print(name, member, "emulated int8x3 worst row %.2e" % ref.check_beams_rows(ref.int8x3_beams(vin, w, r), exp)[0])
    vin, w, _ = cases.threshold_case(name, member, multi=True)
    r = assert_same(w)
    a, b = cases.THRESHOLDS[name][member], cases.THRESHOLDS[name][1 - member]
    assert (r.tiles_bf16, r.outlier_inputs) == (a[0] + b[0], a[1] + b[1])
    assert r.routed[1].sum() == 0 and r.routed[0, 1] == 0 and r.routed[2, 0] == 0


@pytest.mark.parametrize("name", cases.EXTRAS)
def test_extra_cases(name):
    vin, w, tot = cases.extra_case(name)
    r = assert_same(w)
    assert (r.tiles_bf16, r.outlier_inputs) == tot
    exp = ref.beams_f64(vin, w)
    ref.check_beams_rows(ref.beams_c64(vin, w), exp, ref.BEAM_RTOL / 3)
    ref.check_beams_rows(ref.int8x3_beams(vin, w, r), exp)


def test_random_rows_against_the_brute_force_rule():
    """A few thousand rows of every kind: smooth and heavy-tailed, with zeros, denormals, stand-out entries, few inputs."""
    rng = np.random.default_rng(5)
    for ninput, nbeam in ((16, 70), (40, 64), (192, 33)):
        for sigma in (0.3, 1.0, 3.0, 8.0):
            w = (rng.standard_normal((6, nbeam, ninput)) + 1j * rng.standard_normal((6, nbeam, ninput)))
            w *= np.exp(sigma * rng.standard_normal(w.shape))
            w[rng.random(w.shape) < 0.1] = 0
            w[rng.random(w.shape) < 0.02] = 1e-41
            k = rng.integers(0, 14, (6, nbeam))            # 0..13 stand-out entries per row, 2^1 .. 2^9 above
            for c in range(6):
                for b in range(nbeam):
                    w[c, b, rng.choice(ninput, k[c, b], replace=False)] *= 2.0 ** rng.integers(1, 10)
            w[0, 0] = 0
            assert_same(w.astype(np.complex64))
            assert_same(w.astype(np.complex64), False)


@pytest.mark.parametrize("kind", ["block", "uniform"])
@pytest.mark.parametrize("ninput", [64, 192, 704])
def test_ordinary_weights_route_nowhere(kind, ninput):
    """More than 10^4 rows each of the Beamform block's weights and of the benchmark's uniform(-17, 17) weights: no
    outlier, no routed tile, and both of the guard's spreads (maximum to median, median to lower-eighth entry) a binade
    short of their thresholds."""
    nchan, nbeam = 8, 1312                                  # 10496 rows, 41 tiles per channel
    if kind == "block":
        w = cases.block_weights(nchan, nbeam, ninput, seed=ninput)
    else:
        rng = np.random.default_rng(ninput)
        w = (rng.uniform(-17, 17, (nchan, nbeam, ninput)) + 1j * rng.uniform(-17, 17, (nchan, nbeam, ninput))).astype(np.complex64)
    r = ref.route(w)
    top, bulk = ref.exponent_field(r.m) - r.Emed, r.Emed - r.Elow
    print(kind, ninput, "m to median %d binades (guard %d), median to lower eighth %d (guard %d)" % (
        top.max(), ref.GUARD_BINADES, bulk.max(), ref.SPREAD_BINADES))
    assert (r.tiles_bf16, r.outlier_inputs) == (0, 0)
    assert top.max() < ref.GUARD_BINADES and bulk.max() < ref.SPREAD_BINADES        # a binade to spare


def test_majority_of_dominant_dead_weights_is_routed():
    """The hole of the median guard alone: dominant weights on more than half of a row's inputs.  The median sits among
    them and nothing is routed; the lower-eighth entry still sits among the ordinary weights at 52 % and at 80 %."""
    for ninput, share, gain in cases.MAJORITY:
        vin, w = cases.majority_case(ninput, share, gain)
        old, new = ref.route(w, False), ref.route(w)
        assert old.tiles_bf16 == 0 and new.tiles_bf16 == new.tiles_total
        exp = ref.beams_f64(vin, w)
        ref.check_beams_rows(ref.beams_c64(vin, w), exp, ref.BEAM_RTOL / 3)
        was = ref.row_errors(ref.int8x3_beams(vin, w, old), exp).max()
        print(ninput, share, gain, "median guard alone: emulated worst row %.2e" % was)
        if ninput == 192 and gain == 1e3:
            assert was > ref.BEAM_RTOL                       # what the old rule cost
        ref.check_beams_rows(ref.int8x3_beams(vin, w, new), exp)


@pytest.mark.parametrize("name", cases.UNEVEN)
def test_uneven_rows_emulated(name):
    vin, w = cases.uneven_case(name)
    exp = ref.beams_f64(vin, w)
    ref.check_beams_rows(ref.beams_c64(vin, w), exp, ref.BEAM_RTOL / 3)
    ref.check_beams_rows(ref.int8x3_beams(vin, w), exp)
    if name == "zero_rows":
        assert not exp[:, [3, 5, 32, 33]].any() and exp[:, 4].any()


def test_heavy_tails_emulated():
    for seed in range(cases.TAIL_SEEDS + cases.MIXED_SEEDS):
        vin, w = cases.heavy_tail_case(seed)
        exp = ref.beams_f64(vin, w)
        ref.check_beams_rows(ref.beams_c64(vin, w), exp, ref.BEAM_RTOL / 3)
        ref.check_beams_rows(ref.int8x3_beams(vin, w), exp)


def test_check_power_rows_catches_a_weak_pair():
    """The per-(pair, block, channel) bound sees an error in a weak pair that the global measure cannot."""
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((2, 4, 48)) + 1j * rng.standard_normal((2, 4, 48)))
    v[:, 2:] *= 1e-4
    v = v.astype(np.complex64)
    p = ref.power_f64(v, 12)
    assert ref.check_power_rows(p.astype(np.float32), v, 12, 0.0) <= 1.0
    bad = p.copy()
    bad[1] *= 1 + 1e-4
    assert np.all(np.isclose(bad, p, rtol=1e-5, atol=1e-5 * np.abs(p).max()))      # the old global measure passes it
    with pytest.raises(AssertionError):
        ref.check_power_rows(bad.astype(np.float32), v, 12, ref.BEAM_RTOL)
