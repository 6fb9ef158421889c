"""tests/upchan_local_ref.py without a GPU: seven seeded defects that the global check of the upchan GPU tests accepts and the
per-row check rejects; the float32 emulations of upchan_beamform_kernel and upchan_sum_beams_kernel within a quarter of the
row bar and inside the a-priori bounds on every case the GPU tests use; the bounds zero exactly where the reference is
structurally zero; and the emulations obeying the power-of-two covariance bit for bit."""
import numpy as np
import pytest

from tests import upchan_local_ref as L
from tests.upchan_beams_ref import beam_channelise

QUARTER = 2.5e-6            # the emulation's margin under the 1e-5 row bar


def _old_check(got, exp):
    """The check the upchan GPU tests had on its own: the largest error of the whole output against the RMS of the whole output."""
    rms = np.sqrt(np.mean(np.abs(exp) ** 2))
    err = np.max(np.abs(got.astype(exp.dtype) - exp))
    assert rms > 0 and err <= 1e-5 * rms, "max |err| %.3g = %.3g of RMS %.3g" % (err, err / rms, rms)


def _accepted_by_old_rejected_by_rows(got, exp):
    assert not np.array_equal(got, exp)
    _old_check(got, exp)
    with pytest.raises(AssertionError, match="row"):
        L.check_rows(got, exp)
    L.check_rows(exp, exp)


# ---------------------------------------------------------------- seeded defects
class _Uneven:
    """36 inputs (chunks of 16 + 16 + 4), 3 channels, N = 8, 6 beams, 12 frames; the beams of every (c, j) carry a permutation
    of 2^(20, 20, 3, -10, -14, -20): two strong rows, three weak ones (k <= -10)."""
    ninput, nchan, N, nbeam, nframe = 36, 3, 8, 6, 12

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.stream = rng.integers(0, 256, (self.nframe * self.N, self.nchan, self.ninput), dtype=np.uint8)
        self.k = np.stack([rng.permutation(np.array([20, 20, 3, -10, -14, -20], np.int32)) for _ in range(self.nchan * self.N)])
        self.k = self.k.reshape(self.nchan, self.N, self.nbeam)
        self.w = L.scale_weights(L.rand_w(rng, self.nchan, self.N, self.nbeam, self.ninput), self.k)
        self.h = rng.standard_normal(4 * self.N).astype(np.float32)
        self.weak = np.transpose(self.k, (2, 0, 1)) <= -10            # [b][c][j]

    def ref(self, w=None, h=None, **kw):
        return L.ref_beamform(self.stream, self.w if w is None else w, self.N, self.nbeam, h, **kw)


@pytest.fixture(scope="module")
def uneven():
    return _Uneven()


def test_defect_weak_rows_zeroed(uneven):
    exp = uneven.ref()
    got = exp.copy()
    got[:, uneven.weak] = 0
    _accepted_by_old_rejected_by_rows(got, exp)


def test_defect_two_weak_beams_swapped(uneven):
    exp = uneven.ref()
    got = exp.copy()
    for c in range(uneven.nchan):
        for j in range(uneven.N):
            b1, b2 = np.flatnonzero(uneven.weak[:, c, j])[:2]
            got[:, b1, c, j], got[:, b2, c, j] = exp[:, b2, c, j], exp[:, b1, c, j]
    _accepted_by_old_rejected_by_rows(got, exp)


def test_defect_weak_row_takes_a_millionth_of_the_strongest(uneven):
    """+ 2^-20 of the strongest row of the same (c, j)"""
    exp = uneven.ref()
    strongest = np.argmax(uneven.k, axis=2)                              # [c][j]
    leak = np.take_along_axis(exp, strongest[None, None], axis=1)       # [f][1][c][j]
    got = np.where(uneven.weak[None], exp + 2.0 ** -20 * leak, exp)
    _accepted_by_old_rejected_by_rows(got, exp)


def test_defect_last_partial_chunk_left_out_for_weak_rows(uneven):
    exp = uneven.ref()
    w = uneven.w.copy()
    w[..., 32:] = 0
    got = np.where(uneven.weak[None], uneven.ref(w), exp)
    _accepted_by_old_rejected_by_rows(got, exp)


def test_defect_weak_rows_power_window_not_cleared(uneven):
    exp = uneven.ref(nframe_sum=3)
    got = exp.copy()
    got[1:] += np.where(uneven.weak[None], exp[:-1], 0)
    _accepted_by_old_rejected_by_rows(got, exp)


@pytest.mark.parametrize("dual", [False, True])
def test_defect_oldest_tap_dropped_for_weak_rows(uneven, dual):
    exp = uneven.ref(h=uneven.h, nframe_sum=3 * dual, dual=dual)
    h = uneven.h.copy()
    h[:uneven.N] = 0
    bad = uneven.ref(h=h, nframe_sum=3 * dual, dual=dual)
    weak = (uneven.weak[0::2] & uneven.weak[1::2])[..., None] if dual else uneven.weak
    got = np.where(weak[None], bad, exp)
    _accepted_by_old_rejected_by_rows(got, exp)


def test_defect_quiet_y_crossed_with_the_next_pair():
    """UpchanSumBeams, X loud and Y quiet: the cross terms of pair p formed with the Y of pair p + 1."""
    N, W = 8, 32
    v, _ = L.sum_beams_case("loud_x_quiet_y", N, False)
    exp = L.ref_sum_beams(v, N, W)
    V = beam_channelise(v, N, None, 0, v.shape[-1])                      # [f][c][b][j]
    X, Y = V[:, :, 0::2], np.roll(V[:, :, 1::2], -1, axis=2)
    xy = (X * np.conj(Y)).reshape((V.shape[0] // W, W) + X.shape[1:]).sum(axis=1).transpose(0, 2, 1, 3)
    got = exp.copy()
    got[..., 2], got[..., 3] = xy.real, xy.imag
    _accepted_by_old_rejected_by_rows(got, exp)


def test_check_rows_zero_rows_must_be_exactly_zero():
    exp = np.ones((4, 2, 3, 8))
    exp[:, 1] = 0
    got = exp.copy()
    got[2, 1, 0, 0] = -0.0
    L.check_rows(got, exp)
    got[2, 1, 0, 0] = 1e-300
    with pytest.raises(AssertionError, match="row"):
        L.check_rows(got, exp)
    pair = np.ones((4, 2, 3, 8, 4))
    pair[:, 0, ..., 1:] = 0                                              # (YY zero: the cross terms must be zero too)
    got = pair.copy()
    got[1, 0, 1, 1, 3] = 1e-300
    with pytest.raises(AssertionError, match="row"):
        L.check_rows(got, pair)


# ---------------------------------------------------------------- the emulation's margins, the bounds
@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("mode,N,nbeam,nframe,ns", L.beamform_points())
def test_beamform_emulation_margins(mode, N, nbeam, nframe, ns, pfb):
    """Both gulps of every row-bar case at every shape the GPU test asserts: the emulation within a quarter of the bar of each row and inside the bound; the tone
    case against the bound alone; zero rows exactly zero."""
    worst_row = worst_bound = 0.0
    for name in L.BEAMFORM_CASES + ("tone",):
        stream, w, h = L.beamform_case(name, N, nbeam, pfb, nframe=nframe)
        ntime = stream.shape[0] // 2
        for g in range(2):
            a = dict(h=h, start=g * ntime, ntime=ntime, nframe_sum=ns, dual=mode == "dual")
            exp, got = L.ref_beamform(stream, w, N, nbeam, **a), L.emu_beamform(stream, w, N, nbeam, **a)
            bound = L.bound_beamform(stream, w, N, nbeam, **a)
            worst_bound = max(worst_bound, L.bound_ratio(got, exp, bound))
            if name != "tone":
                worst_row = max(worst_row, L.check_rows(got, exp, QUARTER))
            if name == "zero_beam":
                assert ((got[:, 0, ..., 1:] if mode == "dual" else got[:, 1]) == 0).all()
            if name == "zero_chan":
                assert (got[:, :, 1] == 0).all()
    print("emulation %s N=%d nbeam=%d nframe=%d ns=%d pfb=%d: worst err/rowRMS %.3g, worst err/bound %.3g" % (mode, N, nbeam, nframe, ns, pfb, worst_row, worst_bound))
    assert worst_bound <= 1


@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("span", [False, True])
@pytest.mark.parametrize("N", [8, 64])
def test_sum_beams_emulation_margins(N, span, pfb):
    F = L.SUM_NTIME // N
    W = 2 * F if span else F // 2
    worst_row = worst_bound = 0.0
    for name in L.SUM_CASES:
        if name == "burst" and pfb:
            continue
        v, h = L.sum_beams_case(name, N, pfb)
        exp, got = L.ref_sum_beams(v, N, W, h, 1, 2), L.emu_sum_beams(v, N, W, L.SUM_NTIME, h, 1, 2)
        worst_bound = max(worst_bound, L.bound_ratio(got, exp, L.bound_sum_beams(v, N, W, h, 1, 2)))
        worst_row = max(worst_row, L.check_rows(got, exp, QUARTER))
        if name == "zero_beam":
            assert (got[:, 0, ..., 1:] == 0).all() and (got[:, 0, ..., 0] > 0).all()
    print("emulation SumBeams N=%d W=%d pfb=%d: worst err/rowRMS %.3g, worst err/bound %.3g" % (N, W, pfb, worst_row, worst_bound))
    assert worst_bound <= 1


@pytest.mark.parametrize("mode,ns", [("voltage", 0), ("power", 3), ("dual", 3)])
def test_bounds_are_zero_exactly_where_the_reference_is_structurally_zero(mode, ns):
    N, nbeam = 8, 6
    for name in ("zero_beam", "zero_chan"):
        stream, w, h = L.beamform_case(name, N, nbeam, True)
        a = dict(h=h, start=0, ntime=stream.shape[0] // 2, nframe_sum=ns, dual=mode == "dual")
        bound, exp = L.bound_beamform(stream, w, N, nbeam, **a), L.ref_beamform(stream, w, N, nbeam, **a)
        zero = np.zeros(bound.shape, bool)
        if name == "zero_chan":
            zero[:, :, 1] = True
        elif mode == "dual":
            zero[:, 0, ..., 1:] = True                                  # (beam 1 is the Y of pair 0: YY and both cross terms)
        else:
            zero[:, 1] = True
        assert np.array_equal(bound == 0, zero) and (exp[zero] == 0).all()
        assert (bound[~zero] > np.abs(exp[~zero]) * 2.0 ** -26).all()          # (and elsewhere no smaller than a rounding of the value)
    v, h = L.sum_beams_case("zero_beam", N, True)
    bound = L.bound_sum_beams(v, N, 32, h)
    zero = np.zeros(bound.shape, bool)
    zero[:, 1, ..., 1:] = True
    assert np.array_equal(bound == 0, zero)


# ---------------------------------------------------------------- the emulation obeys the covariance bit for bit
@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("mode,ns", [("voltage", 0), ("power", 3), ("dual", 3)])
def test_beamform_emulation_is_covariant_bit_for_bit(mode, ns, pfb):
    N, nbeam, ninput, nchan, nframe = 8, 6, 36, 3, 12
    rng = np.random.default_rng(77 + ns + pfb)
    stream = rng.integers(0, 256, (nframe * N, nchan, ninput), dtype=np.uint8)
    w = L.rand_w(rng, nchan, N, nbeam, ninput)
    h = rng.standard_normal(4 * N).astype(np.float32) if pfb else None
    k = L.uneven_k(rng, (nchan, N, nbeam))
    dual = mode == "dual"
    assert L.in_range(L.ref_beamform(stream, w, N, nbeam, h, nframe_sum=ns, dual=dual), L.term_magnitudes(stream, w, N, nbeam, h))
    base = L.emu_beamform(stream, w, N, nbeam, h, nframe_sum=ns, dual=dual)
    got = L.emu_beamform(stream, L.scale_weights(w, k), N, nbeam, h, nframe_sum=ns, dual=dual)
    assert L.same_bits(got, L.scaled_beamform(base, k, ns, dual)).size == 0
    perm = L.pair_perm(rng, nbeam) if dual else rng.permutation(nbeam)
    got = L.emu_beamform(stream, np.ascontiguousarray(w[:, :, perm]), N, nbeam, h, nframe_sum=ns, dual=dual)
    assert L.same_bits(got, base[:, perm[::2] // 2] if dual else base[:, perm]).size == 0


@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("span", [False, True])
def test_sum_beams_emulation_is_covariant_bit_for_bit(span, pfb):
    N = 8
    F = L.SUM_NTIME // N
    W = 2 * F if span else F // 2
    rng = np.random.default_rng(5 + span + 2 * pfb)
    v = L.rand_beams(rng, L.SUM_NCHAN, L.SUM_NBEAM, L.SUM_NGULP * L.SUM_NTIME)
    h = rng.standard_normal(4 * N).astype(np.float32) if pfb else None
    k = L.uneven_k(rng, (L.SUM_NCHAN, L.SUM_NBEAM))
    base = L.emu_sum_beams(v, N, W, L.SUM_NTIME, h, 1, 2)
    got = L.emu_sum_beams(L.scale_beams(v, k), N, W, L.SUM_NTIME, h, 1, 2)
    assert L.same_bits(got, L.scaled_sum_beams(base, k, 1, 2)).size == 0
    if pfb:
        got = L.emu_sum_beams(v, N, W, L.SUM_NTIME, 8 * h, 1, 2)
        assert L.same_bits(got, np.ldexp(base, 6)).size == 0
    else:                                                               # one window's samples by 2^-13: that window alone
        vw = v.copy()
        vw[..., W * N:2 * W * N] = L.scale_beams(v[..., W * N:2 * W * N], np.full(k.shape, -13, np.int32))
        want = base.copy()
        want[1] = np.ldexp(base[1], -26)
        assert L.same_bits(L.emu_sum_beams(vw, N, W, L.SUM_NTIME, None, 1, 2), want).size == 0
