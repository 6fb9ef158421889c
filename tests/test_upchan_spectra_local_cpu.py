"""tests/upchan_spectra_local_ref.py without a GPU: the float32 emulation of upchan_spectra_kernel inside a third of the cell
bars and a tenth of the a-priori bound on every case and point that tests/test_upchan_spectra_local_gpu.py asserts; a burst
on which the old plane-RMS rule fails that correct emulation; six seeded defects that the old rule accepts and check_cells
rejects; sk_margin holding for the emulation; and the emulation giving the exact-tone data word for word, which is what
lets the GPU test assert them on the bits."""
import numpy as np
import pytest

from caltech_bifrost_dsp_amd.blocks.spectral_kurtosis import spectral_kurtosis
from tests import upchan_spectra_local_ref as S

THIRD1, THIRD2 = S.BAR1 / 3, S.BAR2 / 3


def _emu_and_ref(name, point, ninput, pfb):
    N, P, F, W, ngulp = point
    stream, info = S.spectra_case(name, N, F, ngulp, ninput)
    h = S.point_taps(N, P, pfb)
    return stream, info, h, S.emu_spectra(stream, N, W, F * N, h), S.ref_spectra(stream, N, W, h)


# ---------------------------------------------------------------- the emulation's margins, the bound, the SK margin
@pytest.mark.parametrize("ninput", S.NINPUTS)
@pytest.mark.parametrize("point", S.POINTS, ids=lambda p: "N%d-P%d-F%d-W%d-g%d" % p)
def test_emulation_within_a_third_of_the_bars_and_a_tenth_of_the_bound(point, ninput):
    """Every case, with the PFB and with the plain FFT: each S1 cell within bar1 / 3, each S2 cell within bar2 / 3, every
    output within 0.1 of bound_spectra, dead cells exactly zero, and |SK_emu - SK_ref| <= sk_margin wherever S1 > 0.

    The (case, point) pairs of S.BOUND_ONLY -- the tone at N = 64 in windows of 3 and 6 frames -- are outside a third of the
    bars (asserted too, so that the list holds nothing that does not need to be there) and are judged by the bound alone,
    here and on the GPU: the FFT's rounding of the amplitude-6 tone, about u log2(N) 6N per frame, reaches the other fine
    channels of the frame, and in three frames a cell at the noise level of the tone's own input can be that small."""
    N, P, F, W, ngulp = point
    for name in S.CASES:
        over = False
        for pfb in (False, True):
            stream, info, h, got, exp = _emu_and_ref(name, point, ninput, pfb)
            rel = S.cell_ratios(got, exp)
            r1, r2 = float(rel[:, 0].max()), float(rel[:, 1].max())
            rb = S.bound_ratio(got, exp, S.bound_spectra(stream, N, W, h))
            sk_e, sk_g = spectral_kurtosis(exp[:, 0], exp[:, 1], W), spectral_kurtosis(got[:, 0], got[:, 1], W)
            live = exp[:, 0] > 0
            rs = float((np.abs(sk_g - sk_e)[live] / S.sk_margin(sk_e[live], W)).max())
            print("emulation %s N=%d P=%d F=%d W=%d ninput=%d pfb=%d: err/cell S1 %.3g S2 %.3g, err/bound %.3g, |dSK|/margin %.3g"
                  % (name, N, P, F, W, ninput, pfb, r1, r2, rb, rs))
            assert rb <= 0.1, (name, pfb, rb)
            assert rs <= 1 and np.array_equal(np.isnan(sk_g), ~live), (name, pfb, rs)
            if (name, point) in S.BOUND_ONLY:
                over |= r1 > THIRD1 or r2 > THIRD2
            else:
                assert r1 <= THIRD1 and r2 <= THIRD2, (name, pfb, r1, r2)
            if name == "uneven":
                d = info["dead"]
                assert (got.transpose(0, 1, 3, 2, 4)[..., d] == 0).all() and np.array_equal(exp.sum(axis=(0, 1, 3)) == 0, d)
        if (name, point) in S.BOUND_ONLY and ninput == S.NINPUTS[-1]:
            assert over or _over_at_the_other_size(name, point), (name, point)


def _over_at_the_other_size(name, point):
    for pfb in (False, True):
        _, _, _, got, exp = _emu_and_ref(name, point, S.NINPUTS[0], pfb)
        rel = S.cell_ratios(got, exp)
        if rel[:, 0].max() > THIRD1 or rel[:, 1].max() > THIRD2:
            return True
    return False


def test_the_bound_is_zero_exactly_where_the_input_is_dead():
    N, P, F, W, ngulp = S.POINTS[3]
    stream, info = S.spectra_case("uneven", N, F, ngulp, 70)
    for pfb in (False, True):
        b = S.bound_spectra(stream, N, W, S.point_taps(N, P, pfb))
        dead = np.broadcast_to(info["dead"][None, None, :, None, :], b.shape)
        assert np.array_equal(b == 0, dead)
    small = S.spectra_case("steps", 4, 8, 1, 70)[0]          # no tap, no table twiddle: the voltage is exact, the chain is not
    b, exp = S.bound_spectra(small, 4, 8), S.ref_spectra(small, 4, 8)
    assert (b[exp > 0] > 0).all() and (b <= 16 * S.U * exp).all()          # ((W + 2) + 5) u of the sum at W = 8


# ---------------------------------------------------------------- the old rule fails a correct result
def test_the_plane_bar_fails_the_correct_emulation_of_a_burst():
    """One loud frame in quiet noise: the error of the emulation sits in the few cells far above the plane's RMS, so the
    largest error over the plane's RMS exceeds 1e-5 at these points while every cell is within a third of its bar."""
    for point, ninput, pfb in (((32, 4, 30, 30, 3), 70, False), ((32, 8, 30, 15, 3), 70, False), ((64, 2, 6, 3, 3), 70, False)):
        _, _, _, got, exp = _emu_and_ref("burst", point, ninput, pfb)
        plane = S.plane_ratios(got, exp)
        cells = S.check_cells(got, exp, THIRD1, THIRD2)
        print("burst %s: err / plane RMS S1 %.3g S2 %.3g; err / own cell S1 %.3g S2 %.3g" % ((point,) + plane + cells))
        assert plane[1] > 1e-5 and plane[0] <= 1e-5


# ---------------------------------------------------------------- seeded defects
def _accepted_by_planes_rejected_by_cells(got, exp):
    assert not np.array_equal(got, exp)
    plane = S.plane_ratios(got, exp)
    print("defect: err / plane RMS S1 %.3g S2 %.3g, worst err / own cell %.3g" % (plane + (S.cell_ratios(got, exp).max(),)))
    assert plane[0] <= 1e-5 and plane[1] <= 1e-5, plane
    with pytest.raises(AssertionError, match="cell"):
        S.check_cells(got, exp)
    S.check_cells(exp, exp)


def _moments(p, W):
    """[f][c][i][j] -> [w][2][c][j][i]"""
    p = p.reshape((p.shape[0] // W, W) + p.shape[1:])
    return np.stack([p.sum(axis=1), (p * p).sum(axis=1)], axis=1).transpose(0, 1, 2, 4, 3)


class _Tone:
    """The tone case (plain FFT): a third of the inputs carry an amplitude-6 tone in one fine channel over sigma 0.7 noise, the
    others ('quiet') sigma 0.4 noise.  The tone's cells are 1 / 3N of all and set the RMS of both planes."""

    def __init__(self, point, ninput=70):
        self.N, _, self.F, self.W, self.ngulp = point
        self.stream, info = S.spectra_case("tone", self.N, self.F, self.ngulp, ninput, quiet=0.4)
        self.quiet, self.j = ~info["inputs"], info["j"]
        self.p = S.frame_powers(self.stream, self.N)
        self.exp = S.ref_spectra(self.stream, self.N, self.W)
        assert np.allclose(_moments(self.p, self.W), self.exp, rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def w90():
    return _Tone((32, 1, 30, 90, 3))


@pytest.fixture(scope="module")
def w27():
    return _Tone((64, 8, 9, 27, 3))


# With 4-bit samples the S1 plane has too little range to hide a whole frame, tap or gulp of a quiet input under 1e-5 of its
# RMS (tone cell / quiet cell = 36 N / 0.42, the plane's RMS sqrt(3N) below the tone cells): the old rule did catch those
# through S1.  S2 squares that range, and the defects below are the ones of the kernel's S2 lines -- the fmaf chain, the slot
# and gulp additions of red[(N + k) ...] and acc[o + plane] -- plus a leak between lanes, which hides in both planes.
def test_defect_last_frame_left_out_of_the_s2_chain_of_quiet_inputs(w90):
    """W = 90 = 4 x 22 + 2: the slots' chains are unequal; the last frame of each window missing from S2."""
    p = w90.p.copy()
    p[w90.W - 1::w90.W][:, :, w90.quiet] = 0
    got = w90.exp.copy()
    got[:, 1] = _moments(p, w90.W)[:, 1]
    _accepted_by_planes_rejected_by_cells(got, w90.exp)


def test_defect_first_gulps_s2_partial_left_out_for_quiet_inputs(w27):
    """A window of three gulps whose first partial never reached the S2 half of the accumulator."""
    p = w27.p.copy()
    p[:w27.F][:, :, w27.quiet] = 0
    got = w27.exp.copy()
    got[:, 1] = _moments(p, w27.W)[:, 1]
    _accepted_by_planes_rejected_by_cells(got, w27.exp)


def test_defect_lane_neighbour_takes_a_millionth_of_the_loudest_cell(w90):
    """2^-20 of the loudest input's S1 and S2 added to the next input's cell (same window, channel and fine channel)."""
    exp = w90.exp
    i = int(np.argmax(exp[0, 0, 0, w90.j]))
    assert w90.quiet[i + 1]
    got = exp.copy()
    got[..., i + 1] += 2.0 ** -20 * exp[..., i]
    _accepted_by_planes_rejected_by_cells(got, exp)


def test_defect_s2_of_quiet_inputs_replaced_by_s1_squared_over_m(w27):
    got = w27.exp.copy()
    got[:, 1][..., w27.quiet] = (w27.exp[:, 0] ** 2 / w27.W)[..., w27.quiet]
    _accepted_by_planes_rejected_by_cells(got, w27.exp)


def test_defect_quiet_inputs_of_the_tail_run_keep_the_previous_windows_s2():
    """70 inputs: the run i >= 64; three windows of 27 frames, one per gulp."""
    t = _Tone((64, 1, 27, 27, 3))
    tail = t.quiet & (np.arange(70) >= 64)
    got = t.exp.copy()
    got[1:, 1][..., tail] = t.exp[:-1, 1][..., tail]
    _accepted_by_planes_rejected_by_cells(got, t.exp)


def test_defect_s2_slot_three_left_out_for_quiet_inputs(w27):
    """Frames 3, 7, 11, ... of each launch window (slot 3 of 4) missing from S2: a slot that never reached the S2 half of the
    LDS reduction."""
    p = w27.p.copy()
    slot3 = (np.arange(p.shape[0]) % w27.F) % S.NSLOT == 3
    p[np.ix_(slot3, np.arange(p.shape[1]), w27.quiet)] = 0
    got = w27.exp.copy()
    got[:, 1] = _moments(p, w27.W)[:, 1]
    _accepted_by_planes_rejected_by_cells(got, w27.exp)


def test_check_cells_zero_cells_must_be_exactly_zero():
    exp = np.ones((2, 2, 3, 8, 5))
    exp[..., 2] = 0
    got = exp.copy()
    got[1, 1, 0, 0, 2] = -0.0
    assert S.check_cells(got, exp) == (0.0, 0.0)
    got[1, 1, 0, 0, 2] = 1e-300
    with pytest.raises(AssertionError, match="cell S2"):
        S.check_cells(got, exp)
    got = exp.copy()
    got[0, 0, 1, 1, 1] = 1 + 1.5e-5                                     # (inside S2's bar, outside S1's)
    with pytest.raises(AssertionError, match="cell S1"):
        S.check_cells(got, exp)
    got = exp.copy()
    got[0, 1, 1, 1, 1] = 1 + 1.5e-5
    assert S.check_cells(got, exp)[1] > 1e-5


# ---------------------------------------------------------------- what the GPU asserts on the bits, the emulation gives on the bits
@pytest.mark.parametrize("taps", [False, True])
@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_emulation_gives_the_exact_tones_word_for_word(N, taps):
    """x[n] = a_f i^(m n): only the twiddles 1 and -i meet a non-zero value, the live bin holds N a_f, every sum is an
    integer below 2^24 times a power of two.  Windows of 16 frames within the gulp and of 256 over four gulps; with an
    integer PFB that is constant within each tap as well."""
    for W in (16, 256):
        stream, h, want = S.exact_tones(N, W, taps)
        got = S.emu_spectra(stream, N, W, S.TONE_F * N, h)
        assert got.dtype == np.float32 and S.same_bits(got, want).size == 0
        assert np.array_equal(S.ref_spectra(stream, N, W, h), want.astype(np.float64))
        assert (np.count_nonzero(want[:, 0], axis=2) <= 1).all() and want[:, 0].any(axis=2).mean() > 0.9


def test_emulation_is_covariant_bit_for_bit():
    """steps at k[i] against the same data at k = 0, and h 2^k: ldexp by 2k and 4k, on the bits."""
    N, P, F, W, ngulp = S.POINTS[1]
    stream, info = S.spectra_case("steps", N, F, ngulp, 70)
    for pfb in (False, True):
        h = S.point_taps(N, P, pfb)
        base = S.emu_spectra(info["base"], N, W, F * N, h)
        assert S.same_bits(S.emu_spectra(stream, N, W, F * N, h), S.scaled_inputs(base, info["k"])).size == 0
        if pfb:
            assert S.same_bits(S.emu_spectra(info["base"], N, W, F * N, np.ldexp(h, -9)), S.scaled_taps(base, -9)).size == 0
