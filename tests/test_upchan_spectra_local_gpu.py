"""upchan_spectra_kernel on the MI355X, every cell on a scale of its own (tests/upchan_spectra_local_ref.py).

The bounded part: on inputs of uneven scale with dead ones, a burst, a tone and power-of-two steps, at the fourteen points of
test_against_the_float64_restatement with 70 and 130 inputs, every S1 within 1e-5 and every S2 within 2e-5 of its own float64
value, every output inside an a-priori bound, dead cells exactly zero; the spectral kurtosis of every cell within what the two
bars allow, and its flags those of the float64 sums away from the limits.  The worst figures are printed (DESIGN.md records
them).

The exact part, on the bits: scaling an input's samples or the taps by 2^k scales S1 by 2^2k and S2 by 2^4k; permuting
inputs, coarse channels or whole windows permutes the outputs; x -> -x changes nothing; tones that meet only the twiddles 1
and -i equal an int64 restatement at N = 8 to 64; and at W = 1 S2 is the square of the device's own S1.  The kernel is a
fixed-order fp32 sum per cell, so any leak between lanes, slots, windows or planes breaks these, however quiet the cell.
No wall-clock assertions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import sk_flags, sk_limits, spectral_kurtosis  # noqa: E402
from oracle import xeng_oracle as orc  # noqa: E402
from tests import upchan_spectra_local_ref as S  # noqa: E402
from tests.test_upchan_spectra_gpu import US  # noqa: E402

POINT_IDS = ["N%d-P%d-F%d-W%d-g%d" % p for p in S.POINTS]
ONE_PER_N = [(8, 8, 12, 12, 3), (16, 8, 10, 20, 4), (32, 8, 30, 15, 3), (64, 2, 6, 3, 3)]


@pytest.fixture
def us():
    yield US
    ffi.call("xengUpchanSpectraDestroy")


def _device(us, stream, N, F, W, h=None):
    """The stream's gulps of F frames through a fresh context: f32 [nwin][2][nchan][N][ninput] (US.run checks the poison
    guard past the output)."""
    T, nchan, ninput = stream.shape
    ngulp = T // (F * N)
    if h is not None:
        h = np.ascontiguousarray(h, np.float32)
    u = us(ninput, nchan, F * N, N, W, ngulp=ngulp, ntap=1 if h is None else h.size // N, h=h)
    outs = u.run(stream)
    assert len(outs) == (ngulp // (W // F) if W > F else ngulp)
    return np.concatenate(outs)


def _assert_same_bits(got, want, what):
    d = S.same_bits(got, want)
    assert d.size == 0, "%s: words differ, the first at %s" % (what, d.tolist())


# ---------------------------------------------------------------- the cell bars and the a-priori bound
@pytest.mark.parametrize("name", S.CASES)
@pytest.mark.parametrize("ninput", S.NINPUTS)
@pytest.mark.parametrize("point", S.POINTS, ids=POINT_IDS)
def test_cells_within_their_own_bars_and_bound(us, point, ninput, name):
    """Each case on consecutive gulps, with the PFB (the point's P taps, 4 where it has one) and with the plain FFT:
    check_cells, a ratio <= 1 to bound_spectra, exact zeros for the dead inputs and the dead half channel.

    The tone at N = 64 in windows of 3 and 6 frames (S.BOUND_ONLY) is judged by the bound alone: the float32 emulation is not
    inside a third of the bars there (tests/test_upchan_spectra_local_cpu.py) -- the FFT's rounding of the amplitude-6 tone
    reaches the other fine channels of its frames, and three frames leave cells at the noise level that are that small."""
    N, P, F, W, ngulp = point
    stream, info = S.spectra_case(name, N, F, ngulp, ninput)
    for pfb in (False, True):
        h = S.point_taps(N, P, pfb)
        got, exp = _device(us, stream, N, F, W, h), S.ref_spectra(stream, N, W, h)
        rel = S.cell_ratios(got, exp)
        rb = S.bound_ratio(got, exp, S.bound_spectra(stream, N, W, h))
        sk_r, sk_d = spectral_kurtosis(exp[:, 0], exp[:, 1], W), spectral_kurtosis(got[:, 0], got[:, 1], W)
        live = exp[:, 0] > 0
        rs = (np.abs(sk_d - sk_r)[live] / S.sk_margin(sk_r[live], W)).max() if W > 1 else 0.0
        print("UpchanSpectra %s N=%d P=%d F=%d W=%d ninput=%d pfb=%d: err/cell S1 %.3g S2 %.3g, err/bound %.3g, |dSK|/margin %.3g"
              % (name, N, P, F, W, ninput, pfb, rel[:, 0].max(), rel[:, 1].max(), rb, rs))
        if (name, point) not in S.BOUND_ONLY:
            S.check_cells(got, exp)
        assert rb <= 1, "%s pfb %d: worst |err| / bound = %.3g" % (name, pfb, rb)
        if name == "uneven":
            assert (got.transpose(0, 1, 3, 2, 4)[..., info["dead"]] == 0).all()


# ---------------------------------------------------------------- exact power-of-two covariance
def _terms_in_range(*streams_and_taps):
    """Every p and p^2 term and every output of the float64 reference in RANGE, for (stream, N, W, h) tuples."""
    for stream, N, W, h in streams_and_taps:
        p = S.frame_powers(stream, N, h)
        if not S.in_range(p, p * p, S.ref_spectra(stream, N, W, h)):
            return False
    return True


@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("point", S.POINTS, ids=POINT_IDS)
def test_scaling_inputs_by_powers_of_two_is_exact(us, point, pfb):
    """Samples in -1..1 times 2^k[i], k in {0, 1, 2} per input, against the same samples at k = 0: S1 = ldexp(S1, 2 k[i]),
    S2 = ldexp(S2, 4 k[i]), on the bits, 130 inputs."""
    N, P, F, W, ngulp = point
    stream, info = S.spectra_case("steps", N, F, ngulp, S.NINPUTS[1])
    h = S.point_taps(N, P, pfb)
    assert _terms_in_range((info["base"], N, W, h), (stream, N, W, h))
    base, got = _device(us, info["base"], N, F, W, h), _device(us, stream, N, F, W, h)
    _assert_same_bits(got, S.scaled_inputs(base, info["k"]), "inputs scaled by 2^k[i]")
    assert set(info["k"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("point", [p for p in S.POINTS if p[1] > 1], ids=[i for p, i in zip(S.POINTS, POINT_IDS) if p[1] > 1])
def test_scaling_the_taps_by_a_power_of_two_is_exact(us, point):
    """h 2^k for the widest k either way that keeps every p and p^2 term and every output of the float64 reference in
    [2^-100, 2^100] (at least +-8): S1 = ldexp(S1, 2k), S2 = ldexp(S2, 4k), on the bits.  The uneven case, 70 inputs."""
    N, P, F, W, ngulp = point
    stream, _ = S.spectra_case("uneven", N, F, ngulp, S.NINPUTS[0])
    h = S.point_taps(N, P, True)
    p, out = S.frame_powers(stream, N, h), S.ref_spectra(stream, N, W, h)
    hi, lo = [], []
    for a, mult in ((p, 2), (p * p, 4), (out[:, 0], 2), (out[:, 1], 4)):
        nz = a[a > 0]
        hi.append((np.log2(S.RANGE[1]) - np.log2(nz.max())) / mult)
        lo.append((np.log2(S.RANGE[0]) - np.log2(nz.min())) / mult)
    kmax, kmin = int(np.floor(min(hi))), int(np.ceil(max(lo)))
    assert kmax >= 8 and kmin <= -8, (kmin, kmax)
    base = _device(us, stream, N, F, W, h)
    for k in (kmin, kmax):
        hk = np.ldexp(h, k).astype(np.float32)
        assert np.array_equal(hk.astype(np.float64), h.astype(np.float64) * 2.0 ** k) and _terms_in_range((stream, N, W, hk))
        _assert_same_bits(_device(us, stream, N, F, W, hk), S.scaled_taps(base, k), "taps scaled by 2^%d" % k)
    print("taps 2^k exact at N=%d P=%d W=%d for k = %d and %d" % (N, P, W, kmin, kmax))


@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("point", ONE_PER_N, ids=lambda p: "N%d-W%d" % (p[0], p[3]))
def test_permuting_inputs_and_channels_permutes_the_outputs(us, point, pfb):
    """130 inputs of uneven scale permuted across the 64-lane runs, and the coarse channels rotated: the same bits elsewhere."""
    N, P, F, W, ngulp = point
    stream, _ = S.spectra_case("uneven", N, F, ngulp, S.NINPUTS[1])
    h = S.point_taps(N, P, pfb)
    rng = np.random.default_rng([N, int(pfb)])
    ip, cp = rng.permutation(S.NINPUTS[1]), np.array([2, 0, 1])
    assert (ip[:64] >= 64).any() and (ip[128:] < 128).any()
    base = _device(us, stream, N, F, W, h)
    got = _device(us, np.ascontiguousarray(stream[:, :, ip]), N, F, W, h)
    _assert_same_bits(got, base[..., ip], "inputs permuted")
    got = _device(us, np.ascontiguousarray(stream[:, cp]), N, F, W, h)
    _assert_same_bits(got, base[:, :, cp], "channels permuted")


@pytest.mark.parametrize("point", [(8, 1, 12, 4, 3), (16, 2, 10, 5, 3), (32, 8, 30, 15, 3), (64, 2, 6, 3, 3)], ids=lambda p: "N%d-W%d" % (p[0], p[3]))
def test_permuting_the_windows_of_a_gulp_permutes_the_output_windows(us, point):
    """Plain FFT, W | F: the windows of every gulp of the burst case reversed, one loud window among them."""
    N, _, F, W, ngulp = point
    stream, info = S.spectra_case("burst", N, F, ngulp, S.NINPUTS[0])
    wpg = F // W
    base = _device(us, stream, N, F, W)
    sw = stream.reshape((ngulp, wpg, W * N) + stream.shape[1:])[:, ::-1].reshape(stream.shape)
    got = _device(us, np.ascontiguousarray(sw), N, F, W)
    want = base.reshape((ngulp, wpg) + base.shape[1:])[:, ::-1].reshape(base.shape)
    _assert_same_bits(got, want, "windows reversed within each gulp")
    loud = info["frame"] // W
    assert base[loud, 0].mean() > 2 * np.delete(base[:, 0], loud, axis=0).mean()


@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("point", ONE_PER_N, ids=lambda p: "N%d-W%d" % (p[0], p[3]))
def test_negating_the_samples_changes_no_bit(us, point, pfb):
    """x -> -x on the tone case (samples in -7..7): every fp32 operation of the chain is odd or even in its inputs."""
    N, P, F, W, ngulp = point
    stream, _ = S.spectra_case("tone", N, F, ngulp, S.NINPUTS[0])
    re, im = orc.decode(stream)
    assert re.min() >= -7 and im.min() >= -7
    h = S.point_taps(N, P, pfb)
    _assert_same_bits(_device(us, S.pack(-re, -im), N, F, W, h), _device(us, stream, N, F, W, h), "samples negated")


# ---------------------------------------------------------------- exact tones
@pytest.mark.parametrize("taps", [False, True])
@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_exact_tones_equal_the_int64_restatement(us, N, taps):
    """x[n] = a_f i^(m n), m in 0..3 per input: only the twiddles 1 and -i meet a non-zero value, one fine channel per input
    holds N a_f, every other is exactly zero, and both sums are integers below 2^24 times a power of two.  130 inputs x 2
    channels, windows of 16 frames within the gulp and of 256 over four gulps; with an integer PFB that is constant within
    each tap as well.  Word for word; the emulation gives the same words (tests/test_upchan_spectra_local_cpu.py)."""
    for W in (16, 256):
        stream, h, want = S.exact_tones(N, W, taps)
        _assert_same_bits(_device(us, stream, N, S.TONE_F, W, h), want, "N %d W %d taps %d" % (N, W, taps))


# ---------------------------------------------------------------- W = 1
@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("N", [4, 16, 64])
def test_single_frame_windows_give_s2_as_the_square_of_s1(us, N, pfb):
    """W = 1: one slot, one term: S1 = p and S2 = fmaf(p, p, 0) = f32(S1 S1) of the device's own S1, on the bits; and both
    inside bound_spectra (a single frame's cell can be as small against its frame as the FFT's rounding, so there is no cell
    bar here).  Every byte value, 130 inputs, two gulps of 12 frames."""
    F, ngulp = 12, 2
    rng = np.random.default_rng([N, int(pfb), 1])
    stream = rng.integers(0, 256, (ngulp * F * N, S.NCHAN, S.NINPUTS[1]), dtype=np.uint8)
    h = S.point_taps(N, 4, pfb)
    got = _device(us, stream, N, F, 1, h)
    assert got.shape[0] == ngulp * F
    s1 = got[:, 0].astype(np.float64)
    _assert_same_bits(got[:, 1], (s1 * s1).astype(np.float32), "S2 against the square of S1")
    rb = S.bound_ratio(got, S.ref_spectra(stream, N, 1, h), S.bound_spectra(stream, N, 1, h))
    print("W = 1, N = %d, pfb %d: err / bound %.3g" % (N, pfb, rb))
    assert rb <= 1


# ---------------------------------------------------------------- spectral kurtosis on RFI
@pytest.mark.parametrize("name", ["tone", "burst", "uneven"])
@pytest.mark.parametrize("point,pfb", [((32, 4, 30, 30, 3), False), ((32, 4, 30, 30, 3), True), ((32, 1, 30, 90, 3), False)],
                         ids=["M30", "M30-pfb", "M90-three-gulps"])
def test_spectral_kurtosis_of_rfi_within_the_margin_of_the_bars(us, point, pfb, name):
    """M = 30 (a window per gulp, plain and with the point's 4 taps) and M = 90 (three gulps), 130 inputs: |SK_dev - SK_ref|
    <= sk_margin wherever S1 > 0 and NaN exactly where the reference's S1 is 0 (the uneven case has such cells); at 3 and at 2
    sigma, sk_flags of the device's sums equals that of the reference's in every cell farther than sk_margin from both
    limits, and those left out are at most 1 % of all (counted on the reference alone).

    The data exercise both tails (plain FFT): every cell of the tone is flagged low wherever the lower limit is positive
    (at M = 30 that needs the 2-sigma limits: 1 - 3 sigma is negative there and SK >= 0), and more than half of the cells of
    the window that holds the burst are flagged high (a burst frame's power is exponential: a quarter of the cells draw too
    little of it to pass the limit) while at most a twentieth of the cells of the other windows are."""
    N, P, F, M, ngulp = point
    stream, info = S.spectra_case(name, N, F, ngulp, S.NINPUTS[1])
    h = S.point_taps(N, P, pfb)
    got, exp = _device(us, stream, N, F, M, h), S.ref_spectra(stream, N, M, h)
    sk_r, sk_d = spectral_kurtosis(exp[:, 0], exp[:, 1], M), spectral_kurtosis(got[:, 0], got[:, 1], M)
    live = exp[:, 0] > 0
    assert np.array_equal(np.isnan(sk_d), ~live) and (name != "uneven" or (~live).sum() == info["dead"].sum() * N * exp.shape[0])
    margin = np.where(live, S.sk_margin(np.where(live, sk_r, 0.0), M), np.inf)
    ratio = float((np.abs(sk_d - sk_r)[live] / margin[live]).max())
    print("SK %s M=%d pfb=%d: worst |dSK| / margin %.3g" % (name, M, pfb, ratio))
    assert ratio <= 1
    low_limit_met = False
    for nsigma in (3.0, 2.0):
        lo, hi = sk_limits(M, nsigma)
        near = live & ((np.abs(sk_r - lo) <= margin) | (np.abs(sk_r - hi) <= margin))
        fd, fr = sk_flags(got[:, 0], got[:, 1], M, nsigma), sk_flags(exp[:, 0], exp[:, 1], M, nsigma)
        print("  %g sigma: flagged %.2f %%, cells near a limit %d of %d" % (nsigma, 100 * fr.mean(), near.sum(), near.size))
        assert near.mean() <= 0.01
        assert np.array_equal(fd[~near], fr[~near])
        if pfb:
            continue
        if name == "tone" and lo > 0:
            low_limit_met = True
            assert (sk_r[:, :, info["j"]][..., info["inputs"]] < lo).all()
        if name == "burst":
            w = info["frame"] // M
            rest = np.delete(sk_r, w, axis=0)
            assert (sk_r[w] > hi).mean() > 0.5 and (rest.size == 0 or (rest > hi).mean() < 0.05)
    assert low_limit_met or name != "tone" or pfb
