"""upchan_beamform_kernel and upchan_sum_beams_kernel on the MI355X with rows of very different scale (tests/upchan_local_ref.py).

The exact part: scaling a row's weights (UpchanBeamform) or a beam's samples (UpchanSumBeams) by 2^k, k in [-20, 20], scales
that row's outputs by 2^k, 2^2k or 2^(kx + ky) and nothing else, on the bits; permuting beams (whole pairs in dual-pol)
permutes the outputs on the bits.  Both kernels are fixed-order fp32 chains, so any leak between rows, a shared or late-cleared
accumulator or a mask on the wrong beam breaks the equality, however small the row.

The bounded part: every output within 1e-5 of the RMS of its own row against the float64 restatements, zero rows exactly
zero, and inside an a-priori bound per output; the worst ratios are printed (DESIGN.md 4.18 records them).  No wall-clock
assertions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from tests import upchan_local_ref as L  # noqa: E402
from tests.test_upchan_beams_gpu import UB  # noqa: E402
from tests.test_upchan_pfb_gpu import UP  # noqa: E402

NINPUT, NCHAN = 36, 3           # input chunks of 16 + 16 + 4


@pytest.fixture
def up():
    yield UP
    ffi.call("xengUpchanDestroy")


@pytest.fixture
def ub():
    yield UB
    ffi.call("xengUpchanSumBeamsDestroy")


def _gulps(u, stream, ntime, w):
    """The stream's gulps through the context from a fresh history."""
    ffi.call("xengUpchanReset")
    return [u.run(stream[g * ntime:(g + 1) * ntime], w if g == 0 else None) for g in range(stream.shape[0] // ntime)]


def _assert_same_bits(got, want, what):
    d = L.same_bits(got, want)
    assert d.size == 0, "%s: words differ, the first at %s" % (what, d.tolist())


# ---------------------------------------------------------------- UpchanBeamform: exact covariance
@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("mode,N,nbeam,nframe,ns", L.beamform_points())
def test_beamform_scaling_and_permuting_rows_is_exact(up, mode, N, nbeam, nframe, ns, pfb):
    """w' = w 2^k per (c, j, b): v' = ldexp(v, k), p' = ldexp(p, 2k), dual-pol 2k of beam 2p / 2k of beam 2p+1 / the sum of the two
    for both cross terms; then the beams of w' permuted: the outputs permuted.  All on the bits.  With the PFB (4 random taps)
    over two gulps, so that the history takes part."""
    dual = mode == "dual"
    rng = np.random.default_rng([N, nbeam, nframe, ns, int(pfb), int(dual)])
    ntime = nframe * N
    stream = rng.integers(0, 256, ((2 if pfb else 1) * ntime, NCHAN, NINPUT), dtype=np.uint8)
    w = L.rand_w(rng, NCHAN, N, nbeam, NINPUT)
    h = rng.standard_normal(4 * N).astype(np.float32) if pfb else None
    k = L.uneven_k(rng, (NCHAN, N, nbeam))
    ws = L.scale_weights(w, k)
    perm = L.pair_perm(rng, nbeam) if dual else rng.permutation(nbeam)
    for g in range(stream.shape[0] // ntime):           # nothing leaves the normal range: scaling commutes with every rounding
        a = dict(h=h, start=g * ntime, ntime=ntime)
        assert L.in_range(L.ref_beamform(stream, w, N, nbeam, nframe_sum=ns, dual=dual, **a), L.term_magnitudes(stream, w, N, nbeam, **a),
                          L.ref_beamform(stream, ws, N, nbeam, nframe_sum=ns, dual=dual, **a), L.term_magnitudes(stream, ws, N, nbeam, **a))
    u = up(NINPUT, NCHAN, ntime, N, nbeam, ns, dual, 4 if pfb else None, h)
    base = _gulps(u, stream, ntime, w)
    scaled = _gulps(u, stream, ntime, ws)
    permuted = _gulps(u, stream, ntime, np.ascontiguousarray(ws[:, :, perm]))
    for g, (b, s, p) in enumerate(zip(base, scaled, permuted)):
        _assert_same_bits(s, L.scaled_beamform(b, k, ns, dual), "gulp %d, rows scaled [window or frame][beam or pair][c][j]" % g)
        _assert_same_bits(p, s[:, perm[::2] // 2] if dual else s[:, perm], "gulp %d, beams permuted" % g)


# ---------------------------------------------------------------- UpchanBeamform: row bar and a-priori bound
@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("mode,N,nbeam,nframe,ns", L.beamform_points())
def test_beamform_rows_within_their_own_bar_and_bound(up, mode, N, nbeam, nframe, ns, pfb):
    """Every shape of the covariance test at 52 inputs (upchan_local_ref.ROW_NINPUT), 3 channels, two gulps of nframe frames, rows scaled by 2^k with a tenth of each row's inputs at 64 times the rest
    and a tenth at zero; a zero beam and a channel of zero bytes (exactly zero outputs); a channel of nibbles in -1..1; with the
    PFB the taps of a low-pass prototype (several decades).  Every output within 1e-5 of its own row's RMS and inside
    bound_beamform.

    The tone case (amplitude 7 in one fine channel on a quarter of the inputs over +-1 noise) is judged by the bound alone: the
    fp32 FFT's rounding of the tone reaches the other fine channels of the same (frame, channel, input) at about
    u log2(N) 7N, which is not small against a row at the noise level.  The bound is local in (frame, beam, channel), and that
    is all fp32 can promise there."""
    dual = mode == "dual"
    worst_row = worst_bound = 0.0
    for name in L.BEAMFORM_CASES + ("tone",):
        stream, w, h = L.beamform_case(name, N, nbeam, pfb, nframe=nframe)
        ntime = stream.shape[0] // 2
        u = up(L.ROW_NINPUT, L.ROW_NCHAN, ntime, N, nbeam, ns, dual, L.ROW_NTAP if pfb else None, h)
        for g, got in enumerate(_gulps(u, stream, ntime, w)):
            a = dict(h=h, start=g * ntime, ntime=ntime, nframe_sum=ns, dual=dual)
            exp = L.ref_beamform(stream, w, N, nbeam, **a)
            rb = L.bound_ratio(got, exp, L.bound_beamform(stream, w, N, nbeam, **a))
            rr = float(np.max(L.row_ratios(got, exp)))
            print("UpchanBeamform %s N=%d nbeam=%d nframe=%d ns=%d pfb=%d %s gulp %d: err/rowRMS %.3g, err/bound %.3g" % (mode, N, nbeam, nframe, ns, pfb, name, g, rr, rb))
            worst_bound = max(worst_bound, rb)
            if name != "tone":
                worst_row = max(worst_row, rr)
                L.check_rows(got, exp)
            assert rb <= 1, "%s gulp %d: worst |err| / bound = %.3g" % (name, g, rb)
            if name == "zero_beam":
                assert ((got[:, 0, ..., 1:] if dual else got[:, 1]) == 0).all()
            if name == "zero_chan":
                assert (got[:, :, 1] == 0).all()
    print("UpchanBeamform %s N=%d nbeam=%d nframe=%d ns=%d pfb=%d: worst err/rowRMS %.3g, worst err/bound %.3g" % (mode, N, nbeam, nframe, ns, pfb, worst_row, worst_bound))


# ---------------------------------------------------------------- UpchanSumBeams
def _windows(u, v, span):
    """The stream's gulps through the context from a fresh history: [nwin][npair][nchan][N][4]."""
    ffi.call("xengUpchanSumBeamsReset")
    outs = []
    for g in range(L.SUM_NGULP):
        last = not span or g % 2 == 1
        u.poison()
        u.run(v[..., g * L.SUM_NTIME:(g + 1) * L.SUM_NTIME], out=last)
        if last:
            outs.append(u.result().copy())
    return np.concatenate(outs)


def _sum_ctx(ub, N, span, h, pair0=0, npair=None):
    F = L.SUM_NTIME // N
    W = 2 * F if span else F // 2
    return ub(L.SUM_NCHAN, L.SUM_NBEAM, L.SUM_NTIME, N, W, pair0, npair, ntap=None if h is None else h.size // N, h=h), W


@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("span", [False, True])
@pytest.mark.parametrize("N", [8, 16, 64])
def test_sum_beams_scaling_rows_is_exact(ub, N, span, pfb):
    """3 channels, 8 beams, 4 gulps of 512 samples, windows of F / 2 frames (inside a gulp) and of 2F (the accumulator adds gulp
    partials), 1 and 4 taps.  v' = v 2^k per (c, b): XX by 2^2kx, YY by 2^2ky, both cross terms by 2^(kx + ky), on the bits, for
    all pairs and for the pair subset 1..2; h' = 8h: every output by 2^6; and (plain FFT) one window's samples by 2^k: that
    window's outputs by 2^2k, every other window's bits as they were."""
    rng = np.random.default_rng([N, int(span), int(pfb)])
    v = L.rand_beams(rng, L.SUM_NCHAN, L.SUM_NBEAM, L.SUM_NGULP * L.SUM_NTIME)
    h = rng.standard_normal(4 * N).astype(np.float32) if pfb else None
    k = L.uneven_k(rng, (L.SUM_NCHAN, L.SUM_NBEAM))
    vs = L.scale_beams(v, k)
    F = L.SUM_NTIME // N
    W = 2 * F if span else F // 2
    kw = int(rng.integers(5, 21)) * (-1 if span else 1)
    nw = W * N                                          # samples per window
    vw = v.copy()
    vw[..., nw:2 * nw] = L.scale_beams(v[..., nw:2 * nw], np.full((L.SUM_NCHAN, L.SUM_NBEAM), kw, np.int32))
    for x in (v, vs, vw):
        assert L.in_range(L.ref_sum_beams(x, N, W, h), L.ref_sum_beams(x, N, W, None if h is None else 8 * h))
    for pair0, npair in ((0, None), (1, 2)):
        base = _windows(_sum_ctx(ub, N, span, h, pair0, npair)[0], v, span)
        scaled = _windows(_sum_ctx(ub, N, span, h, pair0, npair)[0], vs, span)
        _assert_same_bits(scaled, L.scaled_sum_beams(base, k, pair0, npair), "pairs from %d, beams scaled [window][pair][c][j][4]" % pair0)
        if pfb:
            _assert_same_bits(_windows(_sum_ctx(ub, N, span, 8 * h, pair0, npair)[0], v, span), np.ldexp(base, 6), "pairs from %d, h scaled by 8" % pair0)
        else:
            want = base.copy()
            want[1] = np.ldexp(base[1], 2 * kw)
            _assert_same_bits(_windows(_sum_ctx(ub, N, span, h, pair0, npair)[0], vw, span), want, "pairs from %d, window 1 scaled" % pair0)


@pytest.mark.parametrize("pfb", [False, True])
@pytest.mark.parametrize("span", [False, True])
@pytest.mark.parametrize("N", [8, 64])
def test_sum_beams_rows_within_their_own_bar_and_bound(ub, N, span, pfb):
    """Beams scaled by 2^k; X loud and Y quiet inside every pair (2^20 / 2^-20); a zero Y (YY and both cross terms exactly
    zero); a burst 2^15 louder in one window (plain FFT); with the PFB the taps of a low-pass prototype.  Pairs 1..2 of 4.  Every
    output within 1e-5 of its own row's scale and inside bound_sum_beams.

    In the burst case a row spans the windows, so its RMS is set by the window that is 2^30 louder: check_rows says nothing
    about the quiet windows of such a row.  They are held by bound_sum_beams, which is local to a window, and by the covariance
    test above (one window scaled: every other window's bits as they were)."""
    worst_row = worst_bound = 0.0
    for name in L.SUM_CASES:
        if name == "burst" and pfb:
            continue
        v, h = L.sum_beams_case(name, N, pfb)
        u, W = _sum_ctx(ub, N, span, h, 1, 2)
        got = _windows(u, v, span)
        exp = L.ref_sum_beams(v, N, W, h, 1, 2)
        rb = L.bound_ratio(got, exp, L.bound_sum_beams(v, N, W, h, 1, 2))
        rr = float(np.max(L.row_ratios(got, exp)))
        print("UpchanSumBeams N=%d W=%d pfb=%d %s: err/rowRMS %.3g, err/bound %.3g" % (N, W, pfb, name, rr, rb))
        worst_row, worst_bound = max(worst_row, rr), max(worst_bound, rb)
        L.check_rows(got, exp)
        assert rb <= 1, "%s: worst |err| / bound = %.3g" % (name, rb)
        if name == "zero_beam":
            assert (got[:, 0, ..., 1:] == 0).all() and (got[:, 0, ..., 0] > 0).all()
    print("UpchanSumBeams N=%d W=%d pfb=%d: worst err/rowRMS %.3g, worst err/bound %.3g" % (N, W, pfb, worst_row, worst_bound))
