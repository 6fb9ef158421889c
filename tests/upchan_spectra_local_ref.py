"""Local checks for upchan_spectra_kernel (UpchanSpectra), for inputs whose scales differ and for windows that
a few cells dominate: what tests/upchan_local_ref.py is for the fine-channel beam engines.

  check_cells    every S1 within 1e-5 and every S2 within 2e-5 of its OWN reference value, a zero cell exactly zero
  bound_spectra  an a-priori fp32 error bound per output, from the inputs alone (float64)
  emu_spectra    a float32 numpy emulation of the kernel's fixed sum: slot order, table twiddles, the two fmaf
  sk_margin      what the two cell bars allow the spectral kurtosis of a cell to move
  spectra_case   seeded 4-bit data: inputs of uneven scale with dead ones, a burst, a tone, power-of-two steps

Every term of both sums is non-negative, so a cell's own value is a scale that its error can be held to.  The float64
reference stays tests/upchan_spectra_ref.py; U, K_FFT, RANGE, emu_fft, _emu_pfb, _tap_sums, same_bits and pack come from
tests/upchan_local_ref.py."""
import numpy as np

from oracle import xeng_oracle as orc
from tests.upchan_local_ref import K_FFT, RANGE, U, _emu_pfb, _tap_sums, bound_ratio, emu_fft, f32, in_range, pack, same_bits  # noqa: F401
from tests.upchan_spectra_ref import channelised, upchan_spectra

BAR1 = 1e-5             # the house bar, per S1 cell
BAR2 = 2e-5             # per S2 cell: d(p^2) / p^2 = 2 dp / p
NSLOT = 4               # US_DEFSLOT of upchan_spectra_kernels.h

# (N, P, F, W, ngulp) of test_against_the_float64_restatement (tests/test_upchan_spectra_gpu.py)
POINTS = [(8, 1, 12, 4, 3), (8, 4, 12, 36, 3), (8, 8, 12, 12, 3), (16, 2, 10, 5, 3), (16, 8, 10, 20, 4), (16, 1, 750, 750, 1),
          (32, 4, 30, 30, 3), (32, 1, 30, 90, 3), (32, 8, 30, 15, 3), (32, 2, 30, 60, 4), (64, 2, 6, 3, 3), (64, 1, 6, 12, 4),
          (64, 4, 6, 6, 3), (64, 8, 9, 27, 3)]
NINPUTS = (70, 130)     # one and two full 64-lane runs plus a tail
NCHAN = 3
CASES = ("uneven", "burst", "tone", "steps")
# (case, point) pairs that the emulation does not hold inside a third of the cell bars (tests/test_upchan_spectra_local_cpu.py
# asserts both that and the rest): judged by bound_spectra alone, on the CPU and on the GPU
BOUND_ONLY = {("tone", (64, 2, 6, 3, 3)), ("tone", (64, 4, 6, 6, 3))}


# ---------------------------------------------------------------- the cell bar
def cell_ratios(got, exp):
    """|got - exp| / exp per cell of [..][2][nchan][N][ninput]; a cell whose reference is exactly 0 gives 0 where got is exactly
    zero (-0 included), inf otherwise."""
    got, exp = np.asarray(got), np.asarray(exp, np.float64)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert np.isfinite(got).all() and (exp >= 0).all()
    err = np.abs(got.astype(np.float64) - exp)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(exp > 0, err / exp, np.where(got != 0, np.inf, 0.0))


def check_cells(got, exp, bar1=BAR1, bar2=BAR2):
    """Every S1 within bar1 of its own reference value, every S2 within bar2 of its own.  Returns the two worst figures."""
    rel = cell_ratios(got, exp)
    worst = []
    for pl, bar in ((0, bar1), (1, bar2)):
        r = rel[:, pl]
        k = np.unravel_index(np.argmax(r), r.shape)
        assert r[k] <= bar, "cell S%d [window, c, j, i] = %s: |err| / own value = %.3e > %.1e" % (pl + 1, tuple(int(i) for i in k), r[k], bar)
        worst.append(float(r[k]))
    return tuple(worst)


def plane_ratios(got, exp):
    """The rule the UpchanSpectra tests had on its own: the largest error of each plane over the RMS of that whole plane."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return tuple(float(np.abs(got[:, pl] - exp[:, pl]).max() / np.sqrt(np.mean(exp[:, pl] ** 2))) for pl in range(2))


def sk_margin(sk_ref, M, bar1=BAR1, bar2=BAR2):
    """How far the cell bars let SK = (M+1)/(M-1) (r - 1), r = M S2 / S1^2, move: dr / r = dS2 / S2 - 2 dS1 / S1 to first
    order, at most bar2 + 2 bar1, and r = SK (M-1)/(M+1) + 1.  The margin is r (bar2 + 2 bar1): the bound on |dr|, which is
    (M+1)/(M-1) tighter than the bound on |dSK| itself (7 % at M = 30), and holds |SK| for r's sake where SK < 0."""
    return (np.abs(sk_ref) * (M - 1.0) / (M + 1.0) + 1.0) * (bar2 + 2 * bar1)


# ---------------------------------------------------------------- the float32 emulation
def _fma(a, b, c):
    """f32(a * b + c) of float32 arrays: the product is exact in float64 and the sum is rounded there before the rounding to
    float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def emu_spectra(stream, N, W, ntime, h=None):
    """upchan_spectra_kernel over the whole stream u8 [T][nchan][ninput] in gulps of ntime samples from a fresh context, in
    float32 numpy: decode, the PFB chain (_emu_pfb) or the plain frame, ucc_fft (emu_fft with the twiddles 1 and -i exact),
    p = f32(re re + f32(im im)); per launch window of wf = min(W, F) frames nslot = min(4, wf) chains over the frames
    s, s + nslot, ...: s1 = s1 + p, s2 = f32(p p + s2), the slots added as ((s0 + s1) + s2) + s3; for W > F the gulps' sums
    added in order.  Returns float32 [nwin][2][nchan][N][ninput]."""
    stream = np.asarray(stream)
    T, nchan, ninput = stream.shape
    nframe, F = T // N, ntime // N
    re, im = orc.decode(stream)
    xr, xi = re.astype(f32), im.astype(f32)
    if h is None:
        yr, yi = xr.reshape(nframe, N, nchan, ninput), xi.reshape(nframe, N, nchan, ninput)
    else:
        yr, yi = _emu_pfb(xr, xi, N, h, 0, nframe)
    Xr, Xi = emu_fft(yr.transpose(0, 2, 3, 1), yi.transpose(0, 2, 3, 1), exact_units=True)     # [f][c][i][j]
    p = _fma(Xr, Xr, Xi * Xi)
    wf = min(W, F)
    nslot = min(NSLOT, wf)
    p = p.reshape((nframe // wf, wf) + p.shape[1:])
    t1 = t2 = None
    for s in range(nslot):
        a1, a2 = np.zeros(p[:, 0].shape, f32), np.zeros(p[:, 0].shape, f32)
        for f in range(s, wf, nslot):
            a1 = a1 + p[:, f]
            a2 = _fma(p[:, f], p[:, f], a2)
        t1, t2 = (a1, a2) if s == 0 else (t1 + a1, t2 + a2)
    part = np.stack([t1, t2], axis=1)                                   # [launch window][2][c][i][j]
    if W > F:
        g = W // F
        part = part.reshape((part.shape[0] // g, g) + part.shape[1:])
        acc = part[:, 0]
        for q in range(1, g):
            acc = acc + part[:, q]
        part = acc
    return np.ascontiguousarray(part.transpose(0, 1, 2, 4, 3))


# ---------------------------------------------------------------- the a-priori bound
def frame_powers(stream, N, h=None):
    """p = |X|^2 of every frame of the stream in float64, [nframe][nchan][ninput][N]: the terms of S1 (and, squared, of S2)."""
    X = channelised(stream, N, 0, np.asarray(stream).shape[0], h)
    return X.real ** 2 + X.imag ** 2


def bound_spectra(stream, N, W, h=None):
    """B[w, m, c, j, i] >= |fp32 S_m - exact S_m| of upchan_spectra_kernel over the whole stream, to first order in u = 2^-24,
    from the inputs alone; shaped as the output.

    The voltage.  bound_voltage_error of tests/upchan_local_ref.py without the sum over inputs: every fine channel of a frame
    is off by at most E = K_FFT (log2 N + ntap) u A, A = sum_{n, k} |h[k, n]| |x[k, n]|_1 (K = 12 from the butterfly: a table
    twiddle at 4 ulp, an fma complex product, an add; the PFB's fmaf chain is ntap u of the same A).  Where no tap and no
    table twiddle is involved -- the plain FFT at N <= 4, whose butterflies use 1 and -i alone (ucc_fft) on small integers --
    the voltage is exact and E = 0.  A dead input has A = 0, so E = 0 there too.

    One frame's term.  The computed |X^| <= |X| + E, so with p^ = (|X| + E)^2
      p = fmaf(re, re, f32(im im)): ||X^|^2 - |X|^2| <= 2 |X| E + E^2, and two roundings of at most u p^ each:
          dp = 2 |X| E + E^2 + 2 u p^
      p p inside s2 = fmaf(p, p, s2): |(p + dp)^2 - p^2| <= 2 p^ dp + dp^2 (p <= p^), and u p^^2 more lets the product be
          rounded on its own as well:   d(p^2) = 2 p^ dp + dp^2 + u p^^2
    The sums.  A term passes through at most ceil(wf / nslot) additions of its slot's chain, nslot - 1 <= 3 of the slots and
    G - 1 of the gulps of its window; that is at most W + 2 for every W, F and G = W / F.  All terms are non-negative, so
    every partial sum is at most the full one and each addition errs by at most u of it: (W + 2) u sum p^ for S1 and
    (W + 2) u sum p^^2 for S2, on top of the summed dp and d(p^2).

    B is zero exactly where the samples that reach the window from that (channel, input) are all zero.  Like the bounds of
    DESIGN.md 4.18 it is a ceiling for what is 50 to 100 times larger than rounding, not a tight check."""
    stream = np.asarray(stream)
    T, nchan, ninput = stream.shape
    nframe = T // N
    hh = np.ones(N) if h is None else np.asarray(h, np.float64)
    ntap = hh.size // N
    X = np.abs(channelised(stream, N, 0, T, h))                         # [f][c][i][j]
    if h is None and N <= 4:
        E = np.zeros(X.shape)
    else:
        re, im = orc.decode(stream)
        a1 = np.abs(re.astype(np.float64)) + np.abs(im.astype(np.float64))
        A = _tap_sums(a1, N, hh, 0, nframe)                             # [f][c][i]
        E = np.broadcast_to((K_FFT * (np.log2(N) + ntap) * U * A)[..., None], X.shape)
    ph = (X + E) ** 2
    dp = 2 * X * E + E ** 2 + 2 * U * ph
    dp2 = 2 * ph * dp + dp ** 2 + U * ph ** 2

    def win(a):
        return a.reshape((nframe // W, W) + a.shape[1:]).sum(axis=1)
    g = (W + 2) * U
    b = np.stack([win(dp) + g * win(ph), win(dp2) + g * win(ph ** 2)], axis=1)     # [w][2][c][i][j]
    return np.ascontiguousarray(b.transpose(0, 1, 2, 4, 3))


def ref_spectra(stream, N, W, h=None):
    """The float64 restatement over the whole stream from a fresh context: [nwin][2][nchan][N][ninput]."""
    return upchan_spectra(stream, N, W, 0, np.asarray(stream).shape[0], h)


# ---------------------------------------------------------------- cases
def _gauss(rng, sigma, shape):
    """Complex Gaussian samples of the given sigma per component, rounded and clipped to -7..7: (re, im) int64."""
    return tuple(np.clip(np.rint(rng.standard_normal(shape) * sigma), -7, 7).astype(np.int64) for _ in range(2))


def point_taps(N, P, pfb):
    """The taps of a point: None for the plain FFT; else P (4 where the point has P = 1) seeded standard_normal taps per
    branch, asymmetric, as in test_against_the_float64_restatement."""
    if not pfb:
        return None
    ntap = P if P > 1 else 4
    return np.random.default_rng([7, N, ntap]).standard_normal(ntap * N).astype(np.float32)


def tone_channel(N):
    """The fine channel of the tone case."""
    return N // 4 + 1


def spectra_case(name, N, F, ngulp, ninput, nchan=NCHAN, seed=0, quiet=0.7):
    """(stream u8 [ngulp F N][nchan][ninput], info) over 4-bit data:
      uneven   Gaussian, sigma per input from {0.4, 1, 2.5}; inputs 5 and ninput - 2 (in the tail run) dead; the odd inputs of
               coarse channel 1 dead.  info['dead'] bool [nchan][ninput]
      burst    sigma 0.6 noise with one frame, in the second gulp if there is one, at sigma 3.5 on every input and channel.
               info['frame']
      tone     amplitude 6 in fine channel N/4 + 1 on every third input over sigma 0.7 noise; the inputs without the tone at
               sigma `quiet`.  info['j'], info['inputs']
      steps    samples in -1..1 times 2^k[i], k in {0, 1, 2} per input.  info['k'], info['base'] (the stream at k = 0)"""
    rng = np.random.default_rng([seed, N, F, ngulp, ninput, CASES.index(name)])
    T = ngulp * F * N
    shape = (T, nchan, ninput)
    info = {}
    if name == "uneven":
        sigma = np.array([0.4, 1.0, 2.5])[rng.permutation(np.arange(ninput) % 3)]
        re, im = _gauss(rng, sigma, shape)
        dead = np.zeros((nchan, ninput), bool)
        dead[:, [5, ninput - 2]] = True
        dead[1, 1::2] = True
        re[:, dead], im[:, dead] = 0, 0
        info["dead"], info["sigma"] = dead, sigma
    elif name == "burst":
        re, im = _gauss(rng, 0.6, shape)
        f = int(rng.integers(0, F)) + (F if ngulp > 1 else 0)
        br, bi = _gauss(rng, 3.5, (N, nchan, ninput))
        re[f * N:(f + 1) * N], im[f * N:(f + 1) * N] = br, bi
        info["frame"] = f
    elif name == "tone":
        j = tone_channel(N)
        on = np.arange(ninput) % 3 == 0
        z = 6 * np.exp(2j * np.pi * (j - N // 2) * np.arange(T) / N)[:, None, None] * on
        nr, ni = _gauss(rng, np.where(on, 0.7, quiet), shape)
        re = np.clip(np.rint(z.real).astype(np.int64) + nr, -7, 7)
        im = np.clip(np.rint(z.imag).astype(np.int64) + ni, -7, 7)
        info["j"], info["inputs"] = j, on
    else:
        assert name == "steps", name
        br, bi = rng.integers(-1, 2, shape), rng.integers(-1, 2, shape)
        k = rng.integers(0, 3, ninput)
        k[:3] = (0, 1, 2)
        re, im = br << k, bi << k
        info["k"], info["base"] = k.astype(np.int32), pack(br, bi)
    return pack(re, im), info


# ---------------------------------------------------------------- the exact power-of-two covariance
def scaled_inputs(out, k):
    """What the kernel must give, bit for bit, for samples times 2^k[i] when `out` is what it gives for the samples."""
    k = np.asarray(k, np.int32)
    return np.ldexp(out, np.stack([2 * k, 4 * k])[None, :, None, None, :])


def scaled_taps(out, k):
    """The same for h 2^k, one k for all taps."""
    return np.ldexp(out, np.array([2 * k, 4 * k], np.int32)[None, :, None, None, None])


# ---------------------------------------------------------------- exact tones
TONE_F, TONE_NGULP, TONE_NINPUT, TONE_NCHAN = 64, 4, 130, 2
TONE_TAPS = (1, -1, 2, 1)


def exact_tones(N, W, taps=False, seed=0):
    """(stream, h, want): x[n] = a_f i^(m n) within every frame, m in 0..3 per input, a_f a complex integer per (frame,
    channel, input) with parts in -7..7 (-2..2 with taps); four gulps of 64 frames, 130 inputs x 2 channels, N a multiple of
    4.  taps: the integer PFB h[k, n] = TONE_TAPS[k], constant within each tap, so that y[n] = b_f i^(m n) with
    b_f = sum_k g_k a_(f - 3 + k); else h is None and b = a.  want: the int64 restatement as float32
    [nwin][2][nchan][N][ninput] -- bin m N / 4 holds N b_f, fine channel (m N / 4 + N / 2) mod N holds S1 = N^2 sum |b|^2 and
    S2 = N^4 sum |b|^4, everything else is zero -- after asserting that every sum is below 2^24 times its power of two."""
    assert N % 4 == 0 and (TONE_F * TONE_NGULP) % W == 0
    rng = np.random.default_rng([seed, N, int(taps), 11])
    nframe = TONE_F * TONE_NGULP
    amax = 2 if taps else 7
    ar, ai = rng.integers(-amax, amax + 1, (2, nframe, 1, TONE_NCHAN, TONE_NINPUT))
    m = rng.integers(0, 4, TONE_NINPUT)
    m[:4] = (0, 1, 2, 3)
    q = ((m[None, :] * np.arange(N)[:, None]) % 4)[None, :, None, :]             # the rotation i^q of sample n, input i
    shape = (nframe, N, TONE_NCHAN, TONE_NINPUT)
    re = np.choose(q, [np.broadcast_to(a, shape) for a in (ar, -ai, -ar, ai)])
    im = np.choose(q, [np.broadcast_to(a, shape) for a in (ai, ar, -ai, -ar)])
    stream = pack(re.reshape(-1, TONE_NCHAN, TONE_NINPUT), im.reshape(-1, TONE_NCHAN, TONE_NINPUT))
    br, bi, h = ar[:, 0], ai[:, 0], None
    if taps:
        P = len(TONE_TAPS)
        h = np.repeat(np.array(TONE_TAPS, f32), N)
        br, bi = np.zeros_like(br), np.zeros_like(bi)
        for k, g in enumerate(TONE_TAPS):
            d = P - 1 - k
            br[d:] += g * ar[:nframe - d, 0]
            bi[d:] += g * ai[:nframe - d, 0]
    pw = (br * br + bi * bi).astype(np.int64)                                   # |b|^2 [f][c][i]
    pw = pw.reshape(nframe // W, W, TONE_NCHAN, TONE_NINPUT)
    s1, s2 = pw.sum(axis=1), (pw * pw).sum(axis=1)
    assert s2.max() < 2 ** 24
    want = np.zeros((nframe // W, 2, TONE_NCHAN, N, TONE_NINPUT), np.int64)
    j = (m * (N // 4) + N // 2) % N
    want[:, 0, :, j, np.arange(TONE_NINPUT)] = (N ** 2 * s1).transpose(2, 0, 1)
    want[:, 1, :, j, np.arange(TONE_NINPUT)] = (N ** 4 * s2).transpose(2, 0, 1)
    return stream, h, want.astype(f32)
