"""Local checks for the fine-channel engines built on upchan_beamform_kernel and upchan_sum_beams_kernel (UpchanBeamform in
its voltage, power and dual-pol modes, UpchanSumBeams), for inputs whose rows differ in scale by many octaves:

  check_rows     every output within 1e-5 of the RMS of its OWN row, a zero row exactly zero
  bound_*        an a-priori fp32 error bound per output, from the inputs alone (float64)
  emu_*          float32 numpy emulations of the two kernels' chains: the same order, table twiddles, no fma
  scaled / ...   the exact power-of-two covariance the kernels must obey bit for bit, and the cases that exercise it

A row is one (beam, coarse channel, fine channel) across the frames or windows of a call; for the four-component outputs one
(pair, coarse channel, fine channel, component).  The float64 references are the restatements of tests/upchan_pfb_ref.py and
tests/upchan_beams_ref.py (the plain FFT is their one tap of ones)."""
import numpy as np

from oracle import xeng_oracle as orc
from tests.upchan_beams_ref import beam_channelise, sum_beams
from tests.upchan_pfb_ref import pfb_channelise, upchan_beamform_pfb

U = 2.0 ** -24          # fp32 unit roundoff
BAR = 1e-5              # the house bar of the upchan tests, here per row
K_FFT = 12              # see bound_voltage_error
RANGE = (2.0 ** -100, 2.0 ** 100)


# ---------------------------------------------------------------- the row bar
def row_ratios(got, exp):
    """max over axis 0 of |got - exp| over the row's scale, per row.  The scale is the RMS of the row's reference; for the
    four-component outputs [..][4] the cross terms (components 2, 3) are judged against sqrt(RMS(XX) RMS(YY)) of their row.  A
    row whose scale is zero (its reference is identically zero) gives 0 where got is exactly zero (-0 included), inf otherwise."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert np.isfinite(got).all()
    err = np.max(np.abs(got.astype(exp.dtype) - exp), axis=0)
    rms = np.sqrt(np.mean(np.abs(exp) ** 2, axis=0))
    if exp.ndim == 5:
        cross = np.sqrt(rms[..., 0] * rms[..., 1])
        scale = np.stack([rms[..., 0], rms[..., 1], cross, cross], axis=-1)
    else:
        scale = rms
    nonzero = (got != 0).any(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, err / scale, np.where(nonzero, np.inf, 0.0))


def check_rows(got, exp, bar=BAR):
    """Every element within `bar` of its own row's scale (row_ratios).  Returns the worst row's figure."""
    rel = row_ratios(got, exp)
    k = np.unravel_index(np.argmax(rel), rel.shape)
    assert rel[k] <= bar, "row %s: max |err| / row scale = %.3e" % (tuple(int(i) for i in k), rel[k])
    return float(rel[k])


# ---------------------------------------------------------------- float64 references
def ref_beamform(stream, w, N, nbeam, h=None, start=0, ntime=None, nframe_sum=0, dual=False):
    """UpchanBeamform's gulp [start, start + ntime) of the stream in float64 (voltage, power or dual-pol); h = None: the plain
    FFT."""
    ntime = stream.shape[0] - start if ntime is None else ntime
    return upchan_beamform_pfb(stream, w, N, nbeam, np.ones(N) if h is None else h, start, ntime, nframe_sum, dual_pol=dual)


def ref_sum_beams(v, N, W, h=None, pair0=0, npair=None):
    """UpchanSumBeams over the whole stream v [nchan][nbeam][T] in float64: [T / N / W][npair][nchan][N][4]."""
    return sum_beams(beam_channelise(v, N, h, 0, v.shape[-1]), W, pair0, npair)


def _abs1(z):
    return np.abs(z.real) + np.abs(z.imag)


def _tap_sums(a1, N, h, start, nframe):
    """A[f, ...] = sum_{k, n} |h[k*N + n]| a1[start + (f - P + 1 + k)*N + n, ...] (samples before 0 count as zero)."""
    habs = np.abs(np.asarray(h, np.float64).reshape(-1, N))
    A = np.zeros((nframe,) + a1.shape[1:])
    for f in range(nframe):
        for k in range(habs.shape[0]):
            t = start + (f - habs.shape[0] + 1 + k) * N
            if t >= 0:
                A[f] += np.tensordot(habs[k], a1[t:t + N], axes=(0, 0))
    return A


# ---------------------------------------------------------------- a-priori bounds
def _fft_factor(N, ntap):
    return K_FFT * (np.log2(N) + ntap) * U


def bound_voltage_error(stream, w, N, nbeam, h=None, start=0, ntime=None):
    """E[f, b, c, j] >= |fp32 voltage - exact voltage| of upchan_beamform_kernel, to first order in u = 2^-24, from the inputs
    alone.  |z|_1 = |Re z| + |Im z| >= |z|.

    The sum over inputs.  Each component of v is a chain of 2 * ninput fmaf, one rounding each, on terms whose magnitudes sum to
    at most S = sum_i |w_i|_1 |X_i|_1: 2 ninput u S per component, sqrt(2) of that in modulus; 4 ninput u S covers it and, by the
    factor 4 / (2 sqrt 2), the second-order terms and the use of the exact X for the rounded one.

    The FFT and the PFB.  A = sum_{n, k} |h[k, n]| |x[k, n]|_1 bounds sum_n |y[n]| for the FFT's input y, and every intermediate
    value of the radix-2 FFT is a sum of a subset of the y[n] times unit factors.  One butterfly is a' = a + b t, b' = a - b t:
      the twiddle t comes from a table filled by sincospif.  OCML's sincospi is built to OpenCL's accuracy for sinpi / cospi,
        4 ulp (OpenCL C specification, "Relative error as ULPs"; no tighter figure is documented for the device library, and the
        bound must not depend on one): each component within 4 * 2^-23 of itself, |dt| <= 8 u;
      the complex product is fmaf(b.x, t.x, -(b.y * t.y)) and its twin: two roundings per component, each <= u |b||t|
        (Cauchy-Schwarz on the two terms), 2 sqrt(2) u |b| in modulus;
      the add rounds each component once: u (|a| + |b|) in modulus.
    Per stage an output collects these over disjoint subsets that cover all n, so a stage adds at most (8 + 2 sqrt 2 + 1) u
    sum_n |y[n]| <= 12 u A: K = 12.  The PFB in front is a chain of ntap fmaf per component from zero, <= ntap u sum_k |h||x|_1
    per sample.  So |dX_i[j]| <= (K log2 N + ntap) u A_i <= K (log2 N + ntap) u A_i, and it reaches v through sum_i |w_i| |dX_i|.
    The plain FFT counts as one tap of ones.

        E = 4 ninput u sum_i |w|_1 |X|_1 + K (log2 N + ntap) u sum_i |w|_1 A_i

    E is zero exactly where the beam's weights or the channel's samples are all zero."""
    ntime = stream.shape[0] - start if ntime is None else ntime
    nchan, ninput = stream.shape[1:]
    h = np.ones(N) if h is None else np.asarray(h, np.float64)
    re, im = orc.decode(np.asarray(stream))
    a1 = np.abs(re.astype(np.float64)) + np.abs(im.astype(np.float64))
    A = _tap_sums(a1, N, h, start, ntime // N)                           # [f][c][i]
    X1 = _abs1(pfb_channelise(stream, N, h, start, ntime))              # [f][c][i][j]
    w1 = _abs1(np.asarray(w).reshape(nchan, N, nbeam, ninput).astype(np.complex128))
    S = np.einsum('cjbi,fcij->fbcj', w1, X1, optimize=True)
    F = np.einsum('cjbi,fci->fbcj', w1, A, optimize=True)
    return 4 * ninput * U * S + _fft_factor(N, h.size // N) * F


def _bound_products(X, Y, EX, EY, ns):
    """Bound on the four window sums of X, Y [nwin * ns][...] with voltage errors EX, EY: the propagation
    ||v + d|^2 - |v|^2| <= 2 |v| E + E^2 and |(X + dX) conj(Y + dY) - X conj Y| <= |X| EY + |Y| EX + EX EY (which bounds both
    components of the cross term), plus (2 ns + 2) u of the summed magnitudes of the perturbed terms: a product is at most two
    roundings and the window's chain (frames, then gulp partials) at most 2 ns more, on terms that sum to at most
    sum_f |X||Y| (= sum_f |X|^2 for XX)."""
    def win(a):
        return a.reshape((a.shape[0] // ns, ns) + a.shape[1:]).sum(axis=1)
    aX, aY = np.abs(X), np.abs(Y)
    g = (2 * ns + 2) * U
    bxx = win(2 * aX * EX + EX ** 2) + g * win((aX + EX) ** 2)
    byy = win(2 * aY * EY + EY ** 2) + g * win((aY + EY) ** 2)
    bxy = win(aX * EY + aY * EX + EX * EY) + g * win((aX + EX) * (aY + EY))
    return bxx, byy, bxy


def bound_beamform(stream, w, N, nbeam, h=None, start=0, ntime=None, nframe_sum=0, dual=False):
    """The a-priori bound for every output of UpchanBeamform, shaped as the output: bound_voltage_error itself in voltage mode,
    pushed through |v|^2 or the 2x2 products and the window sums (_bound_products) otherwise."""
    E = bound_voltage_error(stream, w, N, nbeam, h, start, ntime)
    if not nframe_sum:
        return E
    v = ref_beamform(stream, w, N, nbeam, h, start, ntime)
    if not dual:
        return _bound_products(v, v, E, E, nframe_sum)[0]
    bxx, byy, bxy = _bound_products(v[:, 0::2], v[:, 1::2], E[:, 0::2], E[:, 1::2], nframe_sum)
    return np.stack([bxx, byy, bxy, bxy], axis=-1)


def bound_sum_beams(v, N, W, h=None, pair0=0, npair=None):
    """The same for UpchanSumBeams over the whole stream v [nchan][nbeam][T]: there is no sum over inputs, so the voltage error
    is the FFT / PFB term alone, K (log2 N + ntap) u sum_{n, k} |h||v|_1 for every fine channel of a frame."""
    v = np.asarray(v).astype(np.complex128)
    nchan, nbeam, T = v.shape
    npair = nbeam // 2 - pair0 if npair is None else npair
    hh = np.ones(N) if h is None else np.asarray(h, np.float64)
    A = _tap_sums(np.moveaxis(_abs1(v), -1, 0), N, hh, 0, T // N)       # [f][c][b]
    E = np.broadcast_to((_fft_factor(N, hh.size // N) * A)[..., None], A.shape + (N,))
    V = beam_channelise(v, N, h, 0, T)                                  # [f][c][b][j]
    sel = slice(2 * pair0, 2 * (pair0 + npair))
    V, E = V[:, :, sel], E[:, :, sel]
    bxx, byy, bxy = _bound_products(V[:, :, 0::2], V[:, :, 1::2], E[:, :, 0::2], E[:, :, 1::2], W)
    return np.stack([bxx, byy, bxy, bxy], axis=-1).transpose(0, 2, 1, 3, 4)


def bound_ratio(got, exp, bound):
    """The worst |got - exp| / bound; where the bound is zero the output must be exactly zero (inf otherwise)."""
    err = np.abs(np.asarray(got).astype(exp.dtype) - exp)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(bound > 0, err / bound, np.where(np.asarray(got) != 0, np.inf, 0.0))))


# ---------------------------------------------------------------- float32 emulations of the kernels' chains
f32 = np.float32


def cplx(re, im):
    """complex64 from float32 parts, bit for bit (a + 1j * b would turn a real part of -0 into +0)."""
    z = np.empty(np.shape(re), np.complex64)
    z.real, z.imag = re, im
    return z


_TW = (np.cos(-np.pi * np.arange(32) / 32).astype(f32), np.sin(-np.pi * np.arange(32) / 32).astype(f32))


def _bitrev(N):
    bits = N.bit_length() - 1
    return np.array([int(format(n, '0%db' % bits)[::-1], 2) for n in range(N)])


def emu_fft(yr, yi, exact_units=False):
    """uc_fft on float32 [...][N] in natural order, every operation rounded to float32 (no fma), the twiddles rounded from
    float64; returns the fine-channel order j = (k + N/2) mod N.  exact_units: ucc_fft, which applies the twiddles 1 and -i
    as a copy and a swap instead of reading them from the table."""
    N = yr.shape[-1]
    rev = _bitrev(N)
    vr, vi = np.ascontiguousarray(yr[..., rev]), np.ascontiguousarray(yi[..., rev])
    ln = 2
    while ln <= N:
        half = ln // 2
        for k in range(half):
            k64 = k * (64 // ln)
            tr, ti = _TW[0][k64], _TW[1][k64]
            a, b = slice(k, None, ln), slice(k + half, None, ln)
            if exact_units and k64 == 0:
                br, bi = vr[..., b].copy(), vi[..., b].copy()
            elif exact_units and k64 == 16:
                br, bi = vi[..., b].copy(), -vr[..., b]
            else:
                br = vr[..., b] * tr - vi[..., b] * ti
                bi = vr[..., b] * ti + vi[..., b] * tr
            ar, ai = vr[..., a].copy(), vi[..., a].copy()
            vr[..., a], vi[..., a] = ar + br, ai + bi
            vr[..., b], vi[..., b] = ar - br, ai - bi
        ln *= 2
    return np.roll(vr, N // 2, axis=-1), np.roll(vi, N // 2, axis=-1)


def _emu_pfb(xr, xi, N, h, start, nframe):
    """y[f][n][...] = the k-ascending chain y + h[k, n] x of float32 samples x [T][...] (frames before 0 are zeros)."""
    h = np.asarray(h, f32).reshape(-1, N)
    P = h.shape[0]
    tail = (1,) * (xr.ndim - 1)
    yr, yi = np.zeros((nframe, N) + xr.shape[1:], f32), np.zeros((nframe, N) + xr.shape[1:], f32)
    for f in range(nframe):
        for k in range(P):
            t = start + (f - P + 1 + k) * N
            if t >= 0:
                hk = h[k].reshape((N,) + tail)
                yr[f] = yr[f] + hk * xr[t:t + N]
                yi[f] = yi[f] + hk * xi[t:t + N]
    return yr, yi


def _emu_windows(terms, ns):
    """The chain s = s + term over each window of ns frames of terms [nframe][...], from zero, float32."""
    out = np.zeros((terms[0].shape[0] // ns,) + terms[0].shape[1:], f32)
    for fr in range(ns):
        for t in terms:
            out = out + t[fr::ns]
    return out


def emu_beamform(stream, w, N, nbeam, h=None, start=0, ntime=None, nframe_sum=0, dual=False):
    """upchan_beamform_kernel in float32 numpy: decode, the PFB chain (with h), the FFT, the sum over inputs in input order
    (four rounded multiply-adds per input and output, in the kernel's order), then |v|^2 or the 2x2 products added frame by
    frame within each window."""
    ntime = stream.shape[0] - start if ntime is None else ntime
    nchan, ninput = stream.shape[1:]
    nframe = ntime // N
    re, im = orc.decode(np.asarray(stream))
    xr, xi = re.astype(f32), im.astype(f32)
    if h is None:
        yr = xr[start:start + ntime].reshape(nframe, N, nchan, ninput)
        yi = xi[start:start + ntime].reshape(nframe, N, nchan, ninput)
    else:
        yr, yi = _emu_pfb(xr, xi, N, h, start, nframe)
    Xr, Xi = emu_fft(yr.transpose(0, 2, 3, 1), yi.transpose(0, 2, 3, 1))        # [f][c][i][j]
    w = np.asarray(w).reshape(nchan, N, nbeam, ninput)
    wr, wi = w.real.astype(f32).transpose(2, 0, 1, 3), w.imag.astype(f32).transpose(2, 0, 1, 3)   # [b][c][j][i]
    ar, ai = np.zeros((nframe, nbeam, nchan, N), f32), np.zeros((nframe, nbeam, nchan, N), f32)
    for i in range(ninput):
        x, y = Xr[:, None, :, i, :], Xi[:, None, :, i, :]
        ar = ar + wr[..., i] * x
        ar = ar + (-wi[..., i]) * y
        ai = ai + wr[..., i] * y
        ai = ai + wi[..., i] * x
    if not nframe_sum:
        return cplx(ar, ai)
    if not dual:
        return _emu_windows([ar * ar, ai * ai], nframe_sum)
    Ar, Ai, Br, Bi = ar[:, 0::2], ai[:, 0::2], ar[:, 1::2], ai[:, 1::2]
    return np.stack([_emu_windows([Ar * Ar, Ai * Ai], nframe_sum), _emu_windows([Br * Br, Bi * Bi], nframe_sum),
                     _emu_windows([Ar * Br, Ai * Bi], nframe_sum), _emu_windows([Ai * Br, (-Ar) * Bi], nframe_sum)], axis=-1)


def emu_sum_beams(v, N, W, ntime, h=None, pair0=0, npair=None):
    """upchan_sum_beams_kernel over the stream v complex64 [nchan][nbeam][T] in gulps of ntime samples, float32 numpy: the PFB
    chain, the FFT, the four products of a frame (two rounded products and one rounded add each), the frames of a gulp added in
    order in chains of min(W, F) frames, and for W > F the gulps' partial sums added in order."""
    v = np.asarray(v, np.complex64)
    nchan, nbeam, T = v.shape
    npair = nbeam // 2 - pair0 if npair is None else npair
    v = v[:, 2 * pair0:2 * (pair0 + npair)]
    xr, xi = np.moveaxis(v.real, -1, 0).astype(f32), np.moveaxis(v.imag, -1, 0).astype(f32)     # [T][c][b]
    nframe, F = T // N, ntime // N
    if h is None:
        yr, yi = xr.reshape(nframe, N, nchan, 2 * npair), xi.reshape(nframe, N, nchan, 2 * npair)
    else:
        yr, yi = _emu_pfb(xr, xi, N, h, 0, nframe)
    Vr, Vi = emu_fft(yr.transpose(0, 2, 3, 1), yi.transpose(0, 2, 3, 1))        # [f][c][b][j]
    Ar, Ai, Br, Bi = Vr[:, :, 0::2], Vi[:, :, 0::2], Vr[:, :, 1::2], Vi[:, :, 1::2]
    prod = np.stack([Ar * Ar + Ai * Ai, Br * Br + Bi * Bi, Ar * Br + Ai * Bi, Ai * Br - Ar * Bi], axis=-1)   # [f][c][p][j][4]
    wf = min(W, F)
    part = _emu_windows([prod], wf)
    if W > F:
        g = W // F
        part = part.reshape((part.shape[0] // g, g) + part.shape[1:])
        acc = part[:, 0]
        for q in range(1, g):
            acc = acc + part[:, q]
        part = acc
    return part.transpose(0, 2, 1, 3, 4)


# ---------------------------------------------------------------- the exact power-of-two covariance
def in_range(*arrays):
    """True when every non-zero magnitude lies in [2^-100, 2^100]: then scaling by 2^k, |k| <= 40, of any fp32 value in the
    chain neither overflows nor reaches the denormals, and commutes with every rounding."""
    for a in arrays:
        a = np.abs(np.asarray(a))
        a = a[a > 0]
        if a.size and not (a.min() >= RANGE[0] and a.max() <= RANGE[1]):
            return False
    return True


def term_magnitudes(stream, w, N, nbeam, h=None, start=0, ntime=None):
    """The non-zero |w[c, j, b, i]| |X[f, c, i, j]| of a gulp: (min, max), for in_range."""
    ntime = stream.shape[0] - start if ntime is None else ntime
    nchan, ninput = stream.shape[1:]
    X = np.abs(pfb_channelise(stream, N, np.ones(N) if h is None else h, start, ntime))
    wa = np.abs(np.asarray(w).reshape(nchan, N, nbeam, ninput).astype(np.complex128))
    lo, hi = np.inf, 0.0
    for b in range(nbeam):
        t = wa[:, :, b, :].transpose(0, 2, 1)[None] * X
        t = t[t > 0]
        if t.size:
            lo, hi = min(lo, t.min()), max(hi, t.max())
    return np.array([lo, hi]) if hi > 0 else np.zeros(0)


def scale_weights(w, k):
    """w[c, j, b, :] * 2^k[c, j, b], exact in complex64."""
    s = np.ldexp(f32(1), k)[..., None]
    return cplx(w.real * s, w.imag * s)


def scale_beams(v, k):
    """v[c, b, :] * 2^k[c, b], exact in complex64."""
    s = np.ldexp(f32(1), k)[..., None]
    return cplx(v.real * s, v.imag * s)


def scaled_beamform(out, k, nframe_sum=0, dual=False):
    """What UpchanBeamform must give, bit for bit, for scale_weights(w, k) when `out` is what it gives for w; k [c][j][b]."""
    kb = np.transpose(k, (2, 0, 1))                                     # [b][c][j]
    if not nframe_sum:
        return cplx(np.ldexp(out.real, kb), np.ldexp(out.imag, kb))
    if not dual:
        return np.ldexp(out, 2 * kb)
    kx, ky = kb[0::2], kb[1::2]
    return np.ldexp(out, np.stack([2 * kx, 2 * ky, kx + ky, kx + ky], axis=-1))


def scaled_sum_beams(out, k, pair0=0, npair=None):
    """The same for UpchanSumBeams with v[c, b, :] * 2^k[c, b]: out [nwin][npair][nchan][N][4]."""
    npair = k.shape[1] // 2 - pair0 if npair is None else npair
    kx, ky = k[:, 2 * pair0:2 * (pair0 + npair):2].T, k[:, 2 * pair0 + 1:2 * (pair0 + npair):2].T    # [p][c]
    e = np.stack([2 * kx, 2 * ky, kx + ky, kx + ky], axis=-1)[:, :, None, :]
    return np.ldexp(out, e)


def pair_perm(rng, nbeam):
    """A permutation of the beams that moves whole pairs (2p, 2p+1)."""
    pp = rng.permutation(nbeam // 2)
    return np.stack([2 * pp, 2 * pp + 1], axis=1).reshape(-1)


def same_bits(a, b):
    """Word-for-word equality; returns the indices of the first few words that differ (empty: equal)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    return np.argwhere(ua != ub)[:8]


# ---------------------------------------------------------------- uneven cases
def uneven_k(rng, shape):
    """k drawn from the integers in [-20, 20]."""
    return rng.integers(-20, 21, shape).astype(np.int32)


def rand_w(rng, nchan, N, nbeam, ninput):
    return (rng.standard_normal((nchan, N, nbeam, ninput)) + 1j * rng.standard_normal((nchan, N, nbeam, ninput))).astype(np.complex64)


def uneven_weights(rng, nchan, N, nbeam, ninput):
    """standard_normal weights, a tenth of each row's inputs at 64 times the rest and a tenth at zero, every row (c, j, b)
    scaled by 2^k; returns (w, k)."""
    w = rand_w(rng, nchan, N, nbeam, ninput)
    m = rng.random((nchan, N, nbeam, ninput))
    w = (w * np.where(m < 0.1, 64, np.where(m < 0.2, 0, 1))).astype(np.complex64)
    k = uneven_k(rng, (nchan, N, nbeam))
    return scale_weights(w, k), k


def pack(re, im):
    """4+4-bit samples from integer arrays in -8..7."""
    return (((np.asarray(re) & 0xF) << 4) | (np.asarray(im) & 0xF)).astype(np.uint8)


def lowpass_prototype(ntap, N):
    """A real low-pass prototype, Hann-windowed sinc with its cutoff at one fine channel: its taps span several decades."""
    n = np.arange(ntap * N) + 0.5
    x = n / N - ntap / 2
    return (np.sinc(x) * np.sin(np.pi * n / (ntap * N)) ** 2).astype(np.float32)


def rand_beams(rng, nchan, nbeam, T):
    return (rng.standard_normal((nchan, nbeam, T)) + 1j * rng.standard_normal((nchan, nbeam, T))).astype(np.complex64)


# ---------------------------------------------------------------- the cases of the row bar (CPU margins and GPU tests share them)
# 52 inputs (chunks of 16 + 16 + 16 + 4).  A row's fp32 error grows with the number of inputs: at 64 the emulation reached 2.52e-6
# of one row's RMS (power, N = 64, 6 beams, windows of 3), past the quarter of the bar that tests/test_upchan_local_cpu.py keeps
# between the emulation and the bar; at 52 its worst row is at 2.35e-6.
ROW_NINPUT, ROW_NCHAN, ROW_NFRAME, ROW_NTAP = 52, 3, 12, 4


def beamform_points():
    """(mode, N, nbeam, nframe, nframe_sum) of the covariance tests and of the row bar alike: 1 beam per thread (N = 8 to 32), 2
    (6 beams at N = 64; 5 beams: beams 5..7 masked) and 4 (16 beams); windows of 3 frames (runs of 6: two windows close inside an
    8-frame sub-tile; 9 frames: the last work-group holds half a run) and of 12."""
    pts = [("voltage", N, 6, 12, 0) for N in (8, 16, 32, 64)] + [("voltage", 64, 16, 12, 0), ("voltage", 64, 5, 12, 0), ("voltage", 64, 5, 9, 0)]
    for ns in (3, 12):
        pts += [("power", 8, 6, 12, ns), ("power", 64, 6, 12, ns), ("power", 64, 16, 12, ns), ("power", 64, 5, 12, ns)]
        pts += [("dual", 8, 6, 12, ns), ("dual", 64, 6, 12, ns), ("dual", 64, 16, 12, ns)]
    return pts + [("power", 8, 6, 9, 3), ("power", 64, 5, 9, 3), ("dual", 8, 6, 9, 3), ("dual", 64, 16, 9, 3)]
BEAMFORM_CASES = ("uneven", "zero_beam", "zero_chan", "small_chan")


def beamform_case(name, N, nbeam, pfb, seed=0, nframe=ROW_NFRAME, ninput=ROW_NINPUT, nchan=ROW_NCHAN):
    """(stream, w, h) of two gulps of nframe frames: uniform random bytes and uneven_weights (2^k rows), plus
      zero_beam    beam 1 all zero
      zero_chan    coarse channel 1 all-zero bytes
      small_chan   coarse channel 0 with nibbles in -1..1 next to the full-range ones
      tone         an amplitude-7 tone in fine channel N/4 + 1 on a quarter of the inputs over +-1 noise
    h (pfb): the ROW_NTAP-tap low-pass prototype, else None."""
    rng = np.random.default_rng([seed, N, nbeam, int(pfb), BEAMFORM_CASES.index(name) if name in BEAMFORM_CASES else 9])
    T = 2 * nframe * N
    stream = rng.integers(0, 256, (T, nchan, ninput), dtype=np.uint8)
    w, _ = uneven_weights(rng, nchan, N, nbeam, ninput)
    if name == "zero_beam":
        w[:, :, 1, :] = 0
    elif name == "zero_chan":
        stream[:, 1, :] = 0
    elif name == "small_chan":
        stream[:, 0, :] = pack(rng.integers(-1, 2, (T, ninput)), rng.integers(-1, 2, (T, ninput)))
    elif name == "tone":
        t = np.arange(T)[:, None, None]
        tone = 7 * np.exp(2j * np.pi * (N // 4 + 1 - N // 2) * t / N) * (np.arange(ninput) % 4 == 0)
        nr, ni = rng.integers(-1, 2, stream.shape), rng.integers(-1, 2, stream.shape)
        stream = pack(np.clip(np.rint(tone.real).astype(int) + nr, -8, 7), np.clip(np.rint(tone.imag).astype(int) + ni, -8, 7))
    else:
        assert name == "uneven", name
    return stream, w, (lowpass_prototype(ROW_NTAP, N) if pfb else None)


SUM_NCHAN, SUM_NBEAM, SUM_NTIME, SUM_NGULP = 3, 8, 512, 4
SUM_CASES = ("uneven", "loud_x_quiet_y", "zero_beam", "burst")


def sum_beams_case(name, N, pfb, seed=0):
    """(v, h): standard_normal beams [3][8][4 * 512] with
      uneven           every (channel, beam) scaled by 2^k
      loud_x_quiet_y   X at 2^20, Y at 2^-20 in every pair
      zero_beam        beam 3 (Y of pair 1) all zero
      burst            the samples of gulp 1's first half (one window of F / 2 frames) 2^15 louder (for the plain FFT)
    h (pfb): the 4-tap low-pass prototype, else None."""
    rng = np.random.default_rng([seed, N, int(pfb), SUM_CASES.index(name)])
    v = rand_beams(rng, SUM_NCHAN, SUM_NBEAM, SUM_NGULP * SUM_NTIME)
    if name == "uneven":
        v = scale_beams(v, uneven_k(rng, (SUM_NCHAN, SUM_NBEAM)))
    elif name == "loud_x_quiet_y":
        v = scale_beams(v, np.tile(np.array([20, -20], np.int32), (SUM_NCHAN, SUM_NBEAM // 2)))
    elif name == "zero_beam":
        v[:, 3] = 0
    else:
        assert name == "burst", name
        win = slice(SUM_NTIME, SUM_NTIME + SUM_NTIME // 2)
        v[..., win] = scale_beams(v[..., win], np.full((SUM_NCHAN, SUM_NBEAM), 15, np.int32))
    return v, (lowpass_prototype(ROW_NTAP, N) if pfb else None)
