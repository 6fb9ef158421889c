"""Plain numpy restatement of the beamformer's precision control and of the int8x3 arithmetic, and the per-row error
measures of the beamformer tests.

Written from the comment block "precision of the fixed-point weights" in csrc/beamform_kernels.h (not from the kernels):

  per (channel, beam) row of complex64 weights, with a = max(|re|, |im|) of an entry and e = a's fp32 exponent field
    * E  = the smallest e-bucket with at most ROW_OUT entries above it, none of them within GAP_BINADES binades of it;
    * the entries above E are the row's outliers, m = the exact maximum of a over the rest (the inliers);
    * the guard: among the entries with a non-zero exponent field (zeros and denormals do not count), Emed / Elow = the
      largest bucket with at least 1/2 / at least LOW_NUM / LOW_DEN = 7/8 of them at or above it (the median and the
      lower-eighth entry); the row asks for the bf16x3 route when exponent(m) - Emed > GUARD_BINADES or
      Emed - Elow > SPREAD_BINADES;
  per (channel, tile of 32 beams)
    * routed = any row's guard, or more than TILE_OUT distinct outlier inputs in the tile;
    * the sorted union of the rows' outlier inputs.
"""
import numpy as np

BEAM_RTOL = 1e-5            # BASELINE.json north_star: "beamformer fp32 within 1e-5 rel" -- here per (channel, beam) row

ROW_OUT = 8
TILE_OUT = 32
GUARD_BINADES = 4
GAP_BINADES = 3
SPREAD_BINADES = 3
LOW_NUM, LOW_DEN = 7, 8      # the lower-eighth entry: 7/8 of the non-zero entries lie at or above bucket Elow
QMAX = 127 * (255 * 255 + 255 + 1)


class Route:
    """Result of route(): per row E, nout, is_out, m, guard; per tile routed, union; totals tiles_bf16, outlier_inputs."""


def exponent_field(a):
    return ((np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)


def route(w, spread_guard=True):
    """spread_guard=False: the rule without its second clause (the median guard alone), for the record of what it cost."""
    w = np.ascontiguousarray(w, dtype=np.complex64)
    nchan, nbeam, ninput = w.shape
    a = np.maximum(np.abs(w.real), np.abs(w.imag)).reshape(-1, ninput)           # float32, exact
    e = exponent_field(a)
    nrow = a.shape[0]
    cnt = np.bincount((np.arange(nrow)[:, None] * 256 + e).ravel(), minlength=nrow * 256).reshape(nrow, 256)
    atleast = np.cumsum(cnt[:, ::-1], axis=1)[:, ::-1]                          # entries with exponent >= b
    above = np.concatenate([atleast[:, 1:], np.zeros((nrow, 1), np.int64)], axis=1)
    shifted = above[:, np.minimum(np.arange(256) + GAP_BINADES, 255)]
    ok = (above <= ROW_OUT) & (above == shifted)                                 # bucket 255 always qualifies
    E = np.argmax(ok, axis=1)
    is_out = e > E[:, None]
    m = np.max(np.where(is_out, np.float32(0), a), axis=1).astype(np.float32)
    n_nz = atleast[:, 1]
    b = np.arange(256)

    def quantile_bucket(num, den):
        qual = (den * atleast >= num * n_nz[:, None]) & (b >= 1)[None, :]
        return np.max(np.where(qual, b[None, :], 0), axis=1)
    Emed, Elow = quantile_bucket(1, 2), quantile_bucket(LOW_NUM, LOW_DEN)
    guard = exponent_field(m) - Emed > GUARD_BINADES
    if spread_guard:
        guard = guard | (Emed - Elow > SPREAD_BINADES)
    guard = guard & (n_nz > 0)

    r = Route()
    r.E = E.reshape(nchan, nbeam)
    r.is_out = is_out.reshape(nchan, nbeam, ninput)
    r.nout = r.is_out.sum(axis=2)
    r.m = m.reshape(nchan, nbeam)
    r.Emed, r.Elow = Emed.reshape(nchan, nbeam), Elow.reshape(nchan, nbeam)
    r.guard = guard.reshape(nchan, nbeam)
    nbt = (nbeam + 31) // 32
    r.routed = np.zeros((nchan, nbt), bool)
    r.union = [[None] * nbt for _ in range(nchan)]
    for c in range(nchan):
        for t in range(nbt):
            rows = slice(32 * t, min(32 * t + 32, nbeam))
            u = np.flatnonzero(r.is_out[c, rows].any(axis=0))
            r.union[c][t] = u
            r.routed[c, t] = bool(r.guard[c, rows].any()) or len(u) > TILE_OUT
    r.tiles_total = nchan * nbt
    r.tiles_bf16 = int(r.routed.sum())
    r.outlier_inputs = int(sum(len(r.union[c][t]) for c in range(nchan) for t in range(nbt) if not r.routed[c, t]))
    return r


def unpack(vin):
    """uint8[ntime][nchan][ninput] 4+4-bit voltages (high nibble real, low nibble imaginary, two's complement) -> two
    int64 arrays [nchan][ninput][ntime]."""
    v = np.ascontiguousarray(vin, dtype=np.uint8).astype(np.int64)
    re, im = v >> 4, v & 15
    re, im = re - 16 * (re >= 8), im - 16 * (im >= 8)
    return re.transpose(1, 2, 0), im.transpose(1, 2, 0)


def beams_f64(vin, w):
    """The float64 reference: complex128 [nchan][nbeam][ntime]."""
    re, im = unpack(vin)
    return np.einsum("cbi,cit->cbt", np.asarray(w).astype(np.complex128), re + 1j * im)


def beams_c64(vin, w):
    """Input-by-input accumulation in complex64, like an fp32 GEMM: what shows that the per-row bar is reachable."""
    re, im = unpack(vin)
    x = (re + 1j * im).astype(np.complex64)
    w = np.asarray(w, dtype=np.complex64)
    acc = np.zeros((w.shape[0], w.shape[1], x.shape[2]), np.complex64)
    for i in range(w.shape[2]):
        acc += w[:, :, i, None] * x[:, None, i, :]
    return acc


def balanced_digits(q):
    """q -> three balanced base-255 digits in [-127, 127], most significant first."""
    d3 = (q + 127) % 255 - 127
    q = (q - d3) // 255
    d2 = (q + 127) % 255 - 127
    d1 = (q - d2) // 255
    assert np.all(np.abs(d1) <= 127)
    return d1, d2, d3


def int8x3_beams(vin, w, r=None):
    """The int8x3 route's arithmetic on the CPU: digits q = clip(rint(w * QMAX / m)) of the inliers (outliers: zero
    digits), exact integer sums per digit plane against 16 x the voltages, the fp32 recombination
    (m / QMAX / 16) * ((T1 * 255^2 + T2 * 255) + T3), then the outlier products added in fp32 in the order of the tile's
    sorted union.  Tiles that the rule routes to bf16x3 (every weight exact to 24 bits) get the float64 reference.
    Returns complex64 [nchan][nbeam][ntime]."""
    w = np.ascontiguousarray(w, dtype=np.complex64)
    r = route(w) if r is None else r
    nchan, nbeam, ninput = w.shape
    re, im = unpack(vin)
    f32 = np.float32
    m = r.m
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = np.where(m > 0, f32(QMAX) / m, f32(0)).astype(f32)[:, :, None]
        qr = np.clip(np.rint((w.real * inv).astype(f32)), -QMAX, QMAX)
        qi = np.clip(np.rint((w.imag * inv).astype(f32)), -QMAX, QMAX)
    qr = np.where(r.is_out, 0, qr).astype(np.int64)
    qi = np.where(r.is_out, 0, qi).astype(np.int64)
    scale = np.where(m > 0, m / f32(QMAX) / f32(16), f32(0)).astype(f32)[:, :, None]
    o_re = np.zeros((nchan, nbeam, re.shape[2]), f32)
    o_im = np.zeros_like(o_re)
    for k, (dr, di) in enumerate(zip(balanced_digits(qr), balanced_digits(qi))):
        t_re = 16 * (np.einsum("cbi,cit->cbt", dr, re) - np.einsum("cbi,cit->cbt", di, im))
        t_im = 16 * (np.einsum("cbi,cit->cbt", dr, im) + np.einsum("cbi,cit->cbt", di, re))
        f = f32((65025.0, 255.0, 1.0)[k])
        if k < 2:
            o_re, o_im = o_re + t_re.astype(f32) * f, o_im + t_im.astype(f32) * f
        else:
            o_re, o_im = o_re + t_re.astype(f32), o_im + t_im.astype(f32)
    o_re, o_im = scale * o_re, scale * o_im
    exact = None
    for c in range(nchan):
        for t in range(len(r.union[c])):
            rows = slice(32 * t, min(32 * t + 32, nbeam))
            if r.routed[c, t]:
                exact = beams_f64(vin, w) if exact is None else exact
                o_re[c, rows], o_im[c, rows] = exact[c, rows].real, exact[c, rows].imag
                continue
            for i in r.union[c][t]:
                R = np.where(r.is_out[c, rows, i], w[c, rows, i], np.complex64(0))
                xr, xi = re[c, i].astype(f32)[None, :], im[c, i].astype(f32)[None, :]
                Rx, Ry = R.real[:, None], R.imag[:, None]
                o_re[c, rows] += Rx * xr - Ry * xi
                o_im[c, rows] += Rx * xi + Ry * xr
    return (o_re + 1j * o_im).astype(np.complex64)


def row_errors(got, exp):
    """max_t |got - exp| / sqrt(mean_t |exp|^2) per (channel, beam); rows whose reference is identically zero: 0 where
    got is exactly zero, inf otherwise."""
    got, exp = np.asarray(got).astype(np.complex128), np.asarray(exp).astype(np.complex128)
    rms = np.sqrt(np.mean(np.abs(exp) ** 2, axis=-1))
    err = np.max(np.abs(got - exp), axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(rms > 0, err / rms, np.where(err == 0, 0.0, np.inf))
    return rel


def check_beams_rows(got, exp, rtol=BEAM_RTOL):
    """Every (channel, beam) row within rtol of its OWN RMS (a zero reference row: exactly zero).  Returns the worst row's
    figure and its index."""
    assert np.all(np.isfinite(got))
    rel = row_errors(got, exp)
    k = np.unravel_index(np.argmax(rel), rel.shape)
    assert rel[k] <= rtol, "row (channel %d, beam %d): max err / row rms = %.3e" % (k[0], k[1], rel[k])
    return float(rel[k]), tuple(int(i) for i in k)


def power_f64(v, ntime_sum):
    """float64 [npair][nblk][nchan][4] = (XX, YY, Re XY*, Im XY*) of voltages [nchan][nbeam][ntime], X = beam 2p, Y = 2p+1."""
    v = np.asarray(v).astype(np.complex128)
    nchan, nbeam, ntime = v.shape
    nblk = ntime // ntime_sum
    v = v[:, :2 * (nbeam // 2), :nblk * ntime_sum].reshape(nchan, nbeam // 2, 2, nblk, ntime_sum)
    x, y = v[:, :, 0], v[:, :, 1]
    xy = np.sum(x * np.conj(y), axis=-1)
    p = np.stack([np.sum(np.abs(x) ** 2, -1), np.sum(np.abs(y) ** 2, -1), xy.real, xy.imag], axis=-1)   # [c][p][blk][4]
    return p.transpose(1, 2, 0, 3)


def check_power_rows(got, ref_voltages, ntime_sum, eps):
    """Power sums [npair][nblk][nchan][4] against the float64 power of ref_voltages [nchan][nbeam][ntime], with a bound
    of its own per (pair, block, channel).  n = ntime_sum, u = 2^-24 (fp32 unit roundoff), X / Y the block's float64
    sums of |x|^2 / |y|^2, scale S = X for XX, Y for YY, sqrt(X Y) for both cross terms.

    Summation term, (n + 3) u S: a term of the sum is two products and an add, three roundings, so it is within 3u of
    |xr yr| + |xi yi| <= |x||y|; summing n of them in ANY order adds at most n - 1 roundings, each u of a partial sum,
    and every partial sum of the magnitudes is <= sum |x||y| <= sqrt(X Y) (Cauchy-Schwarz; = X for x = y).  Total
    (n + 2) u S to first order; n + 3 covers the second-order terms for any n < 2^20.

    eps = 0: ref_voltages are the device's own complex64 voltages (xengBeamformIntegrate): the summation term alone.

    eps > 0: ref_voltages are the float64 reference and the device's voltages are v + dv with |dv_t| <= eps R, R the row's
    RMS over the gulp (the per-row bar of check_beams_rows).  Then per row and block
        | sum |v + dv|^2 - |v|^2 | <= sum 2|v||dv| + |dv|^2 <= 2 eps R sqrt(n X) + n eps^2 R^2      (Cauchy-Schwarz),
    and for the cross terms
        | sum (x + dx)(y + dy)* - x y* | <= eps Ry sqrt(n X) + eps Rx sqrt(n Y) + n eps^2 Rx Ry,
    which bounds both components.  The summation term then applies to the perturbed sums: (n + 3) u (S + propagation).
    Returns the worst error / bound (0 where both are zero)."""
    got = np.asarray(got, dtype=np.float64)
    v = np.asarray(ref_voltages).astype(np.complex128)
    nchan, nbeam, ntime = v.shape
    n = ntime_sum
    ref = power_f64(v, n)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    R = np.sqrt(np.mean(np.abs(v) ** 2, axis=-1))                                   # [nchan][nbeam]
    Rx, Ry = R[:, 0:2 * (nbeam // 2):2].T[:, None, :], R[:, 1:2 * (nbeam // 2):2].T[:, None, :]   # [npair][1][nchan]
    X, Y = ref[..., 0], ref[..., 1]
    prop_x = 2 * eps * Rx * np.sqrt(n * X) + n * eps ** 2 * Rx ** 2
    prop_y = 2 * eps * Ry * np.sqrt(n * Y) + n * eps ** 2 * Ry ** 2
    prop_c = eps * Ry * np.sqrt(n * X) + eps * Rx * np.sqrt(n * Y) + n * eps ** 2 * Rx * Ry
    u = 2.0 ** -24
    S = np.stack([X, Y, np.sqrt(X * Y), np.sqrt(X * Y)], axis=-1)
    prop = np.stack([prop_x, prop_y, prop_c, prop_c], axis=-1)
    bound = prop + (n + 3) * u * (S + prop)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    k = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[k] <= 1.0, "power (pair %d, block %d, channel %d, term %d): err %.3e > bound %.3e (ref %.6e)" % (
        k + (err[k], bound[k], ref[k]))
    return float(ratio[k])
