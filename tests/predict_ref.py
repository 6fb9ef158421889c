"""The contract of xengPredict* (include/xeng.h, "Component lists subtracted from the visibilities") restated in numpy: float64 (the
model by one einsum per product), and float32 in the contract's own order -- z = C a with the stated fused multiply-adds, then per
word and part the fma chain over the records two at a time (the gap between the two on a test's own inputs is a fifth of that test's
bar; with `libm=True` the phase factors are the emulation's, sine and cosine in double precision rounded once, and the result is
what the kernel's source gives on host threads bit for bit); the error measure; a generator of cases on tests/gaincal_ref.py's array
of 1.2 km."""
import math

import numpy as np

from caltech_bifrost_dsp_amd.blocks.imaging import CLEAN_COMPONENT
from tests.gaincal_ref import corrupt, model, noisy, setup, steering

SUBTRACT, MODEL = 0, 1


def records(ngroup, ncomp_max):
    """[ngroup][ncomp_max] empty records"""
    rec = np.zeros((ngroup, ncomp_max), CLEAN_COMPONENT)
    rec['pixel'] = -1
    return rec


def last_filled(rec_g):
    """one past the last filled record of a group's list"""
    k = np.flatnonzero(rec_g['pixel'] >= 0)
    return int(k[-1]) + 1 if k.size else 0


def model64(freq, tau, comps, nfavg, cross):
    """M complex128 [nfine][nstand][2][nstand][2], every word of it"""
    freq, tau = np.asarray(freq, np.float64), np.asarray(tau, np.float64)
    nstand = tau.shape[1]
    M = np.zeros((len(freq), nstand, 2, nstand, 2), np.complex128)
    for g in range(comps.shape[0]):
        rec = comps[g][comps[g]['pixel'] >= 0]
        if not rec.size:
            continue
        ch = slice(g * nfavg, (g + 1) * nfavg)
        a = steering(freq[ch], tau[rec['pixel']])
        C = rec['C'].astype(np.float64)
        for (p, q), w in (((0, 0), C[:, 0]), ((1, 1), C[:, 1]), ((0, 1), C[:, 2] + 1j * C[:, 3]), ((1, 0), C[:, 2] - 1j * C[:, 3])):
            if p == q or cross:
                M[ch, :, p, :, q] = np.einsum('cks,ckt->cst', w[None, :, None] * a, np.conj(a))
    return M


def _fma32(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def steering32(freq, tau_rows, libm=False):
    """(Re a, Im a) float32 [nfine][k][nstand]: the product and its fraction of a turn float64, then single precision; with `libm`
    the sine and cosine of pi (2 fr) in double precision, rounded once (tests/predict_emul/hip/hip_runtime.h's sincospif)."""
    turns = np.asarray(freq, np.float64)[:, None, None] * np.asarray(tau_rows, np.float64)[None]
    fr = (turns - np.rint(turns)).astype(np.float32)
    if libm:
        x = math.pi * (np.float32(2.0) * fr).astype(np.float64)
        cs = np.vectorize(math.cos, otypes=[np.float64])(x).astype(np.float32)
        sn = np.vectorize(math.sin, otypes=[np.float64])(x).astype(np.float32)
    else:
        ang = np.float32(2.0 * np.pi) * fr
        cs, sn = np.cos(ang), np.sin(ang)
    assert cs.dtype == np.float32
    return cs, -sn


def model32(freq, tau, comps, nfavg, cross, libm=False):
    """M complex64 in the kernel's order: per group the records up to the last filled one, rounded up to a pair (an empty record:
    zero operands), per pair and product  re: zr br (k even, odd), zi bi (even, odd);  im: zi br (even, odd), (-zr) bi (even, odd)."""
    freq, tau = np.asarray(freq, np.float64), np.asarray(tau, np.float64)
    nfine, nstand = len(freq), tau.shape[1]
    M = np.zeros((nfine, nstand, 2, nstand, 2), np.complex64)
    for g in range(comps.shape[0]):
        nr = last_filled(comps[g])
        if not nr:
            continue
        nk = (nr + 1) & ~1
        rec = records(1, nk)[0]
        rec[:nr] = comps[g][:nr]
        live = rec['pixel'] >= 0
        ch = slice(g * nfavg, (g + 1) * nfavg)
        ar, ai = steering32(freq[ch], tau[np.where(live, rec['pixel'], 0)], libm)
        ar, ai = np.where(live[None, :, None], ar, np.float32(0)), np.where(live[None, :, None], ai, np.float32(0))
        C = np.where(live[:, None], rec['C'], np.float32(0)).astype(np.float32)[None, :, :, None]        # [1][k][4][1]
        cxx, cyy, cre, cim = C[:, :, 0], C[:, :, 1], C[:, :, 2], C[:, :, 3]
        prods = [((0, 0), cxx * ar, cxx * ai), ((1, 1), cyy * ar, cyy * ai)]
        if cross:
            prods.append(((0, 1), _fma32(cre, ar, -(cim * ai)), _fma32(cre, ai, cim * ar)))
            prods.append(((1, 0), _fma32(cre, ar, cim * ai), _fma32(cre, ai, -(cim * ar))))
        for (p, q), zr, zi in prods:
            assert zr.dtype == np.float32 and zi.dtype == np.float32
            re = np.zeros((zr.shape[0], nstand, nstand), np.float32)
            im = np.zeros_like(re)
            for k in range(0, nk, 2):
                for x, y in ((zr, ar), (zi, ai)):
                    for kk in (k, k + 1):
                        re = _fma32(x[:, kk, :, None], y[:, kk, None, :], re)
                for x, y in ((zi, ar), (-zr, ai)):
                    for kk in (k, k + 1):
                        im = _fma32(x[:, kk, :, None], y[:, kk, None, :], im)
            M[ch, :, p, :, q] = re + 1j * im
    return M


def predict(V, freq, tau, comps, nfavg, cross=True, mode=SUBTRACT, dtype=np.complex128, libm=False):
    """The output of a Run: complex `dtype` [nfine][nstand][2][nstand][2].  Only the words i >= j of V are looked at (V may be None
    in model mode); the upper triangle is the conjugate of the lower, the diagonal real."""
    dtype = np.dtype(dtype)
    freq = np.asarray(freq, np.float64)
    nfine, nstand = len(freq), np.shape(tau)[1]
    n = 2 * nstand
    M = (model32(freq, tau, comps, nfavg, cross, libm) if dtype == np.complex64 else model64(freq, tau, comps, nfavg, cross)).reshape(nfine, n, n)
    if mode == MODEL:
        Y = M
    else:
        with np.errstate(invalid='ignore'):
            Y = np.asarray(V).reshape(nfine, n, n).astype(dtype) - M
    assert Y.dtype == dtype
    low = np.tril(np.ones((n, n), bool), -1)[None]
    out = np.where(low, Y, np.conj(Y.transpose(0, 2, 1)))       # (the mirrored word: the sign of the imaginary part turned, of a zero too)
    out[:, np.arange(n), np.arange(n)] = np.einsum('cii->ci', Y).real
    return out.reshape(nfine, nstand, 2, nstand, 2)


def scale(V, comps, nfavg):
    """max|V| + sum_k (|C_XX| + |C_YY| + 2 |C_Re + i C_Im|) per channel, f64 [nfine][1][1]: what an error is measured against.  max|V|
    is over the finite words of the channel's lower triangle (0 where V is None: model mode)."""
    C = np.where((comps['pixel'] >= 0)[:, :, None], comps['C'], 0).astype(np.float64)
    cs = (np.abs(C[:, :, 0]) + np.abs(C[:, :, 1]) + 2 * np.hypot(C[:, :, 2], C[:, :, 3])).sum(axis=1)
    sc = np.repeat(cs, nfavg)
    if V is not None:
        V = np.asarray(V)
        nfine, nstand = V.shape[:2]
        n = 2 * nstand
        A = np.abs(np.where(np.tril(np.ones((n, n), bool))[None], V.reshape(nfine, n, n), 0).astype(np.complex128))
        sc = sc + np.where(np.isfinite(A), A, 0).max(axis=(1, 2))
    return sc[:, None, None]


def word_error(got, ref, sc):
    """|got - ref| / scale per word [nfine][n][n]; 0 where both the difference and the scale are 0."""
    nfine = sc.shape[0]
    ref = np.asarray(ref, np.complex128)
    n = ref.shape[1] * 2
    d = np.abs(np.asarray(got, np.complex128).reshape(nfine, n, n) - ref.reshape(nfine, n, n))
    sc = np.broadcast_to(sc, d.shape)
    return np.where(sc > 0, d / np.where(sc > 0, sc, 1), np.where(d > 0, np.inf, 0.0))


def float_gap(V, freq, tau, comps, nfavg, cross=True, mode=SUBTRACT, ref=None):
    """The worst word_error of the float32 evaluation against the float64 one: a fifth of the float bar."""
    ref = predict(V, freq, tau, comps, nfavg, cross, mode) if ref is None else ref
    return float(word_error(predict(V, freq, tau, comps, nfavg, cross, mode, np.complex64), ref, scale(None if mode == MODEL else V, comps, nfavg)).max())


def upper_nan(V):
    """V with every word above the diagonal replaced by NaN: nothing may read them."""
    nfine, nstand = V.shape[:2]
    n = 2 * nstand
    up = np.triu(np.ones((n, n), bool), 1)
    return np.where(up[None], np.complex64(complex(np.nan, np.nan)), V.reshape(nfine, n, n)).reshape(V.shape).astype(np.complex64)


def case(nstand, ncomp, nfine, nfavg, ncomp_max=None, seed=None, noise=0.05, spare=3):
    """(tau [ndir][nstand], freq, comps CLEAN_COMPONENT [nfine / nfavg][ncomp_max], V c64): tests/gaincal_ref.py's array of 1.2 km and
    its sky of ndir = (pixels used) + `spare` directions; V = g g^H o M of three of them plus Hermitian noise of uneven rows, the cross
    hands included.  Each group has a list of its own of `ncomp` records: words of either sign between -2 and 3, the cross-hand words
    included; a pixel that repeats (records 0 and 2); empty records in the middle (record 1 where ncomp > 3, every fifth after it) whose
    other words hold NaN; the last record filled, so that an odd ncomp ends on half a pair."""
    ncomp_max = ncomp if ncomp_max is None else ncomp_max
    nused = max(ncomp - 1, 1)
    ndir = nused + spare
    rng, tau, freq, flux, w, g = setup(300 + nstand if seed is None else seed, nstand, ndir, nfine)
    V = noisy(rng, corrupt(model(freq, tau[:3], flux[:, :3]), g), noise)
    ngroup = nfine // nfavg
    comps = records(ngroup, ncomp_max)
    for grp in range(ngroup):
        r = comps[grp]
        r['pixel'][:ncomp] = rng.integers(0, nused, ncomp)
        if ncomp > 2:
            r['pixel'][2] = r['pixel'][0]
        r['C'][:ncomp] = rng.uniform(-2.0, 3.0, (ncomp, 4))
        r['I'][:ncomp] = r['C'][:ncomp, 0] + r['C'][:ncomp, 1]
        if ncomp > 3:
            for k in [1] + list(range(6, ncomp - 1, 5)):
                r[k] = (-1, np.nan, np.full(4, np.nan), 0)
    return tau, freq, comps, V


def integer_case(nstand, ncomp, nfine, nfavg, ncomp_max, seed=7):
    """(V Gaussian-integer Hermitian c64, comps with integer words of either sign and an empty record, V - sum C on every product)"""
    rng = np.random.default_rng(seed)
    n = 2 * nstand
    Z = rng.integers(-50, 51, (nfine, n, n)) + 1j * rng.integers(-50, 51, (nfine, n, n))
    L = np.where(np.tril(np.ones((n, n), bool), -1)[None], Z, 0)
    Z = L + np.conj(L.transpose(0, 2, 1)) + np.einsum('ci,ij->cij', rng.integers(1, 99, (nfine, n)), np.eye(n))
    V = Z.astype(np.complex64).reshape(nfine, nstand, 2, nstand, 2)
    comps = records(nfine // nfavg, ncomp_max)
    comps['pixel'][:, :ncomp] = rng.integers(0, 4, (nfine // nfavg, ncomp))
    comps['C'][:, :ncomp] = rng.integers(-9, 10, (nfine // nfavg, ncomp, 4))
    if ncomp > 2:
        comps['pixel'][:, 1] = -1
    C = np.where((comps['pixel'] >= 0)[:, :, None], comps['C'], 0).astype(np.float64).sum(axis=1)       # [ngroup][4]
    C = np.repeat(C, nfavg, axis=0)
    exp = V.astype(np.complex128)
    exp[:, :, 0, :, 0] -= C[:, 0, None, None]
    exp[:, :, 1, :, 1] -= C[:, 1, None, None]
    exp[:, :, 0, :, 1] -= (C[:, 2] + 1j * C[:, 3])[:, None, None]
    exp[:, :, 1, :, 0] -= (C[:, 2] - 1j * C[:, 3])[:, None, None]
    d = np.arange(n)
    E = exp.reshape(nfine, n, n)
    E[:, d, d] = E[:, d, d].real
    return V, comps, exp
