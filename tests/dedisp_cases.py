"""Shapes and float data shared by the tests that hold xengDedisp* to the contract's summation order bit for bit
(tests/test_dedisp_cpu.py, tests/test_dedisp_emul_cpu.py, tests/test_dedisp_gpu.py).  Every case is a fixed function of its name
and nprod.  max_delay = S, so the ring has L = S + nwin slots."""
import numpy as np

CASES = {
    # (a) nfine 70: three ingest tiles with the last ragged, Q = 18 and a last segment of 16 channels; calls of 1..5 windows give
    #     tiles of 1, 2, 4 and 8 windows with idle lanes along time (3, 5 of 4, 8) and along the trials (5 of 8, 16, ...); L = 16,
    #     55 windows: the ring wraps three times
    "a": dict(npair=2, nfine=70, nwin=5, ndm=5, S=11, calls=[5, 1, 3, 5, 2, 4, 5, 5, 1, 1, 5, 5]),
    # (b) fewer channels than segments: Q = 1, segment 3 is empty
    "b": dict(npair=1, nfine=3, nwin=3, ndm=1, S=2, calls=[3, 1, 2, 3, 3]),
    # (c) more windows than a wave has lanes: TT = 64; calls of 70 and 65 take two time tiles, the second with 6 and 1 live
    #     windows, and the call of 33 leaves 31 idle lanes in its only tile; the ingest grid's z is 3, 2, 2, 3
    "c": dict(npair=1, nfine=40, nwin=70, ndm=3, S=5, calls=[70, 33, 64, 65]),
    # (d) no delay at all: L = nwin, every call starts where the last one ended and wraps
    "d": dict(npair=2, nfine=70, nwin=5, ndm=5, S=0, calls=[5, 2, 5, 1, 4]),
}


def float_case(name, nprod):
    """(x f32 [sum calls][npair][nfine][4], delays i32 [ndm][nfine], w f32 [nfine]): chi^2-like powers (cross words normal for
    nprod 4), any delays 0..S with S reached, weights in [0.5, 1.5] with an eighth exactly 0 -- and NaN in those channels."""
    c = CASES[name]
    rng = np.random.default_rng(100 * sorted(CASES).index(name) + nprod)
    total, npair, nfine, ndm, S = sum(c["calls"]), c["npair"], c["nfine"], c["ndm"], c["S"]
    x = rng.chisquare(4, (total, npair, nfine, 4)).astype(np.float32)
    if nprod == 4:
        x[..., 2:] = rng.standard_normal((total, npair, nfine, 2)).astype(np.float32)
    s = rng.integers(0, S + 1, (ndm, nfine)).astype(np.int32)
    s[rng.integers(ndm), rng.integers(nfine)] = S
    w = rng.uniform(0.5, 1.5, nfine).astype(np.float32)
    off = rng.choice(nfine, (nfine + 7) // 8, replace=False) if nfine >= 8 else np.array([1])
    w[off] = 0
    x[:, :, off] = np.nan
    return x, s, w
