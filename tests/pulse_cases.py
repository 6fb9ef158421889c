"""Shapes, call sizes and data shared by the tests of xengPulse* (tests/test_pulse_gpu.py, tests/test_pulse_emul_cpu.py).  Every
case is a fixed function of its arguments."""
import numpy as np

from tests.pulse_ref import pulse_search, series


def _sizes(rng, total, nwin, choices=None):
    out = []
    while total:
        nc = int(rng.choice(choices)) if choices else int(rng.integers(1, nwin + 1))
        out.append(min(total, nc))
        total -= out[-1]
    return out


INT_CASES = {
    # npair, ndm, nprod, nwidth, nstat, windows, seed (checked on the CPU: every winner leads, see integer_case)
    "111 series, I, 4 widths": (3, 37, 1, 4, 16, 110, 0),
    "128 series, XX+YY, 4 widths": (2, 64, 4, 4, 16, 110, 0),
    "111 series, XX+YY, no tail": (3, 37, 4, 1, 16, 110, 0),
    "128 series, I, a tail of 127 windows": (2, 64, 1, 8, 128, 512, 3),
    "111 series, XX+YY, a tail of 127 windows": (3, 37, 4, 8, 128, 512, 10),
}
FIXED_SIZES = [7, 1, 1, 7, 1, 30, 1, 1, 7, 7, 1, 1, 30, 7, 1, 1, 1, 1, 1, 1, 1, 1]       # 110 windows


def integer_case(name):
    """(x, sizes, float32 restatement, float64 reference) of a case.  Values 0..49; per series two planted box pulses of
    amplitude 40-200 per window.  With nstat = 16 the calls are FIXED_SIZES: windows 0, 16, 48, 64 are the first window of a call,
    32 and 80 inner ones, 16, 63, 64 the last (window 15, a block's last, ends a call too); with nstat = 128 a random sequence
    of 1, 7 and 30."""
    npair, ndm, nprod, nwidth, nstat, total, seed = INT_CASES[name]
    rng = np.random.default_rng([seed, sorted(INT_CASES).index(name)])
    x = rng.integers(0, 50, (total, npair, ndm, nprod)).astype(np.float32)
    for p in range(npair):
        for d in range(ndm):
            for _ in range(2):
                w = 1 << int(rng.integers(0, nwidth))
                n1 = int(rng.integers(nstat + w, total))
                x[n1 - w + 1:n1 + 1, p, d, 0] += float(rng.integers(40, 201))
    sizes = FIXED_SIZES if nstat == 16 else _sizes(rng, total, 30, (1, 7, 30))
    assert sum(sizes) == total >= 3 * nstat + (1 << (nwidth - 1)) and {1, 7, 30} <= set(sizes)
    z32, z64 = series(x, np.float32), series(x, np.float64)
    return x, sizes, pulse_search(z32, nstat, nwidth, np.float32, sizes), pulse_search(z64, nstat, nwidth, np.float64, sizes)


def float_case(rng, nwindows, npair, ndm, nprod):
    """chi^2 powers summed over 3072 channels (4 degrees of freedom each: mean / sigma = 78) times a gain in [0.5, 1.5] per
    series; with nprod = 4, XX and YY take half each and the cross terms are noise."""
    gain = rng.uniform(0.5, 1.5, (npair, ndm))
    if nprod == 1:
        return (rng.chisquare(4 * 3072, (nwindows, npair, ndm)) * gain).astype(np.float32)[..., None]
    x = rng.standard_normal((nwindows, npair, ndm, 4)) * 100
    x[..., 0] = rng.chisquare(2 * 3072, (nwindows, npair, ndm)) * gain
    x[..., 1] = rng.chisquare(2 * 3072, (nwindows, npair, ndm)) * gain
    return x.astype(np.float32)
