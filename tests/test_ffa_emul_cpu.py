"""The fast-folding kernels without a GPU: the kernels' own source (csrc/ffa_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/ffa_emul/) and run as 256 host threads per work-group, barriers and shuffles included, in the order
ffa.hip launches them.  The driver is a program of its own, built with -fsanitize=address,undefined, and every buffer has its exact
size: a word read or written outside one ends the run.  What this can show is the kernels' logic -- the downsample chain across
calls that cut a group, the pyramid, the fold stages between the two LDS buffers, the boxcar tree, the tie rules, the invalid
series -- not the GPU's arithmetic: the time buffer exactly, the statistics at the GPU test's bar, and the records bit for bit
against the float32 restatement (tests/ffa_ref.py) from the emulation's own {c, m, g}."""
import os
import subprocess

import numpy as np
import pytest

from tests import ffa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "ffa_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "ffa_kernels.h")
LDS_LINE = "extern __shared__ float fa_lds[];"
G_TOL, M_TOL = 9.7e-7, 6.1e-7       # the bars of tests/test_ffa_gpu.py


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("ffa_emul")
    src = open(KERNELS).read()
    assert src.count(LDS_LINE) == 1
    with open(os.path.join(d, "ffa_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* fa_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # (the runtime inside the program: it starts whatever else the loader brings first)
                           "-Wno-unknown-pragmas", "-I", str(d), "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, x, calls, nds, nt, noct, pmin, pmax, nwidth):
    """x [nwindows][nser][nprod]; (stats [nser][noct][4], records [nser][noct][nwidth], tbuf [nser][nt])."""
    exe, d = driver
    nser, nprod = x.shape[1], x.shape[2]
    assert sum(calls) == x.shape[0]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([nser, nprod, nds, nt, noct, pmin, pmax, nwidth, len(calls)] + list(calls), np.int32).tobytes())
        f.write(np.ascontiguousarray(x, np.float32).tobytes())
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), np.uint8)
    a, b = nser * noct * 16, nser * noct * nwidth * 16
    return (raw[:a].view(np.float32).reshape(nser, noct, 4), raw[a:a + b].view(ffa_ref.RECORD).reshape(nser, noct, nwidth),
            raw[a + b:].view(np.float32).reshape(nser, nt))


def case(seed, nwindows, nds, nprod):
    """Four series: chi^2 powers with mean / sigma = 55, a dead one, one with a NaN, and an integer-valued one: a constant with two
    equal pulses per 20 samples, so that equal maxima abound."""
    rng = np.random.default_rng(seed)
    z = (rng.chisquare(2 * 55 ** 2, (nwindows, 4)) * rng.uniform(0.5, 1.5, 4)).astype(np.float32)
    z[:, 1] = 0
    z[nwindows // 3, 2] = np.nan
    k = np.arange(nwindows) // nds
    z[:, 3] = 10 + 64 * ((k % 20 == 3) | (k % 20 == 8))
    if nprod == 1:
        return z[:, :, None]
    x = rng.standard_normal((nwindows, 4, 4)).astype(np.float32)
    x[..., 0] = np.floor(z / 2)
    x[..., 1] = z - x[..., 0]
    x[:, 2] = np.where(np.isnan(z[:, 2:3]), np.nan, x[:, 2])
    return x


def check(stats, rec, tbuf, x, nds, nt, noct, pmin, pmax, nwidth, tail=0):
    u0 = ffa_ref.downsample(ffa_ref.series(x)[:nt * nds], nds)
    ok = [0, 3]
    # (a call's windows past the segment have overwritten the first `tail` samples of the time buffer)
    assert tbuf[[0, 1, 3], tail:].tobytes() == np.ascontiguousarray(u0.T[[0, 1, 3], tail:]).tobytes()
    for o, u in enumerate(ffa_ref.pyramid(u0, noct)):
        c, m, v, g = ffa_ref.stats64(u[:, ok])
        assert (stats[ok, o, 0] == c).all()
        assert (np.abs(stats[ok, o, 1] - m) * g <= M_TOL).all() and (np.abs(stats[ok, o, 3] / g - 1) <= G_TOL).all()
    exp, _ = ffa_ref.records(u0, noct, pmin, pmax, nwidth, stats)
    assert rec.tobytes() == exp.tobytes(), np.argwhere(rec != exp)[:5]
    none = np.array([(0.0, -1, -1, -1)] * nwidth, ffa_ref.RECORD).tobytes()
    for s in (1, 2):
        for o in range(noct):
            assert rec[s, o].tobytes() == none
    assert (rec['p'][ok] >= pmin).all() and (rec['p'][ok] <= pmax).all() and (rec['snr'][ok] > 0).all()
    return exp


def test_smallest_segment_three_octaves(driver):
    """NT = 256, 3 octaves, p = 16..32: M * p = N_o exactly at 16 and 32, M = 2 at the top octave, odd p, nwidth = 4 = pmin / 2.  The
    integer series' two equal pulses per 20 samples tie within a profile (the smaller j wins) and between
    p = 19, i = 7 and p = 20, i = 0 (the smaller p wins)."""
    nt, noct, pmin, pmax, nwidth = 256, 3, 16, 32, 4
    x = case(1, nt + 5, 1, 1)
    stats, rec, tbuf = run(driver, x, [100, 100, 61], 1, nt, noct, pmin, pmax, nwidth)
    exp = check(stats, rec, tbuf, x, 1, nt, noct, pmin, pmax, nwidth, tail=5)
    snr, p, i, j = exp[3, 0, 0]
    xs = ((ffa_ref.series(x)[:nt, 3] - stats[3, 0, 0]) - stats[3, 0, 1])[None]
    prof = ffa_ref.fold(xs, int(p))[0]
    top = np.argwhere(prof == prof.max())
    assert len(top) >= 2 and tuple(top[0]) == (i, j) and j == 3, (exp[3, 0, 0], top)      # equal maxima at j = 3 and j = 8: the smaller j
    assert p == 19 and ffa_ref.fold(xs, 20)[0].max() == prof.max()          # 19 + 7/7 = 20 + 0/7 samples, 8 rows each: the smaller p
    assert ffa_ref.ffa_rows(nt >> 2, 32) == 2 and ffa_ref.ffa_rows(nt, 16) * 16 == nt


def test_downsampled_segment_that_is_no_power_of_two(driver):
    """NT = 768, nds = 3, nprod = 4, calls that cut downsample groups (1, 4, 100, 7 ... windows) and a tail past the segment."""
    nt, nds, noct, pmin, pmax, nwidth = 768, 3, 2, 17, 24, 3
    x = case(2, nt * nds + 4, nds, 4)
    calls = [1, 4, 100, 7, 1000, 2, 2, 1, 500]
    calls.append(x.shape[0] - sum(calls))
    stats, rec, tbuf = run(driver, x, calls, nds, nt, noct, pmin, pmax, nwidth)
    # (the tail of the last call has overwritten the first samples of the time buffer: compare what the records saw instead)
    u0 = ffa_ref.downsample(ffa_ref.series(x)[:nt * nds], nds)
    assert tbuf[[0, 1, 3], 2:].tobytes() == np.ascontiguousarray(u0.T[[0, 1, 3], 2:]).tobytes()
    exp, _ = ffa_ref.records(u0, noct, pmin, pmax, nwidth, stats)
    assert rec.tobytes() == exp.tobytes()
    assert (rec['p'][[1, 2]] == -1).all() and (rec['snr'][[1, 2]] == 0).all() and (rec['p'][[0, 3]] >= pmin).all()


@pytest.mark.parametrize("pmin,pmax", [(300, 303), (8192, 8192)])
def test_largest_segment(driver, pmin, pmax):
    """NT = 2^14, one octave, 8 widths: p = 300..303 (M = 32) and p = 8192 = NT / 2 (M = 2, all of the
    segment: 128 KiB between the two LDS buffers)."""
    nt, nwidth = 1 << 14, 8
    x = case(3, nt, 1, 1)
    stats, rec, tbuf = run(driver, x, [nt], 1, nt, 1, pmin, pmax, nwidth)
    check(stats, rec, tbuf, x, 1, nt, 1, pmin, pmax, nwidth)
