"""The single-pulse search kernel without a GPU: the kernel's own source (csrc/pulse_kernels.h) compiled as host C++ against a stand-in
for <hip/hip_runtime.h> (tests/pulse_emul/) and run as 256 host threads per work-group with the grid, the LDS bytes and the
arguments pulse.hip launches it with.  The driver is a program of its own and every buffer has its exact size: a word read or
written outside one -- a slot past the y ring (ps_slot), a series past the plane in a clamped idle lane (sc), a window past the
call, an LDS word past the launch's max(T + 2 nc, 16) rows (the red[3][64] overlay of the last reduction when T + 2 nc < 16) --
ends the run of the address-sanitizer build; and a word two threads of a work-group touch with no barrier between them -- "it
reads r - w before anybody writes it, so a level needs one barrier", the rows wave 0 and waves 1-3 fill, the overlay over Y -- is
a report of the thread-sanitizer build.  The thread sanitizer sees races inside a work-group between barriers; it cannot see races
between the work-groups of one launch, which run one after another here.  The dynamic LDS is NaN before every work-group; the
state and the y ring start as NaN and a Reset clears nothing, so a value used from before window 0 shows.  After every call the
driver compares the records, and after a call that completes a block the seven state rows (c, m, v, g, and c, a, q of the running
block), with what this side wrote from the float32 restatement (tests/pulse_ref.py) and ends with a status of 5 or more unless
they are equal: on the host, with -ffp-contract=off and libm's fmaf and sqrtf, every step of the contract is bit for bit on float
data, g and snr included.  What this shows is the kernel's logic, bounds and barriers, not the GPU's arithmetic
(tests/test_pulse_gpu.py).  Nothing is loaded into Python under a sanitizer.

Every case has 3 x 37 = 111 series (two work-groups, the second with 47 live lanes), nwin 30, calls of 1, 7 and 30 windows, and runs
under both builds and both nprod.  A run is a prefix of calls reaching into block 1, a Reset, and the whole sequence again on
other data.  After the Reset series 3 is constant (v = 0: never valid), series 40 has a NaN window and series 70 a +Inf window in
block 1 (block 2 then has no y, block 3 recovers), among clean neighbours.
  (nwidth, nstat) = (1, 2): T = 0; calls of 1 and 7 windows take the 16-row LDS floor, where the red overlay is longer than Y and
                    G; every call of 7 or 30 completes several blocks.
  (4, 16):          FIXED_SIZES of tests/pulse_cases.py: block boundaries on the first, an inner and the last window of a call.
  (5, 24):          nstat not a power of two: m and v round; boundaries on the first, an inner and the last window of a call.
  (8, 128):         T = 127 is longer than any call: the ring's tail is read across four or more calls and wraps.
And one integer case of INT_CASES (exact ties between windows and between widths: the tie rule is walked)."""
import os

import numpy as np
import pytest

from tests import emul_build, pulse_cases
from tests.pulse_ref import block_chain, pulse_search, series

EMUL = os.path.join(emul_build.ROOT, "tests", "pulse_emul")
LDS_LINE = "extern __shared__ float ps_lds[];"
NPAIR, NDM, NWIN = 3, 37, 30
RECORD = np.dtype([('snr', '<f4'), ('n', '<i4'), ('iw', '<i4'), ('B', '<f4')])       # the record of include/xeng.h


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("pulse_emul")
    src = open(os.path.join(emul_build.CSRC, "pulse_kernels.h")).read()
    assert src.count(LDS_LINE) == 1
    with open(os.path.join(d, "pulse_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "float* ps_lds = g_lds;"))
    return emul_build.build_both(d, EMUL, [d]), str(d)


def split(n):
    """n windows as calls of 30, 7 and 1."""
    out = []
    for c in (30, 7, 1):
        out += [c] * (n // c)
        n %= c
    return out


def sizes_for(nstat, total):
    """Calls of 1, 7 and 30: block 0 in whole calls (a call ends on a block's last window and the next begins on a block's
    first), a call of 7 with a block's first window inside, a call of 30 whose last window is a block's first."""
    if nstat <= 16:
        assert total == sum(pulse_cases.FIXED_SIZES)
        return list(pulse_cases.FIXED_SIZES)
    s = split(nstat) + split(nstat - 3) + [7]
    k = -(-(sum(s) + 29) // nstat)
    s += split(k * nstat - 29 - sum(s)) + [30]
    s += split(total - sum(s))
    ends = np.cumsum(s)
    starts = ends - np.array(s)
    assert ends[-1] == total and {1, 7, 30} <= set(s)
    assert any(a % nstat == 0 for a in starts) and any((e - 1) % nstat == 0 for e in ends) and any((e - 1) % nstat == nstat - 1 for e in ends)
    assert any(a < j * nstat < e - 1 for a, e in zip(starts, ends) for j in range(1, 8))
    return s


def expectation(x, sizes, nstat, nwidth):
    """The bytes the driver must see for a run of `sizes` from a reset, from the float32 restatement."""
    z = series(x, np.float32).reshape(x.shape[0], -1)
    r = pulse_search(z, nstat, nwidth, np.float32, sizes)
    out, a = [], 0
    for k, nc in enumerate(sizes):
        rec = r['records'][k]
        plane = np.zeros(z.shape[1], RECORD)
        plane['snr'], plane['n'], plane['iw'], plane['B'] = rec['snr'], rec['n'], rec['iw'], rec['B']
        out.append(plane.tobytes())
        if a % nstat + nc >= nstat:
            a += nc
            blk = a // nstat - 1
            first = blk * nstat if a % nstat == 0 else (blk + 1) * nstat          # the running block: the one just completed, or the next
            rc, ra, rq = block_chain(z[None, first:a], np.float32)
            out.append(np.stack([r['c'][blk], r['m'][blk], r['v'][blk], r['g'][blk], rc[0], ra[0], rq[0]]).astype(np.float32).tobytes())
        else:
            a += nc
    return b"".join(out), r


def run(drivers, parts, nprod, nwidth, nstat):
    """parts: [(x [windows][NPAIR][NDM][nprod], sizes)], a Reset between two parts.  Returns the restatement's results per part and
    the number of calls that completed a block."""
    exes, d = drivers
    calls = [nc for _, sizes in parts for nc in sizes]
    resets = np.cumsum([len(sizes) for _, sizes in parts])[:-1]
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([NPAIR * NDM, NWIN, nprod, nwidth, nstat, len(calls), len(resets)], np.int32).tobytes())
        f.write(np.asarray(calls, np.int32).tobytes() + np.asarray(resets, np.int32).tobytes())
        for x, _ in parts:
            assert x.shape[1:] == (NPAIR, NDM, nprod)
            f.write(np.ascontiguousarray(x, np.float32).tobytes())
    exp = [expectation(x, sizes, nstat, nwidth) for x, sizes in parts]
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        f.write(b"".join(e[0] for e in exp))
    ndone = sum(int(a % nstat + nc >= nstat) for _, sizes in parts for a, nc in zip(np.cumsum(sizes) - np.array(sizes), sizes))
    for name in sorted(exes):
        assert int(emul_build.run(exes[name], os.path.join(d, "in.bin"), os.path.join(d, "exp.bin"))) == ndone
    return [e[1] for e in exp]


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("nwidth,nstat", [(1, 2), (4, 16), (5, 24), (8, 128)])
def test_float_data_a_reset_and_series_without_a_baseline(drivers, nwidth, nstat, nprod):
    total = {2: 110, 16: 110, 24: 4 * 24 + 17, 128: 4 * 128 + 17}[nstat]
    sizes = sizes_for(nstat, total)
    prefix = sizes[:int(np.searchsorted(np.cumsum(sizes), nstat + 9)) + 1]         # (into block 1: the state and the ring are in use)
    rng = np.random.default_rng(100 * nstat + nprod)
    x0 = pulse_cases.float_case(rng, sum(prefix), NPAIR, NDM, nprod)
    x = pulse_cases.float_case(rng, total, NPAIR, NDM, nprod)
    at = nstat + nstat // 2
    x[:, 0, 3, :2] = 777.0
    x[at, 1, 3, 0] = np.nan                 # series 40
    x[at, 1, 33, 0] = np.inf                # series 70
    r0, r = run(drivers, [(x0, prefix), (x, sizes)], nprod, nwidth, nstat)
    valid = r['valid'].reshape(r['valid'].shape[0], -1)
    assert not valid[:, 3].any() and not valid[1, 40] and not valid[1, 70] and valid[0].sum() == valid[1].sum() + 2 == NPAIR * NDM - 1
    assert valid[2:, 40].all() and valid[2:, 70].all()
    scored = r['scored'].reshape(total, nwidth, -1)
    assert not scored[:, :, 3].any() and not scored[2 * nstat:3 * nstat, :, [40, 70]].any() and scored[3 * nstat:, 0].all(axis=0)[[40, 70]].all()
    assert scored[nstat:, 0, 5].all() and not scored[:nstat].any() and r0['scored'][nstat:, 0].all()
    assert np.isposinf(r['snr'].reshape(total, nwidth, -1)[at, 0, 70])


def test_integer_data_walk_the_tie_rule(drivers):
    """"111 series, I, 4 widths" of INT_CASES: equal scores at two windows and at two widths are common there, and the smallest
    n, then the smallest iw, wins."""
    name = "111 series, I, 4 widths"
    npair, ndm, nprod, nwidth, nstat, total, _ = pulse_cases.INT_CASES[name]
    assert (npair, ndm) == (NPAIR, NDM)
    x, sizes, r32, _ = pulse_cases.integer_case(name)
    r, = run(drivers, [(x, sizes)], nprod, nwidth, nstat)
    snr = np.where(r['scored'], r['snr'], -np.inf).reshape(total, nwidth, -1)
    ties, a = 0, 0
    for nc in sizes:
        s = snr[a:a + nc].reshape(nc * nwidth, -1)
        ties += int(((s == s.max(axis=0)) & np.isfinite(s)).sum(axis=0).max() > 1)
        a += nc
    assert ties >= 1                    # (calls in which two candidates hold exactly the winning score)
    assert all(np.array_equal(p['n'], q['n'].reshape(-1)) and np.array_equal(p['iw'], q['iw'].reshape(-1)) for p, q in zip(r['records'], r32['records']))
