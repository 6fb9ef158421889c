"""The dedisperser's kernels without a GPU: the kernels' own source (csrc/dedisp_kernels.h, unchanged) compiled as host C++ against a
stand-in for <hip/hip_runtime.h> (tests/dedisp_emul/) and run as 256 host threads per work-group in the order, with the grids and
with the arguments dedisp.hip launches them.  The driver is a program of its own and every buffer has its exact size: a word read
or written outside one -- a slot past the ring (dd_slot), a window past the call or a trial past the table in a clamped idle lane
(tc, dc), a channel past the pair in the ragged ingest tile -- ends the run of the address-sanitizer build, and a word two threads
of a work-group touch with no barrier between them (the ingest tile, the partial sums that meet in LDS) is a report of the
thread-sanitizer build.  The thread sanitizer sees races inside a work-group between barriers; it cannot see races between the
work-groups of one launch, which run one after another here.  The history ring starts as NaN, so a window used from before
window 0 -- after Initialize or after a Reset, which clears nothing -- reaches the output.  After every call the driver compares the
output word for word with what this side wrote from the ordered float32 restatement (tests/dedisp_ref.dedisperse_ordered32) and
ends with status 4 unless they are equal: on the host, with -ffp-contract=off and libm's fmaf, the contract's order is bit for bit
on float data.  What this shows is the kernels' logic, bounds and barriers, not the GPU's arithmetic (tests/test_dedisp_gpu.py).
Nothing is loaded into Python under a sanitizer.

The cases (tests/dedisp_cases.py), each under both builds and both nprod:
  (a) nfine 70: three ingest tiles, the last ragged (6 channels); Q = 18, the last segment has 16.  Calls of 1 to 5 windows: time
      tiles of 1, 2, 4, 8 windows with idle lanes along time and along the 5 trials.  S 11, L = 16: 55 windows wrap the ring three
      times, and calls straddle the wrap.  An eighth of the weights is 0 and those channels hold NaN.
  (b) nfine 3, fewer channels than segments (Q = 1, segment 3 empty), one trial, S 2.
  (c) nwin 70, calls 70, 33, 64, 65: TT = 64, two time tiles with 6 and 1 live windows in the second, 31 idle lanes at 33
      windows, an ingest grid of z = 3.
  (d) S = 0: L = nwin, no history at all.
  (e) case (a) with a SetWeights before call 4 (old windows take the new weights) and a Reset before call 7 (what the ring holds
      lies before window 0 and is left out)."""
import os

import numpy as np
import pytest

from tests import dedisp_cases, emul_build
from tests.dedisp_ref import dedisperse_ordered32

EMUL = os.path.join(emul_build.ROOT, "tests", "dedisp_emul")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("dedisp_emul")
    return emul_build.build_both(d, EMUL, [emul_build.CSRC]), str(d)


def run(drivers, case, nprod, events=()):
    """events: [(the call before which it is given, new weights or None for a Reset)].  Writes the input and, from the
    restatement, the expectation; both drivers compare."""
    exes, d = drivers
    c = dedisp_cases.CASES[case]
    x, s, w = dedisp_cases.float_case(case, nprod)
    calls = c["calls"]
    events = [(0, w)] + list(events)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([c["npair"], c["nfine"], c["nwin"], c["ndm"], c["S"], nprod, len(calls), len(events)], np.int32).tobytes())
        f.write(np.asarray(calls, np.int32).tobytes() + s.tobytes())
        for at, wn in events:
            f.write(np.array([at, int(wn is None)], np.int32).tobytes() + (np.zeros_like(w) if wn is None else np.asarray(wn, np.float32)).tobytes())
        f.write(x.tobytes())
    first, n, outs = 0, 0, []
    with open(os.path.join(d, "exp.bin"), "wb") as f:
        for ic, nc in enumerate(calls):
            for at, wn in events:
                if at == ic:
                    if wn is None:
                        first = n
                    else:
                        w = np.asarray(wn, np.float32)
            n += nc
            outs.append(dedisperse_ordered32(x[first:n], s, w, nprod)[-nc:])
            f.write(outs[-1].tobytes())
    for name in sorted(exes):
        assert int(emul_build.run(exes[name], os.path.join(d, "in.bin"), os.path.join(d, "exp.bin"))) == len(calls)
    return np.concatenate(outs)


@pytest.mark.parametrize("nprod", [1, 4])
@pytest.mark.parametrize("case", sorted(dedisp_cases.CASES))
def test_kernels_on_host_threads_equal_the_ordered_restatement(drivers, case, nprod):
    """Cases (a) to (d): no sanitizer report from either build, every word of every call equal, and every output finite although
    the ring started as NaN and the zero-weight channels hold NaN."""
    assert np.isfinite(run(drivers, case, nprod)).all()


@pytest.mark.parametrize("nprod", [1, 4])
def test_set_weights_and_reset_between_calls(drivers, nprod):
    """Case (e): new weights before call 4 hold for the windows already in the ring; after the Reset before call 7 the first
    outputs are partial sums again, with the ring still full of the windows from before."""
    x, s, w = dedisp_cases.float_case("a", nprod)
    w2 = w * np.linspace(0.75, 1.25, w.size).astype(np.float32)       # (the zeros stay where the NaN are)
    plain = dedisperse_ordered32(x, s, w, nprod)
    out = run(drivers, "a", nprod, [(4, w2), (7, None)])
    calls = dedisp_cases.CASES["a"]["calls"]
    n4, n7 = sum(calls[:4]), sum(calls[:7])
    assert np.isfinite(out).all() and np.array_equal(out[:n4], plain[:n4]) and not np.array_equal(out[n4:n7], plain[n4:n7])
    assert (out[n7, ..., 0] < out[n7 - 1, ..., 0]).all()          # (window 0 after the Reset: only the channels of back-delay 0; XX, I > 0)
