"""BeamPulseSearch (xengPulseRun) at the live size: 16 pairs x 256 and x 1024 DM trials, 30 windows per call, nprod = 1, 8 boxcar
widths, baseline blocks of 256 windows.  Every point streams WARM warm-up calls and then REPS calls back to back over the same
span of noise (the state advances: block boundaries fall inside the timed calls as they do live), ending in a synchronise; one
JSON line per point with the host view and the bytes a call moves (input once, the state and the y ring, the records).

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/pulse_probe.py

(a run of its own: no counters in it) then `python3 profiles/pulse_probe.py --summarize OUT`: the median device time of the timed
launches of pulse_search_kernel at each point, from the kernel trace (the points run one after another, so the launches split by
count)."""
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NWIN, NWIDTH, NSTAT = 16, 30, 8, 256
WARM, REPS = 10, 100
POINTS = [256, 1024]                                                    # ndm, in launch order


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi

    rng = np.random.default_rng(0)
    for ndm in POINTS:
        x = rng.chisquare(4 * 3072, NWIN * NPAIR * ndm).astype(np.float32)
        din = ffi.DeviceBuffer(x.nbytes).upload(x)
        dout = ffi.DeviceBuffer(NPAIR * ndm * 16)
        ffi.call("xengPulseInitialize", 0, NPAIR, ndm, NWIN, 1, NWIDTH, NSTAT)
        for _ in range(WARM):
            ffi.call("xengPulseRun", din.ptr, NWIN, dout.ptr)
        ffi.call("xengPulseSync")
        t0 = time.perf_counter()
        for _ in range(REPS):
            ffi.call("xengPulseRun", din.ptr, NWIN, dout.ptr)
        ffi.call("xengPulseSync")
        dt = (time.perf_counter() - t0) / REPS
        tail = (1 << (NWIDTH - 1)) - 1
        moved = x.nbytes + NPAIR * ndm * 4 * (2 * 7 + tail + min(tail, NWIN)) + dout.nbytes
        print(json.dumps({"what": "xengPulseRun back to back (host view, ends in a synchronise)", "us_per_call": dt * 1e6, "launches": WARM + REPS,
                          "npair": NPAIR, "ndm": ndm, "nwin": NWIN, "nwidth": NWIDTH, "nstat": NSTAT, "work_groups": NPAIR * ndm // 64,
                          "bytes_per_call": moved}), flush=True)
        ffi.call("xengPulseDestroy")
        din.free()
        dout.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + REPS
    t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "pulse_search_kernel" in r["Kernel_Name"]]
    assert len(t) == per * len(POINTS), "%d pulse_search_kernel launches in the trace, %d expected" % (len(t), per * len(POINTS))
    for k, ndm in enumerate(POINTS):
        u = t[k * per + WARM:(k + 1) * per]
        print(json.dumps({"kernel": "pulse_search_kernel", "ndm": ndm, "median_us": float(np.median(u)) / 1e3, "min_us": min(u) / 1e3,
                          "max_us": max(u) / 1e3, "launches": len(u)}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
