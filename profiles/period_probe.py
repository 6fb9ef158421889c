"""BeamPeriodSearch (xengPeriodRun) at the live size: 16 pairs x 256 and x 1024 DM trials, segments of NT = 2^14 windows, nprod = 1,
stacks of 2, 5 harmonic levels, whitening blocks of 64 bins.  Every point streams WARM warm-up segments and then REPS segments,
each as NT / NWIN calls of NWIN = 1024 windows over the same span of noise, ending in a synchronise; one JSON line per point with
the host view and the bytes a segment moves (the input once, the time buffer written and read, A read and written).

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/period_probe.py

(a run of its own: no counters in it) then `python3 profiles/period_probe.py --summarize OUT`: the median device time of the timed
launches of period_ingest_kernel and period_spectrum_kernel at each point, from the kernel trace (the points run one after
another, so the launches split by count; every second spectrum launch completes a stack and forms the harmonic sums)."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NT, NWIN, NSTACK, NLEVEL, NWHITE, KMIN = 16, 1 << 14, 1024, 2, 5, 64, 2
WARM, REPS = 2, 6                                                       # segments
POINTS = [256, 1024]                                                    # ndm, in launch order


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi

    rng = np.random.default_rng(0)
    done = ctypes.c_int()
    for ndm in POINTS:
        x = rng.chisquare(4 * 3072, NWIN * NPAIR * ndm).astype(np.float32)
        din = ffi.DeviceBuffer(x.nbytes).upload(x)
        dout = ffi.DeviceBuffer(NPAIR * ndm * NLEVEL * 8)
        ffi.call("xengPeriodInitialize", 0, NPAIR, ndm, NWIN, 1, NT, NSTACK, NLEVEL, NWHITE, KMIN)

        def segments(n):
            for _ in range(n * (NT // NWIN)):
                ffi.call("xengPeriodRun", din.ptr, NWIN, dout.ptr, ctypes.byref(done))
            ffi.call("xengPeriodSync")

        segments(WARM)
        t0 = time.perf_counter()
        segments(REPS)
        dt = (time.perf_counter() - t0) / REPS
        nser = NPAIR * ndm
        moved = nser * NT * 4 * 3 + nser * (NT // 2) * 4 * 2
        print(json.dumps({"what": "xengPeriodRun, one segment of NT windows in calls of NWIN (host view, ends in a synchronise)", "ms_per_segment": dt * 1e3,
                          "segments": WARM + REPS, "npair": NPAIR, "ndm": ndm, "nt": NT, "nwin": NWIN, "nstack": NSTACK, "nlevel": NLEVEL,
                          "nwhite": NWHITE, "work_groups": nser, "bytes_per_segment": moved}), flush=True)
        ffi.call("xengPeriodDestroy")
        din.free()
        dout.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel, per_seg in (("period_ingest_kernel", NT // NWIN), ("period_spectrum_kernel", 1)):
        per = (WARM + REPS) * per_seg
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        assert len(t) == per * len(POINTS), "%d %s launches in the trace, %d expected" % (len(t), kernel, per * len(POINTS))
        for k, ndm in enumerate(POINTS):
            u = t[k * per + WARM * per_seg:(k + 1) * per]
            groups = {"all": u} if per_seg > 1 else {"stack in progress": u[0::2], "stack complete (harmonic sums)": u[1::2]}
            for which, v in groups.items():
                print(json.dumps({"kernel": kernel, "ndm": ndm, "launches": which, "median_us": float(np.median(v)) / 1e3, "min_us": min(v) / 1e3,
                                  "max_us": max(v) / 1e3, "n": len(v)}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
