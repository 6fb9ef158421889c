"""BeamAccelSearch (xengAccelRun) beside its yardstick: 2 pairs x 256 DM trials = 512 series, segments of NT = 2^20 windows,
nprod = 1, 16 trial accelerations, 5 levels, 32 log-spaced bands, B = 64; then xengPlongRun (nstack = 1) at the same series
count in the same process.  For each engine WARM warm-up segments and then REPS segments are streamed, each as NT / NWIN calls of
NWIN = 1024 windows over the same span of noise, ending in a synchronise; one JSON line per engine with the host view.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/accel_probe.py

(a run of its own: no counters in it) then `python3 profiles/accel_probe.py --summarize OUT`: the device time of the timed
launches of each kernel from the kernel trace, summed per segment, for both engines (the acceleration search's copies of the
plong kernels carry the namespace accel_plong in their names), the cost of a trial against a plong segment without its ingest,
the gathered mean and columns pass against plong's, and the share of the sums."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NDM, NT, NWIN, NTRIAL, NLEVEL, NWHITE, NBAND = 2, 256, 1 << 20, 1024, 16, 5, 64, 32
WARM, REPS = 1, 2                                                       # segments, per engine
ACCEL = ("plong_ingest_kernel", "accel_mean_kernel", "accel_cols_kernel", "plong_rows_kernel", "plong_power_kernel", "plong_whiten_kernel", "plong_sums_kernel",
         "plong_reduce_kernel", "accel_best_kernel")
PLONG = ("plong_ingest_kernel", "plong_mean_kernel", "plong_cols_kernel", "plong_rows_kernel", "plong_power_kernel", "plong_whiten_kernel", "plong_sums_kernel",
         "plong_reduce_kernel")


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.blocks import period_bands

    rng = np.random.default_rng(0)
    done, sb, sbmax = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    nser = NPAIR * NDM
    x = rng.chisquare(4 * 3072, NWIN * nser).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    dout = ffi.DeviceBuffer(nser * NLEVEL * NBAND * 16)
    kedge = period_bands(NT, NBAND, 2)
    edges = (ctypes.c_int * len(kedge))(*kedge)
    # mid-segment shifts of -7.5 .. 7.5 thousand windows: ordinary trials, every one a gather
    alphas = [-4.0 * 1000.0 * (i - 7.5) / float(NT) ** 2 for i in range(NTRIAL)]
    sizes = {"npair": NPAIR, "ndm": NDM, "nt": NT, "nwin": NWIN, "nlevel": NLEVEL, "nwhite": NWHITE, "nband": NBAND}

    def segments(run, sync, n):
        for _ in range(n * (NT // NWIN)):
            ffi.call(run, din.ptr, NWIN, dout.ptr, ctypes.byref(done))
        ffi.call(sync)

    ffi.call("xengAccelInitialize", 0, NPAIR, NDM, NWIN, 1, NT, NLEVEL, NWHITE, NBAND, edges, NTRIAL, (ctypes.c_double * NTRIAL)(*alphas))
    ffi.call("xengAccelGetBatch", ctypes.byref(sb), ctypes.byref(sbmax))
    segments("xengAccelRun", "xengAccelSync", WARM)
    t0 = time.perf_counter()
    segments("xengAccelRun", "xengAccelSync", REPS)
    dt = (time.perf_counter() - t0) / REPS
    print(json.dumps(dict(sizes, what="xengAccelRun, one segment of NT windows in calls of NWIN windows (host view, ends in a synchronise)",
                          ms_per_segment=dt * 1e3, segments=WARM + REPS, ntrial=NTRIAL, series_per_batch=sb.value)), flush=True)
    ffi.call("xengAccelDestroy")

    ffi.call("xengPlongInitialize", 0, NPAIR, NDM, NWIN, 1, NT, 1, NLEVEL, NWHITE, NBAND, edges)
    ffi.call("xengPlongGetBatch", ctypes.byref(sb), ctypes.byref(sbmax))
    segments("xengPlongRun", "xengPlongSync", WARM)
    t0 = time.perf_counter()
    segments("xengPlongRun", "xengPlongSync", REPS)
    dt = (time.perf_counter() - t0) / REPS
    print(json.dumps(dict(sizes, what="xengPlongRun, the same series count, nstack = 1", ms_per_segment=dt * 1e3, segments=WARM + REPS,
                          series_per_batch=sb.value)), flush=True)
    ffi.call("xengPlongDestroy")
    din.free()
    dout.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    table = {}
    for engine, kernels in (("accel", ACCEL), ("plong", PLONG)):
        mine = [r for r in rows if ("accel_" in r["Kernel_Name"]) == (engine == "accel")]
        total = 0.0
        for kernel in kernels:
            t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine if kernel in r["Kernel_Name"]]
            assert t and len(t) % (WARM + REPS) == 0, "%d %s launches of %s in the trace" % (len(t), kernel, engine)
            per_seg = len(t) // (WARM + REPS)
            u = t[WARM * per_seg:]
            table[engine, kernel] = sum(u) / REPS / 1e6
            print(json.dumps({"engine": engine, "kernel": kernel, "launches_per_segment": per_seg, "device_ms_per_segment": table[engine, kernel],
                              "median_us": float(np.median(u)) / 1e3}))
            total += sum(u) / REPS / 1e6
        table[engine] = total
        print(json.dumps({"engine": engine, "device_ms_per_segment": total}))
    trial = (table["accel"] - table["accel", "plong_ingest_kernel"] - table["accel", "accel_best_kernel"]) / NTRIAL
    yard = table["plong"] - table["plong", "plong_ingest_kernel"]
    print(json.dumps({"ms_per_trial": trial, "plong_ms_per_segment_without_ingest": yard, "trial_over_plong_segment": trial / yard,
                      "gathered_mean_over_plong_mean": table["accel", "accel_mean_kernel"] / NTRIAL / table["plong", "plong_mean_kernel"],
                      "gathered_cols_over_plong_cols": table["accel", "accel_cols_kernel"] / NTRIAL / table["plong", "plong_cols_kernel"],
                      "sums_share_of_a_trial": table["accel", "plong_sums_kernel"] / NTRIAL / trial,
                      "sums_share_of_a_plong_segment": table["plong", "plong_sums_kernel"] / table["plong"]}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
