"""BeamPeriodSearchLong (xengPlongRun) at the live size: 16 pairs x 256 DM trials = 4096 series, segments of NT = 2^20 windows,
nprod = 1, stacks of one segment, 5 levels, 32 log-spaced bands, B = 64: 24 GiB of time buffer and stack plus 2 GiB of scratch.
WARM warm-up segments and then REPS segments are streamed, each as NT / NWIN calls of NWIN = 1024 windows over the same span of
noise, ending in a synchronise; one JSON line with the host view and the HBM bytes a segment moves, counted.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/plong_probe.py

(a run of its own: no counters in it) then `python3 profiles/plong_probe.py --summarize OUT`: the device time of the timed
launches of each kernel from the kernel trace, summed per segment (the per-batch kernels run once per batch of SB series)."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NDM, NT, NWIN, NSTACK, NLEVEL, NWHITE, NBAND = 16, 256, 1 << 20, 1024, 1, 5, 64, 32
WARM, REPS = 1, 2                                                       # segments
KERNELS = ("plong_ingest_kernel", "plong_mean_kernel", "plong_cols_kernel", "plong_rows_kernel", "plong_power_kernel", "plong_whiten_kernel",
           "plong_sums_kernel", "plong_reduce_kernel")


def hbm_bytes():
    """HBM bytes per series and segment behind the ingest, counted: the mean reads the segment (4 NT); the columns and the rows
    each read and write the packed transform (8 NT each); the untangle reads every bin and its partner (8 NT) and writes P (2 NT);
    the whitening reads P twice (4 NT) and stores A (2 NT; reads it as well in a stack's later segments)."""
    return (4 + 8 + 8 + 8 + 2 + 4 + 2) * NT


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.blocks import period_bands

    rng = np.random.default_rng(0)
    done, sb, sbmax = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    nser = NPAIR * NDM
    x = rng.chisquare(4 * 3072, NWIN * nser).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    dout = ffi.DeviceBuffer(nser * NLEVEL * NBAND * 8)
    kedge = period_bands(NT, NBAND, 2)
    ffi.call("xengPlongInitialize", 0, NPAIR, NDM, NWIN, 1, NT, NSTACK, NLEVEL, NWHITE, NBAND, (ctypes.c_int * len(kedge))(*kedge))
    ffi.call("xengPlongGetBatch", ctypes.byref(sb), ctypes.byref(sbmax))

    def segments(n):
        for _ in range(n * (NT // NWIN)):
            ffi.call("xengPlongRun", din.ptr, NWIN, dout.ptr, ctypes.byref(done))
        ffi.call("xengPlongSync")

    segments(WARM)
    t0 = time.perf_counter()
    segments(REPS)
    dt = (time.perf_counter() - t0) / REPS
    print(json.dumps({"what": "xengPlongRun, one segment of NT windows in calls of NWIN windows (host view, ends in a synchronise)", "ms_per_segment": dt * 1e3,
                      "segments": WARM + REPS, "npair": NPAIR, "ndm": NDM, "nt": NT, "nwin": NWIN, "nstack": NSTACK, "nlevel": NLEVEL, "nwhite": NWHITE,
                      "nband": NBAND, "series_per_batch": sb.value, "hbm_bytes_per_segment": hbm_bytes() * nser}), flush=True)
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
    total = 0.0
    for kernel in KERNELS:
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        assert t and len(t) % (WARM + REPS) == 0, "%d %s launches in the trace" % (len(t), kernel)
        per_seg = len(t) // (WARM + REPS)
        u = t[WARM * per_seg:]
        print(json.dumps({"kernel": kernel, "launches_per_segment": per_seg, "device_ms_per_segment": sum(u) / REPS / 1e6, "median_us": float(np.median(u)) / 1e3}))
        total += sum(u) / REPS
    print(json.dumps({"device_ms_per_segment": total / 1e6, "hbm_bytes_per_segment": hbm_bytes() * NPAIR * NDM,
                      "hbm_TB_per_s": hbm_bytes() * NPAIR * NDM / (total * 1e-9) / 1e12}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
