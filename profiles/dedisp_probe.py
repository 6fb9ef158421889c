"""BeamDedisperse (xengDedispRun) at the live size: 16 pairs x 3072 fine channels x 30 windows per call, nprod = 1, for 256 and
1024 DM trials, with a history that fits the Infinity Cache (S = 107: DM <= 30 at 30-frame windows, 137 windows x 196 KB = 27 MB)
and one far beyond it (S = 10000: 1-frame windows, 10030 windows = 1.97 GB).  The table is the cold-plasma curve over the 96
channels above 50 MHz scaled to S.  Every point is WARM warm-up calls and then REPS back to back, ending in a synchronise; one
JSON line per point with the host view, the HBM bound's bytes (input once, history written once, output) and the gathered bytes.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/dedisp_probe.py

then `python3 profiles/dedisp_probe.py --summarize OUT`: the median device time of the timed launches of dedisp_ingest_kernel and
dedisp_kernel at each point, from the kernel trace (the points run one after another, so the launches split by count)."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NCHAN, N, NWIN = 16, 96, 32, 30
NFINE = NCHAN * N
WARM, REPS = 5, 40
POINTS = [(256, 107), (1024, 107), (256, 10000), (1024, 10000)]         # (ndm, S), in launch order
HBM_BYTES_PER_S = 8e12                                                  # MI355X peak


def table(ndm, S):
    bw = 23925.78125
    f = (50e6 - bw / 2 + bw / N * np.arange(NFINE)) * 1e-6
    curve = (f ** -2 - f[-1] ** -2) / (f[0] ** -2 - f[-1] ** -2)
    return np.ascontiguousarray(np.rint(S * np.linspace(0, 1, ndm)[:, None] * curve[None, :]).astype(np.int32))


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi

    rng = np.random.default_rng(0)
    x = rng.chisquare(4, NWIN * NPAIR * NFINE * 4).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    for ndm, S in POINTS:
        ffi.call("xengDedispInitialize", 0, NPAIR, NFINE, NWIN, ndm, S, 1)
        s = table(ndm, S)
        ffi.call("xengDedispSetDelays", s.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        dout = ffi.DeviceBuffer(NWIN * NPAIR * ndm * 4)
        for _ in range(WARM):
            ffi.call("xengDedispRun", din.ptr, NWIN, dout.ptr)
        ffi.call("xengDedispSync")
        t0 = time.perf_counter()
        for _ in range(REPS):
            ffi.call("xengDedispRun", din.ptr, NWIN, dout.ptr)
        ffi.call("xengDedispSync")
        dt = (time.perf_counter() - t0) / REPS
        hbm = x.nbytes + NWIN * NPAIR * NFINE * 4 + dout.nbytes
        print(json.dumps({"what": "xengDedispRun back to back (host view, ends in a synchronise)", "us_per_call": dt * 1e6, "launches": WARM + REPS,
                          "ndm": ndm, "S": S, "npair": NPAIR, "nfine": NFINE, "nwin": NWIN, "history_MB": (S + NWIN) * NPAIR * NFINE * 4e-6,
                          "hbm_bound_bytes": hbm, "hbm_bound_us": hbm / HBM_BYTES_PER_S * 1e6, "gathered_bytes": NWIN * NPAIR * ndm * NFINE * 4,
                          "table_bytes": s.nbytes}), flush=True)
        ffi.call("xengDedispDestroy")
        dout.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + REPS
    for kernel in ("dedisp_ingest_kernel", "dedisp_kernel"):
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel + "<" in r["Kernel_Name"] or kernel + "I" in r["Kernel_Name"]]
        assert len(t) == per * len(POINTS), "%d %s launches in the trace, %d expected" % (len(t), kernel, per * len(POINTS))
        for k, (ndm, S) in enumerate(POINTS):
            u = t[k * per + WARM:(k + 1) * per]
            print(json.dumps({"kernel": kernel, "ndm": ndm, "S": S, "median_us": float(np.median(u)) / 1e3, "min_us": min(u) / 1e3, "max_us": max(u) / 1e3,
                              "launches": len(u)}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
