"""BeamFold (xengFoldRun, xengFoldDump) at the live size: 16 pairs x 3072 fine channels x 30 windows per call, 1024 bins, for
nprod = 1 and 4, with 16 different spin periods between 0.03 and 5 s at 40 ms windows (from several turns per window to 125
windows per turn: bins that change at every window and bins that stay).  Every point is WARM warm-up calls and then REPS back to
back, ending in a synchronise, then NDUMP dedispersed dumps (nfscr = nfine, normalised, not clearing) and NDUMP full cubes
(nfscr = 1); one JSON line per point with the host view and the HBM bound's bytes (input once; at most one read and one write of
a profile word per window and word).

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/fold_probe.py

then `python3 profiles/fold_probe.py --summarize OUT`: the median device time of the timed launches of fold_kernel and of
fold_dump_kernel at each point, from the kernel trace (the points run one after another, so the launches split by count)."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NCHAN, N, NWIN, NBIN = 16, 96, 32, 30, 1024
NFINE = NCHAN * N
WARM, REPS, NDUMP = 5, 40, 3
POINTS = [1, 4]                                                         # nprod, in launch order
HBM_BYTES_PER_S = 6.3e12                                                # MI355X, achievable


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi

    rng = np.random.default_rng(0)
    x = rng.chisquare(4, NWIN * NPAIR * NFINE * 4).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    periods = np.geomspace(0.03, 5.0, NPAIR) / 0.04                     # windows per turn
    phi0 = (rng.random(NPAIR) * 2.0 ** 64).astype(np.uint64)
    dphi = np.array([int(round(2 ** 64 / p)) % 2 ** 64 for p in periods], np.uint64)
    ddphi = np.zeros(NPAIR, np.int64)
    active = np.ones(NPAIR, np.uint8)
    rot = np.ascontiguousarray((np.arange(NFINE)[None, :] * (np.arange(NPAIR)[:, None] + 1) // 3) % NBIN, np.int32)
    for nprod in POINTS:
        ffi.call("xengFoldInitialize", 0, NPAIR, NFINE, NWIN, NBIN, nprod)
        ffi.call("xengFoldSetPhase", phi0.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), dphi.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                 ddphi.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), active.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), 0)
        ffi.call("xengFoldSetRotations", rot.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        dout = ffi.DeviceBuffer(NPAIR * nprod * NFINE * NBIN * 4)
        for _ in range(WARM):
            ffi.call("xengFoldRun", din.ptr, NWIN)
        ffi.call("xengFoldSync")
        t0 = time.perf_counter()
        for _ in range(REPS):
            ffi.call("xengFoldRun", din.ptr, NWIN)
        ffi.call("xengFoldSync")
        dt = (time.perf_counter() - t0) / REPS
        words = NWIN * NPAIR * NFINE * nprod
        hbm = x.nbytes + 2 * words * 4
        print(json.dumps({"what": "xengFoldRun back to back (host view, ends in a synchronise)", "us_per_call": dt * 1e6, "launches": WARM + REPS,
                          "nprod": nprod, "npair": NPAIR, "nfine": NFINE, "nwin": NWIN, "nbin": NBIN, "profile_MB": NPAIR * NBIN * NFINE * nprod * 4e-6,
                          "hbm_bound_bytes": hbm, "hbm_bound_us": hbm / HBM_BYTES_PER_S * 1e6}), flush=True)
        for nfscr in (NFINE, 1):
            t0 = time.perf_counter()
            for _ in range(NDUMP):
                ffi.call("xengFoldDump", dout.ptr, None, nfscr, 1, 0)
            ffi.call("xengFoldSync")
            dt = (time.perf_counter() - t0) / NDUMP
            prof = NPAIR * NBIN * NFINE * nprod * 4
            print(json.dumps({"what": "xengFoldDump (host view, ends in a synchronise)", "us_per_call": dt * 1e6, "nprod": nprod, "nfscr": nfscr,
                              "hbm_bound_bytes": prof, "hbm_bound_us": prof / HBM_BYTES_PER_S * 1e6}), flush=True)
        ffi.call("xengFoldDestroy")
        dout.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + REPS
    t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "fold_kernel" in r["Kernel_Name"]]
    assert len(t) == per * len(POINTS), "%d fold_kernel launches in the trace, %d expected" % (len(t), per * len(POINTS))
    for k, nprod in enumerate(POINTS):
        u = t[k * per + WARM:(k + 1) * per]
        print(json.dumps({"kernel": "fold_kernel<%d>" % nprod, "median_us": float(np.median(u)) / 1e3, "min_us": min(u) / 1e3, "max_us": max(u) / 1e3,
                          "launches": len(u)}))
    t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "fold_dump_kernel" in r["Kernel_Name"]]
    assert len(t) == 2 * NDUMP * len(POINTS), "%d fold_dump_kernel launches in the trace, %d expected" % (len(t), 2 * NDUMP * len(POINTS))
    for k, nprod in enumerate(POINTS):
        for j, nfscr in enumerate((NFINE, 1)):
            u = t[(2 * k + j) * NDUMP:(2 * k + j + 1) * NDUMP]
            print(json.dumps({"kernel": "fold_dump_kernel<%d>" % nprod, "nfscr": nfscr, "median_us": float(np.median(u)) / 1e3, "min_us": min(u) / 1e3,
                              "max_us": max(u) / 1e3, "launches": len(u)}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
