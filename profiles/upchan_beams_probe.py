"""UpchanSumBeams (xengUpchanSumBeamsRun) at the live beam size, 96 channels x 32 beams x 960-sample gulps, N = 32 (30 frames),
all 16 pairs, at P = 1 and 4 (default coefficients) and W = 30 (one window per gulp) and 750 (one per 25 gulps), next to the
beamformer's own kernels on the same gulp: xengBeamformRun (704 inputs -> 32 beams) and xengBeamformIntegrate (BeamformSumBeams,
beam_integrate_kernel, ntime_sum 24).  Every point is 5 warm-up launches and then REPS back to back, ending in a synchronise;
one JSON line per point with the host view.

Device time: run it under

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 profiles/upchan_beams_probe.py

then `python3 profiles/upchan_beams_probe.py --summarize OUT`: the median device time of the timed launches of each point, from
the kernel trace (the points run one after another, so the trace's launches of upchan_sum_beams_kernel split by count)."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NINPUT, NCHAN, NBEAM, NTIME, N = 704, 96, 32, 960, 32
WARM, REPS = 5, 60
POINTS = [(1, 30), (4, 30), (1, 750), (4, 750)]         # (pfb_ntap, nframe_sum), in launch order


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.blocks.pfb import pfb_coeffs

    rng = np.random.default_rng(0)
    vin = rng.integers(0, 256, NTIME * NCHAN * NINPUT, dtype=np.uint8)
    din = ffi.DeviceBuffer(vin.nbytes).upload(vin)
    beams = (rng.standard_normal(NCHAN * NBEAM * NTIME) + 1j * rng.standard_normal(NCHAN * NBEAM * NTIME)).astype(np.complex64)
    dbeam = ffi.DeviceBuffer(beams.nbytes).upload(beams)
    dout = ffi.DeviceBuffer(NBEAM // 2 * NCHAN * N * 16)

    def timed(what, call, sync, extra):
        for _ in range(WARM):
            call()
        ffi.call(sync)
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        ffi.call(sync)
        dt = (time.perf_counter() - t0) / REPS
        rec = {"what": what + " back to back (host view, ends in a synchronise)", "us_per_call": dt * 1e6, "launches": WARM + REPS}
        rec.update(extra)
        print(json.dumps(rec), flush=True)

    for ntap, w in POINTS:
        ffi.call("xengUpchanSumBeamsInitialize", 0, NCHAN, NBEAM, NTIME, N, 0, NBEAM // 2, w)
        if ntap > 1:
            h = pfb_coeffs(ntap, N)
            ffi.call("xengUpchanSumBeamsSetPfb", ntap, h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        timed("xengUpchanSumBeamsRun", lambda: ffi.call("xengUpchanSumBeamsRun", dbeam.ptr, dout.ptr), "xengUpchanSumBeamsSync",
              {"pfb_ntap": ntap, "nframe_sum": w, "nupchan": N, "nchan": NCHAN, "nbeam": NBEAM, "ntime": NTIME})
        ffi.call("xengUpchanSumBeamsDestroy")
    w = (rng.uniform(-1, 1, (NCHAN, NBEAM, NINPUT)) + 1j * rng.uniform(-1, 1, (NCHAN, NBEAM, NINPUT))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, NINPUT, NCHAN, NTIME, NBEAM, 0)
    dw = ffi.DeviceBuffer(w.nbytes).upload(w)
    dpow = ffi.DeviceBuffer(NBEAM // 2 * (NTIME // 24) * NCHAN * 16)
    timed("xengBeamformRun", lambda: ffi.call("xengBeamformRun", din.ptr, dbeam.ptr, dw.ptr), "xengBeamformSync", {"ninput": NINPUT, "nbeam": NBEAM})
    timed("xengBeamformIntegrate", lambda: ffi.call("xengBeamformIntegrate", dbeam.ptr, dpow.ptr, 24), "xengBeamformSync", {"ntime_sum": 24})
    ffi.call("xengBeamformDestroy")


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    med = lambda ts: float(np.median(ts)) / 1e3 if ts else None         # ns -> us
    ub = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "upchan_sum_beams_kernel" in r["Kernel_Name"]]
    per = WARM + REPS
    assert len(ub) == per * len(POINTS), "%d upchan_sum_beams_kernel launches in the trace, %d expected" % (len(ub), per * len(POINTS))
    for k, (ntap, w) in enumerate(POINTS):
        t = ub[k * per + WARM:(k + 1) * per]
        print(json.dumps({"kernel": "upchan_sum_beams_kernel", "pfb_ntap": ntap, "nframe_sum": w, "median_us": med(t), "min_us": min(t) / 1e3,
                          "max_us": max(t) / 1e3, "launches": len(t)}))
    names = sorted({r["Kernel_Name"] for r in rows if "upchan_sum_beams" not in r["Kernel_Name"]})
    for name in names:
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if r["Kernel_Name"] == name]
        if len(t) >= REPS:
            print(json.dumps({"kernel": name[:120], "median_us": med(t[WARM:]), "launches": len(t) - WARM}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
