"""UpchanSpectra (xengUpchanSpectraRun) at the live size, 704 inputs x 96 channels x 960-sample gulps, N = 32 (30 frames), at
P = 1 and 4 (default coefficients) and W = 30 (one window per gulp) and 750 (one per 25 gulps), alternating launch by launch with
UpchanCorr's stage kernel (xengUpchanCorrAccumulate, every fine channel, the same P) on the same gulp: upchan_corr_stage_kernel
does the same decode + FFT and writes the channelised data (519 MB) instead of reducing it, and is the yardstick.  Every point is
WARM warm-up rounds and then REPS rounds, ending in a synchronise; one JSON line per point with the host view, the bytes the
kernel has to move and the HBM bound they imply.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/upchan_spectra_probe.py

then `python3 profiles/upchan_spectra_probe.py --summarize OUT`: the median device time of the timed launches of each point and
of the yardstick beside it, from the kernel trace (the points run one after another, so the launches of each kernel split by
count).

`--nslot 1,2,8` adds points at P = 1, W = 30 with that many frame slots per work-group; it needs a -DXENG_DIAGNOSTICS build of
the library (XENG_LIB=profiles/_ab/libxeng_diag.so, profiles/build_diag.sh), the shipped one ignores XENG_SPECTRA_NSLOT.  The
slot count is part of the configuration: it changes the order of the sums, so the last bits, and nothing else."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NINPUT, NCHAN, NTIME, N = 704, 96, 960, 32
WARM, REPS = 5, 45
HBM_TBS = 6.3           # the achievable HBM rate (MI355X_MICROARCH: 6.29 TB/s measured)
POINTS = [(1, 30, 0), (4, 30, 0), (1, 750, 0), (4, 750, 0)]         # (pfb_ntap, nframe_sum, nslot override or 0), in launch order


def points(argv):
    pts = list(POINTS)
    if "--nslot" in argv:
        pts += [(1, 30, int(s)) for s in argv[argv.index("--nslot") + 1].split(",")]
    return pts


def run_points(pts):
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.blocks.pfb import pfb_coeffs

    rng = np.random.default_rng(0)
    vin = rng.integers(0, 256, NTIME * NCHAN * NINPUT, dtype=np.uint8)
    din = ffi.DeviceBuffer(vin.nbytes).upload(vin)
    plane = NCHAN * N * NINPUT * 4
    dout = ffi.DeviceBuffer(2 * plane)
    F = NTIME // N
    for ntap, w, nslot in pts:
        if nslot:
            os.environ["XENG_SPECTRA_NSLOT"] = str(nslot)
        else:
            os.environ.pop("XENG_SPECTRA_NSLOT", None)
        ffi.call("xengUpchanSpectraInitialize", 0, NINPUT, NCHAN, NTIME, N, w)
        # (two staging slots and a Reset before every Accumulate: each Accumulate is a stage kernel alone, no contraction is ever due)
        ffi.call("xengUpchanCorrInitialize", 0, NINPUT, NCHAN, NTIME, N, 0, NCHAN * N, 2)
        if ntap > 1:
            h = pfb_coeffs(ntap, N)
            ffi.call("xengUpchanSpectraSetPfb", ntap, h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
            ffi.call("xengUpchanCorrSetPfb", ntap, h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))

        def round_():
            ffi.call("xengUpchanSpectraRun", din.ptr, dout.ptr)
            ffi.call("xengUpchanCorrReset")
            ffi.call("xengUpchanCorrAccumulate", din.ptr)
        for _ in range(WARM):
            round_()
        ffi.call("xengUpchanSpectraSync")
        t0 = time.perf_counter()
        for _ in range(REPS):
            round_()
        ffi.call("xengUpchanSpectraSync")
        dt = (time.perf_counter() - t0) / REPS
        gpw = max(1, w // F)
        moved = vin.nbytes + (2 * plane / gpw if gpw == 1 else 2 * 2 * plane * (gpw - 1) / gpw + 2 * plane / gpw)
        print(json.dumps({"what": "xengUpchanSpectraRun + xengUpchanCorrAccumulate (stage kernel) alternating (host view of the pair)",
                          "pfb_ntap": ntap, "nframe_sum": w, "nslot_override": nslot, "us_per_pair_host": dt * 1e6, "launches": WARM + REPS,
                          "spectra_bytes_per_gulp": moved, "spectra_hbm_bound_us": moved / (HBM_TBS * 1e12) * 1e6,
                          "stage_bytes_per_gulp": vin.nbytes + NCHAN * N * F * NINPUT * 8.0}), flush=True)
        ffi.call("xengUpchanCorrDestroy")
        ffi.call("xengUpchanSpectraDestroy")


def summarize(out, pts):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + REPS
    for kernel in ("upchan_spectra_kernel", "upchan_corr_stage_kernel"):
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        assert len(t) == per * len(pts), "%d %s launches in the trace, %d expected" % (len(t), kernel, per * len(pts))
        for k, (ntap, w, nslot) in enumerate(pts):
            d = np.array(t[k * per + WARM:(k + 1) * per]) / 1e3          # ns -> us
            print(json.dumps({"kernel": kernel, "pfb_ntap": ntap, "nframe_sum": w, "nslot_override": nslot, "median_us": float(np.median(d)),
                              "min_us": float(d.min()), "max_us": float(d.max()), "launches": len(d)}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], points(sys.argv))
    else:
        run_points(points(sys.argv))
