"""BeamCandFold (xengCandfoldRun) at a full table: 1024 candidates on 2 pairs x 256 DM trials = 512 series (two candidates a series),
segments of NT = 2^20 windows in 64 sub-integrations x 64 bins, nprod = 1, 33 x 17 = 561 trials, 6 widths.  WARM warm-up segments
and then REPS segments are streamed, each as NT / NWIN calls of NWIN = 1024 windows over the same span of noise, ending in a
synchronise; one JSON line with the host view.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/candfold_probe.py

(a run of its own: no counters in it) then `python3 profiles/candfold_probe.py --summarize OUT`: the device time of the timed
launches of each kernel from the kernel trace, summed per segment."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NDM, NCAND, NBIN, NSUB, NSUBWIN, NWIDTH, NWIN, NDRIFT, NCURVE = 2, 256, 1024, 64, 64, 1 << 14, 6, 1024, 16, 8
NT = NSUB * NSUBWIN
WARM, REPS = 1, 2                                                       # segments
KERNELS = ("candfold_fold_kernel", "candfold_refine_kernel", "candfold_clear_kernel")


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.backend import HipBackend
    from caltech_bifrost_dsp_amd.blocks import candfold_gains, candfold_trials, fold_phase

    rng = np.random.default_rng(0)
    nser = NPAIR * NDM
    x = (55 + rng.standard_normal(NWIN * nser)).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    dout = ffi.DeviceBuffer(NCAND * (16 + 4 * NBIN))
    d1, d2 = candfold_trials(NDRIFT, NCURVE)
    be = HipBackend()
    ffi.check("xengCandfoldInitialize", be.candfold_initialize(0, NPAIR, NDM, NWIN, 1, NCAND, NBIN, NSUB, NSUBWIN, NWIDTH, d1, d2, candfold_gains(NBIN, NWIDTH)))
    # periods of 3 to 3000 windows, log-spaced: shorter than a profile and much longer
    oscs = [fold_phase(1.0 / p, 0.0, 0.0, 0.0, 1.0) for p in np.exp(np.linspace(np.log(3.0), np.log(3000.0), NCAND))]
    ffi.check("xengCandfoldSetCandidates", be.candfold_set_candidates([c % nser for c in range(NCAND)], [o[0] for o in oscs], [o[1] for o in oscs],
                                                                       [o[2] for o in oscs], [1] * NCAND))
    done = ctypes.c_int()

    def segments(n):
        for _ in range(n * (NT // NWIN)):
            ffi.call("xengCandfoldRun", din.ptr, NWIN, dout.ptr, ctypes.byref(done))
        ffi.call("xengCandfoldSync")

    segments(WARM)
    t0 = time.perf_counter()
    segments(REPS)
    dt = (time.perf_counter() - t0) / REPS
    print(json.dumps(dict(npair=NPAIR, ndm=NDM, ncand=NCAND, nbin=NBIN, nsub=NSUB, nsubwin=NSUBWIN, nwidth=NWIDTH, ntrial=int(d1.size), nwin=NWIN,
                          what="xengCandfoldRun, one segment of NT windows in calls of NWIN windows (host view, ends in a synchronise)",
                          ms_per_segment=dt * 1e3, segments=WARM + REPS)), flush=True)
    ffi.call("xengCandfoldDestroy")
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
        assert t and len(t) % (WARM + REPS) == 0, "%d launches of %s in the trace" % (len(t), kernel)
        per_seg = len(t) // (WARM + REPS)
        u = t[WARM * per_seg:]
        print(json.dumps({"kernel": kernel, "launches_per_segment": per_seg, "device_ms_per_segment": sum(u) / REPS / 1e6, "median_us": float(np.median(u)) / 1e3}))
        total += sum(u) / REPS / 1e6
    print(json.dumps({"device_ms_per_segment": total}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
