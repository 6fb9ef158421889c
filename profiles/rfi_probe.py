"""BeamRfiClean (xengRfiRun) at the live shape: 16 pairs x 3072 fine channels, calls of NWIN = 30 windows, blocks of NSTAT = 300
windows (a block is decided every tenth call).  WARM warm-up calls and then REPS calls are made over the same span of noise, ending
in a synchronise; one JSON line with the host view.

Counted traffic per call: the span in (23.6 MB), the span into the ring, the ring's span back, the span out, and the block tables
(about 2.4 MB a half, shared in L2): 94.4 MB + tables.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/rfi_probe.py

(a run of its own: no counters in it) then `python3 profiles/rfi_probe.py --summarize OUT`: the device time of the timed launches of
each kernel from the kernel trace and the fraction of the counted traffic at 6.3 TB/s that the call reaches."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NFINE, NWIN, NSTAT = 16, 3072, 30, 300
WARM, REPS = 20, 100                                                    # calls (both whole numbers of blocks)
KERNELS = ("rfi_ingest_kernel", "rfi_decide_kernel", "rfi_apply_kernel")
SPAN_BYTES = NWIN * NPAIR * NFINE * 16
COUNTED_BYTES = 4 * SPAN_BYTES
HBM_BYTES_PER_S = 6.3e12


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.backend import HipBackend
    from caltech_bifrost_dsp_amd.blocks import rfi_controls

    rng = np.random.default_rng(0)
    b = 10.0 ** (-np.arange(NFINE) / (NFINE - 1.0))[None, None, :, None] * 100.0
    x = (rng.standard_normal((NWIN, NPAIR, NFINE, 4)) * 0.1 * b)
    x[..., :2] += b
    x = x.astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    dout = ffi.DeviceBuffer(x.nbytes)
    dst = ffi.DeviceBuffer(NWIN * NPAIR * 16)
    be = HipBackend()
    ffi.check("xengRfiInitialize", be.rfi_initialize(0, NPAIR, NFINE, NWIN, NSTAT))
    ffi.check("xengRfiSetControl", be.rfi_set_control(*(rfi_controls(nfine=NFINE) + (1,))))
    done = ctypes.c_int()

    def calls(n):
        for _ in range(n):
            ffi.call("xengRfiRun", din.ptr, NWIN, dout.ptr, dst.ptr, ctypes.byref(done))
        ffi.call("xengRfiSync")

    calls(WARM)
    t0 = time.perf_counter()
    calls(REPS)
    dt = (time.perf_counter() - t0) / REPS
    st = dst.download(np.int32).reshape(NWIN, NPAIR, 4)
    print(json.dumps(dict(npair=NPAIR, nfine=NFINE, nwin=NWIN, nstat=NSTAT, what="xengRfiRun, one call of NWIN windows (host view, REPS calls and a synchronise)",
                          us_per_call=dt * 1e6, calls=WARM + REPS, counted_mb=COUNTED_BYTES / 1e6, mean_count=float(st[..., 0].mean()),
                          codes=sorted(set(st[..., 2].reshape(-1).tolist())))), flush=True)
    ffi.call("xengRfiDestroy")
    for d in (din, dout, dst):
        d.free()


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
        per_call = len(t) / float(WARM + REPS)
        u = t[int(round(WARM * per_call)):]
        print(json.dumps({"kernel": kernel, "launches": len(t), "launches_per_call": per_call, "device_us_per_call": sum(u) / REPS / 1e3,
                          "median_us": float(np.median(u)) / 1e3}))
        total += sum(u) / REPS / 1e3
    print(json.dumps({"device_us_per_call": total, "counted_us_at_6.3TBs": COUNTED_BYTES / HBM_BYTES_PER_S * 1e6,
                      "fraction_of_counted_rate": COUNTED_BYTES / HBM_BYTES_PER_S * 1e6 / total}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
