"""BeamDetrend (xengDetrendRun) at the live shape: 16 pairs x NDM trials (256 by default, `--ndm 1024` for the other point),
nprod = 1, calls of NWIN = 30 windows, blocks of NBLK = 1000 windows (D = 1500 windows = 50 spans; a block is decided on one call in
33 or 34).  WARM warm-up calls and then REPS calls are made over the same span of noise, ending in a synchronise; one JSON line with
the host view.

Counted traffic: ingest reads the span and writes it into the ring, apply reads it back and writes the output (4 spans of
nwin nser 4 bytes a call; the knots sit in L2), decide reads one block once, nblk nser 4 bytes.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/detrend_probe.py

(a run of its own: no counters in it) then `python3 profiles/detrend_probe.py --summarize OUT [--ndm N]`: the device time of the
timed launches of each kernel from the kernel trace, decide's own time per launch (it runs on block-ending calls only and is not
averaged over the calls), and each beside its counted traffic at 6.3 TB/s."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NWIN, NBLK = 16, 30, 1000
NDM = int(sys.argv[sys.argv.index("--ndm") + 1]) if "--ndm" in sys.argv else 256
WARM, REPS = 100, 400                                                   # calls (3 and 12 blocks)
KERNELS = ("detrend_ingest_kernel", "detrend_decide_kernel", "detrend_apply_kernel")
NSER = NPAIR * NDM
SPAN_BYTES = NWIN * NSER * 4
BLOCK_BYTES = NBLK * NSER * 4
HBM_BYTES_PER_S = 6.3e12


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.backend import HipBackend
    from caltech_bifrost_dsp_amd.blocks import detrend_k_mad

    rng = np.random.default_rng(0)
    x = ((rng.standard_normal((NWIN, NSER, 8)) ** 2).sum(axis=2) * 100.0).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    dout = ffi.DeviceBuffer(x.nbytes)
    be = HipBackend()
    ffi.check("xengDetrendInitialize", be.detrend_initialize(0, NPAIR, NDM, NWIN, 1, NBLK, 1, detrend_k_mad()))
    done = ctypes.c_int()

    def calls(n):
        decided = 0
        for _ in range(n):
            ffi.call("xengDetrendRun", din.ptr, NWIN, dout.ptr, ctypes.byref(done))
            decided += done.value
        ffi.call("xengDetrendSync")
        return decided

    calls(WARM)
    t0 = time.perf_counter()
    decided = calls(REPS)
    dt = (time.perf_counter() - t0) / REPS
    y = dout.download(np.float32)
    print(json.dumps(dict(npair=NPAIR, ndm=NDM, nwin=NWIN, nblk=NBLK, what="xengDetrendRun, one call of NWIN windows (host view, REPS calls and a synchronise)",
                          us_per_call=dt * 1e6, calls=WARM + REPS, blocks_decided_in_reps=decided, counted_mb_per_call=4 * SPAN_BYTES / 1e6,
                          counted_mb_per_block=BLOCK_BYTES / 1e6, out_std=float(y.std()))), flush=True)
    ffi.call("xengDetrendDestroy")
    for d in (din, dout):
        d.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    counted = {"detrend_ingest_kernel": 2 * SPAN_BYTES, "detrend_decide_kernel": BLOCK_BYTES, "detrend_apply_kernel": 2 * SPAN_BYTES}
    for kernel in KERNELS:
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        u = t[int(round(len(t) * WARM / float(WARM + REPS))):]
        print(json.dumps({"kernel": kernel, "launches": len(t), "timed_launches": len(u), "median_us_per_launch": float(np.median(u)) / 1e3,
                          "max_us_per_launch": max(u) / 1e3, "counted_us_at_6.3TBs": counted[kernel] / HBM_BYTES_PER_S * 1e6}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
