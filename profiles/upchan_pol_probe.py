"""UpchanBeamform's dual-pol mode (xengUpchanInitializeDualPol) against the power mode at the same beams: 704 inputs, 96
channels, 960-sample gulps, nupchan 32 (30 frames), 4 and 16 single-pol beams (2 and 8 pairs), windows of 1 and 30 frames.  The
two modes alternate point by point on one input.  Prints one JSON line per point (host view of back-to-back calls ending in a
synchronise).  For the device time of the kernels run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/upchan_pol_probe.py

and group the kernel trace by (kernel name, work-group size, grid size): each point has its own triple (the launch line it
prints says which)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402

NINPUT, NCHAN, NTIME, N = 704, 96, 960, 32


def launch(nbeam, nframe_sum, dual):
    """(kernel template arguments, work-group size, grid size) as upchan.hip picks them"""
    nthr = 256 if nbeam * N >= 256 else (nbeam * N + 63) // 64 * 64
    ppt = -(-nbeam // 2 * N // nthr) * 2 if dual else -(-nbeam * N // nthr)
    ppt = 4 if ppt == 3 else ppt
    run = nframe_sum * (8 // nframe_sum) if nframe_sum <= 8 else nframe_sum
    nframe = NTIME // N
    return "<%d, %d, %s>" % (N, ppt, "true" if dual else "false"), nthr, NCHAN * (-(-nframe // run)) * nthr


def point(din, nbeam, nframe_sum, dual, reps):
    nframe = NTIME // N
    ffi.call("xengUpchanInitializeDualPol" if dual else "xengUpchanInitialize", 0, NINPUT, NCHAN, NTIME, N, nbeam, nframe_sum)
    wbytes = NCHAN * N * nbeam * NINPUT * 8
    obytes = nframe // nframe_sum * NCHAN * N * (nbeam // 2 * 16 if dual else nbeam * 4)
    w = np.random.default_rng(nbeam).standard_normal(wbytes // 4).astype(np.float32)
    dw = ffi.DeviceBuffer(wbytes).upload(w)
    dout = ffi.DeviceBuffer(obytes)
    for _ in range(5):
        ffi.call("xengUpchanRun", din.ptr, dout.ptr, dw.ptr, 1)
    ffi.call("xengUpchanSync")
    t0 = time.perf_counter()
    for _ in range(reps):
        ffi.call("xengUpchanRun", din.ptr, dout.ptr, dw.ptr, 1)
    ffi.call("xengUpchanSync")
    dt = (time.perf_counter() - t0) / reps
    kern, nthr, grid = launch(nbeam, nframe_sum, dual)
    print(json.dumps({"what": "xengUpchanRun back to back (host view, ends in a synchronise)", "mode": "dual-pol" if dual else "power",
                      "nbeam": nbeam, "nframe_sum": nframe_sum, "us_per_call": dt * 1e6, "out_bytes": obytes, "reps": reps + 5,
                      "kernel": kern, "workgroup": nthr, "grid": grid}), flush=True)
    ffi.call("xengUpchanDestroy")


def main():
    vin = np.random.default_rng(0).integers(0, 256, NTIME * NCHAN * NINPUT, dtype=np.uint8)
    din = ffi.DeviceBuffer(vin.nbytes).upload(vin)
    for nbeam in (4, 16):
        for nframe_sum in (1, 30):
            for dual in (False, True):
                point(din, nbeam, nframe_sum, dual, 50)


if __name__ == "__main__":
    main()
