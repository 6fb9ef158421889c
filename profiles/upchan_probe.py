"""UpchanBeamform's kernel (xengUpchanRun, csrc/upchan_kernels.h) at the benchmark points of its issue: 704 inputs, 96 channels,
960-sample gulps (config 4's gulp), nupchan 32 (30 frames), 4 and 16 beams, voltage and power (nframe_sum 30) mode.  Prints one
JSON line per point: the host view of back-to-back calls ending in a synchronise, and the bytes and flops the kernel needs with
the HBM bound they imply.  For the device time of the kernel itself run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/upchan_probe.py
"""
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
HBM_TBS = 6.3           # the issue's round figure for the achievable HBM rate


def point(din, nbeam, nframe_sum, reps):
    nframe = NTIME // N
    ffi.call("xengUpchanInitialize", 0, NINPUT, NCHAN, NTIME, N, nbeam, nframe_sum)
    wbytes = NCHAN * N * nbeam * NINPUT * 8
    obytes = (nframe // nframe_sum if nframe_sum else nframe) * nbeam * NCHAN * N * (4 if nframe_sum else 8)
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
    nbytes = din.nbytes + wbytes + obytes
    flops = 8.0 * nbeam * NINPUT * nframe * NCHAN * N + 5.0 * N * np.log2(N) * nframe * NCHAN * NINPUT
    print(json.dumps({"what": "xengUpchanRun back to back (host view, ends in a synchronise)", "nbeam": nbeam, "nframe_sum": nframe_sum,
                      "us_per_call": dt * 1e6, "bytes": nbytes, "gflop": flops / 1e9, "hbm_bound_us": nbytes / (HBM_TBS * 1e12) * 1e6,
                      "reps": reps}), flush=True)
    ffi.call("xengUpchanDestroy")


def main():
    vin = np.random.default_rng(0).integers(0, 256, NTIME * NCHAN * NINPUT, dtype=np.uint8)
    din = ffi.DeviceBuffer(vin.nbytes).upload(vin)
    for nbeam in (4, 16):
        for nframe_sum in (0, 30):
            point(din, nbeam, nframe_sum, 100)


if __name__ == "__main__":
    main()
