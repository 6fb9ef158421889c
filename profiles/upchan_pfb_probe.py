"""The PFB front end of UpchanBeamform and UpchanCorr (xengUpchanSetPfb / xengUpchanCorrSetPfb) against the plain FFT, P = 1
and P = 4 (default coefficients) alternating point by point in one process:

  * UpchanBeamform at the DESIGN.md 4.11 point: 704 inputs x 96 channels x 960-sample gulps, N = 32 (30 frames); nbeam 4 and 16;
    voltage and nframe_sum = 30;
  * UpchanCorr's gulp (stage kernel; the contraction and dump are not touched by the PFB) at the 4.12 points: N = 32 with 960
    samples and N = 2 with 480 samples, all fine channels, nstage 8.

Prints one JSON line per point (host view of back-to-back calls ending in a synchronise).  For the device time of the kernels
run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/upchan_pfb_probe.py

and group the kernel trace by kernel name (the PFB instantiations carry `xeng::UcPfb` as their last template argument) and grid
size."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.pfb import pfb_coeffs  # noqa: E402

NINPUT, NCHAN = 704, 96


def set_pfb(name, ntap, n):
    h = pfb_coeffs(ntap, n) if ntap > 1 else None
    ffi.call(name, ntap, None if h is None else h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))


def beam_point(din, nbeam, nframe_sum, ntap, reps, ntime=960, n=32):
    ffi.call("xengUpchanInitialize", 0, NINPUT, NCHAN, ntime, n, nbeam, nframe_sum)
    set_pfb("xengUpchanSetPfb", ntap, n)
    nframe = ntime // n
    wbytes = NCHAN * n * nbeam * NINPUT * 8
    obytes = (nframe // nframe_sum if nframe_sum else nframe) * nbeam * NCHAN * n * (4 if nframe_sum else 8)
    dw = ffi.DeviceBuffer(wbytes).upload(np.random.default_rng(nbeam).standard_normal(wbytes // 4).astype(np.float32))
    dout = ffi.DeviceBuffer(obytes)
    for _ in range(5):
        ffi.call("xengUpchanRun", din.ptr, dout.ptr, dw.ptr, 1)
    ffi.call("xengUpchanSync")
    t0 = time.perf_counter()
    for _ in range(reps):
        ffi.call("xengUpchanRun", din.ptr, dout.ptr, dw.ptr, 1)
    ffi.call("xengUpchanSync")
    dt = (time.perf_counter() - t0) / reps
    print(json.dumps({"what": "xengUpchanRun back to back (host view, ends in a synchronise)", "pfb_ntap": ntap, "nbeam": nbeam,
                      "nframe_sum": nframe_sum, "nupchan": n, "us_per_call": dt * 1e6, "reps": reps + 5}), flush=True)
    ffi.call("xengUpchanDestroy")


def corr_point(din, n, ntime, ntap, reps):
    ffi.call("xengUpchanCorrInitialize", 0, NINPUT, NCHAN, ntime, n, 0, NCHAN * n, 8)
    set_pfb("xengUpchanCorrSetPfb", ntap, n)
    for _ in range(8):
        ffi.call("xengUpchanCorrAccumulate", din.ptr)
    ffi.call("xengUpchanCorrReset")
    ffi.call("xengUpchanCorrSync")
    t0 = time.perf_counter()
    for _ in range(reps):
        ffi.call("xengUpchanCorrAccumulate", din.ptr)
    ffi.call("xengUpchanCorrSync")
    dt = (time.perf_counter() - t0) / reps
    print(json.dumps({"what": "xengUpchanCorrAccumulate back to back (stage kernels + a contraction every 8; host view)", "pfb_ntap": ntap,
                      "nupchan": n, "ntime": ntime, "us_per_call": dt * 1e6, "reps": reps + 8}), flush=True)
    ffi.call("xengUpchanCorrDestroy")


def main():
    vin = np.random.default_rng(0).integers(0, 256, 960 * NCHAN * NINPUT, dtype=np.uint8)
    din = ffi.DeviceBuffer(vin.nbytes).upload(vin)
    for nbeam in (4, 16):
        for nframe_sum in (0, 30):
            for ntap in (1, 4):
                beam_point(din, nbeam, nframe_sum, ntap, 40)
    for n, ntime in ((32, 960), (2, 480)):
        for ntap in (1, 4):
            corr_point(din, n, ntime, ntap, 32)


if __name__ == "__main__":
    main()
