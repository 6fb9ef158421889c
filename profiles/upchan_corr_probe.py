"""UpchanCorr's kernels (xengUpchanCorr*, csrc/upchan_corr_kernels.h) at the points of its issue: 704 inputs x 96 channels with
960-sample gulps at nupchan 32 (config 4's gulp: 3072 fine channels x 30 frames), and the reference script's nupchan 2 with
480-sample gulps (192 fine channels x 240 frames), every fine channel, the default staging depth.  Prints one JSON line per
point: the host view of a run of back-to-back gulps ending in a dump and a synchronise, and per gulp the FLOP, the bytes the
kernels move and the two bounds they imply (fp32 MFMA peak, HBM).  For the device time of each kernel run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/upchan_corr_probe.py
"""
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

NINPUT, NCHAN = 704, 96
HBM_TBS = 6.3           # the issue's round figure for the achievable HBM rate
MFMA_TFS = 155.0        # fp32 MFMA, measured (MI355X_MICROARCH.md, Matrix cores)


def point(din, ntime, N, reps):
    nfine, nframe = NCHAN * N, ntime // N
    ffi.call("xengUpchanCorrInitialize", 0, NINPUT, NCHAN, ntime, N, 0, nfine, 0)
    a, nstage = ctypes.c_int(), ctypes.c_int()
    ffi.call("xengUpchanCorrGetInfo", ctypes.byref(a), ctypes.byref(nstage))
    nstage = nstage.value
    dout = ffi.DeviceBuffer(nfine * NINPUT * NINPUT * 8)
    gulp = ntime * NCHAN * NINPUT
    ngulp = din.nbytes // gulp

    def run(n):
        for k in range(n):
            ffi.call("xengUpchanCorrAccumulate", din.ptr + (k % ngulp) * gulp)
        ffi.call("xengUpchanCorrDump", dout.ptr)
        ffi.call("xengUpchanCorrSync")
    run(nstage)
    t0 = time.perf_counter()
    run(reps)
    dt = time.perf_counter() - t0
    ntile = (NINPUT + 31) // 32
    ntp = ntile * (ntile + 1) // 2
    nfp = nframe + (nframe & 1)
    tri = NINPUT * (NINPUT + 1) // 2
    flop_useful = 8.0 * nfine * nframe * tri                 # the issue's count (lower triangle with the diagonal)
    flop_mfma = 8.0 * nfine * nfp * ntp * 1024               # what the 32x32 tiles compute (whole diagonal tiles, pad frames)
    acc = nfine * ntp * 8192.0
    stage = nfine * nfp * NINPUT * 8.0
    per_gulp = gulp + 2 * stage + 2 * acc / nstage           # input, staging written + read, accumulator read + written per contraction
    print(json.dumps({"what": "xengUpchanCorrAccumulate x %d + Dump back to back (host view, ends in a synchronise)" % reps,
                      "ninput": NINPUT, "nchan": NCHAN, "ntime": ntime, "nupchan": N, "nfine": nfine, "nframe": nframe, "nstage": nstage,
                      "ms_per_gulp_host": dt / reps * 1e3, "gflop_per_gulp": flop_useful / 1e9, "gflop_mfma_per_gulp": flop_mfma / 1e9,
                      "compute_bound_ms": flop_useful / (MFMA_TFS * 1e12) * 1e3, "bytes_per_gulp": per_gulp,
                      "hbm_bound_ms": per_gulp / (HBM_TBS * 1e12) * 1e3, "acc_bytes": acc, "stage_bytes": stage * nstage,
                      "dump_bytes": acc + nfine * NINPUT * NINPUT * 8.0,
                      "dump_hbm_bound_ms": (acc + nfine * NINPUT * NINPUT * 8.0) / (HBM_TBS * 1e12) * 1e3, "reps": reps}), flush=True)
    dout.free()
    ffi.call("xengUpchanCorrDestroy")


def main():
    for ntime, N, reps in ((960, 32, 16), (480, 2, 16)):
        vin = np.random.default_rng(N).integers(0, 256, 2 * ntime * NCHAN * NINPUT, dtype=np.uint8)
        din = ffi.DeviceBuffer(vin.nbytes).upload(vin)
        point(din, ntime, N, reps)
        din.free()


if __name__ == "__main__":
    main()
