"""UpchanPredict's kernel (xengPredict*, csrc/predict_kernels.h) at the point of its issue: 704 inputs (352 stands) x 96 fine channels,
32 and 1024 components per channel (one list for all channels' groups, nfavg 1), with and without the cross hands.  Prints one JSON
line per point with the host view of back-to-back runs ending in a synchronise beside the two floors: the bytes of the contract --
the lower triangle read once, the whole matrix written once -- over the measured HBM copy bandwidth, and the model's MFMA work, 8 x
1024 FLOP per record, product and tile pair, over the measured fp32 MFMA rate.  Input plus output are 382 MB, more than the 256 MiB
Infinity Cache holds.  For the device time of the kernel run it, in a run of its own, under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- timeout -k 10 300 python3 profiles/predict_probe.py
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
from caltech_bifrost_dsp_amd.backend import HipBackend  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.imaging import CLEAN_COMPONENT, steering_delays  # noqa: E402

NSTAND, NFINE, NDIR = 352, 96, 1024
POINTS = [(32, 0, 20), (32, 1, 20), (1024, 0, 5), (1024, 1, 5)]      # (ncomp, cross, runs)
HBM_TBS = 6.3                           # measured (MI355X_MICROARCH.md: HBM3E, float4 copy)
MFMA_TFS = 155.0                        # fp32 MFMA, measured


def geometry(rng):
    lm = rng.uniform(-0.65, 0.65, (NDIR, 2))
    lmn = np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)
    r = 1200.0 * np.sqrt(rng.uniform(size=NSTAND))
    a = rng.uniform(0, 2 * np.pi, NSTAND)
    pos = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-5, 5, NSTAND)], axis=-1)
    return steering_delays(pos, lmn)


def point(bf, rng, tau, din, dout, ncomp, cross, reps):
    ffi.check("xengPredictInitialize", bf.predict_initialize(0, NSTAND, NFINE, 1, NDIR, ncomp, cross))
    ffi.check("xengPredictSetGeometry", bf.predict_set_geometry(tau, np.ascontiguousarray(50e6 + 11962.890625 * np.arange(NFINE))))
    rec = np.zeros((NFINE, ncomp), CLEAN_COMPONENT)
    rec['pixel'] = rng.integers(0, NDIR, (NFINE, ncomp))
    rec['C'] = rng.uniform(-1, 1, (NFINE, ncomp, 4))
    ffi.check("xengPredictSetComponents", bf.predict_set_components(rec))

    def run(n):
        for _ in range(n):
            ffi.call("xengPredictRun", din.ptr, dout.ptr)
        ffi.call("xengPredictSync")
    run(2)
    t0 = time.perf_counter()
    run(reps)
    us = (time.perf_counter() - t0) / reps * 1e6
    info = bf.predict_info()
    ffi.call("xengPredictDestroy")
    return us, info


def main():
    rng = np.random.default_rng(1)
    ninput = 2 * NSTAND
    bf = HipBackend()
    chan = ninput * ninput * 8
    din, dout = ffi.DeviceBuffer(NFINE * chan), ffi.DeviceBuffer(NFINE * chan)
    for c in range(NFINE):              # (one random channel, rolled: the kernel's time does not depend on the values)
        v = rng.standard_normal(2 * ninput * ninput).astype(np.float32) if c < 4 else v
        din.upload(np.roll(v, c), c * chan)
    tau = geometry(rng)
    read = float(NFINE) * ninput * (ninput + 1) / 2 * 8
    written = float(NFINE) * chan
    for ncomp, cross, reps in POINTS:
        us, info = point(bf, rng, tau, din, dout, ncomp, cross, reps)
        ntile, nprod = info[0], 4 if cross else 2
        flop = 8.0 * 1024 * (ntile * (ntile + 1) // 2) * nprod * ncomp * NFINE
        print(json.dumps({"what": "xengPredictRun x %d back to back (host view, ends in a synchronise)" % reps, "nstand": NSTAND, "nfine": NFINE, "ncomp": ncomp,
                          "cross": cross, "us_per_run_host": us, "bytes_read": read, "bytes_written": written,
                          "hbm_floor_us": (read + written) / (HBM_TBS * 1e12) * 1e6, "gflop_mfma": flop / 1e9, "mfma_floor_us": flop / (MFMA_TFS * 1e12) * 1e6,
                          "tiles_per_side": ntile, "work_groups": info[1], "lds_bytes": info[2], "state_bytes": info[4]}), flush=True)
    din.free()
    dout.free()


if __name__ == "__main__":
    main()
