"""UpchanCalApply's kernel (xengCalapply*, csrc/calapply_kernels.h) at the point of its issue: 704 inputs (352 stands) x 96 fine channels x
32 sources.  Prints one JSON line with the host view of back-to-back runs ending in a synchronise (with the model and without)
beside the bound: the bytes of the contract -- the lower triangle read once, the whole matrix written once -- over the measured HBM
copy bandwidth, and the model's MFMA work over the measured fp32 MFMA rate.  Input plus output are 382 MB, more than the 256 MiB
Infinity Cache holds.  For the device time of the kernel run it, in a run of its own, under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- timeout -k 10 300 python3 profiles/calapply_probe.py
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
from caltech_bifrost_dsp_amd.blocks.imaging import steering_delays  # noqa: E402

NSTAND, NFINE, NSRC = 352, 96, 32
HBM_TBS = 6.3                           # measured (MI355X_MICROARCH.md: HBM3E, float4 copy)
MFMA_TFS = 155.0                        # fp32 MFMA, measured


def geometry(rng, nsrc):
    lm = rng.uniform(-0.65, 0.65, (nsrc, 2))
    lmn = np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)
    r = 1200.0 * np.sqrt(rng.uniform(size=NSTAND))
    a = rng.uniform(0, 2 * np.pi, NSTAND)
    pos = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-5, 5, NSTAND)], axis=-1)
    return steering_delays(pos, lmn)


def point(bf, rng, din, dout, nsrc, reps):
    ffi.check("xengCalapplyInitialize", bf.calapply_initialize(0, NSTAND, NFINE, nsrc))
    freq = np.ascontiguousarray(50e6 + 11962.890625 * np.arange(NFINE))
    if nsrc:
        ffi.check("xengCalapplySetModel", bf.calapply_set_model(geometry(rng, nsrc), freq, np.ascontiguousarray(rng.uniform(1, 10, (NFINE, nsrc)), np.float32)))
    h = (rng.uniform(0.5, 2.0, (NFINE, 2, NSTAND)) * np.exp(2j * np.pi * rng.uniform(size=(NFINE, 2, NSTAND)))).astype(np.complex64)
    ffi.check("xengCalapplySetFactors", bf.calapply_set_factors(h))

    def run(n):
        for _ in range(n):
            ffi.call("xengCalapplyRun", din.ptr, dout.ptr)
        ffi.call("xengCalapplySync")
    run(2)
    t0 = time.perf_counter()
    run(reps)
    us = (time.perf_counter() - t0) / reps * 1e6
    info = bf.calapply_info()
    ffi.call("xengCalapplyDestroy")
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
    reps = 20
    us_model, info = point(bf, rng, din, dout, NSRC, reps)
    us_plain, _ = point(bf, rng, din, dout, 0, reps)
    read = float(NFINE) * ninput * (ninput + 1) / 2 * 8
    written = float(NFINE) * chan
    ntile = info[0]
    flop = 4.0 * 4096 * (NSRC // 2) * (ntile * (ntile + 1) // 2) * NFINE
    print(json.dumps({"what": "xengCalapplyRun x %d back to back (host view, ends in a synchronise)" % reps, "nstand": NSTAND, "nfine": NFINE, "nsrc": NSRC,
                      "us_per_run_host": us_model, "us_per_run_host_without_model": us_plain, "bytes_read": read, "bytes_written": written,
                      "hbm_floor_us": (read + written) / (HBM_TBS * 1e12) * 1e6, "gflop_mfma": flop / 1e9, "mfma_floor_us": flop / (MFMA_TFS * 1e12) * 1e6,
                      "tiles_per_side": ntile, "work_groups": info[1], "lds_bytes": info[2]}), flush=True)
    din.free()
    dout.free()


if __name__ == "__main__":
    main()
