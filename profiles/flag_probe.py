"""UpchanFlag's kernels (xengFlag*, csrc/flag_kernels.h) at the point of their issue: 704 inputs (352 stands) x 96 fine channels.
Prints one JSON line: the host view of back-to-back runs ending in a synchronise (three launches per run; the input of 381 MB is
larger than the Infinity Cache, so every run streams it from HBM), beside the bound: the bytes of the lower triangle, nfine * ninput
(ninput + 1) / 2 * 8 -- the parallel hands the statistics use lie 16 bytes apart, so every 128-byte line of the lower triangle is
fetched -- over the measured HBM bandwidth.  For the device time of each of the three kernels run it, in a run of its own, under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- timeout -k 10 300 python3 profiles/flag_probe.py
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

NSTAND, NFINE = 352, 96
HBM_TBS = 6.3                           # measured (MI355X_MICROARCH.md: HBM3E)


def main():
    rng = np.random.default_rng(1)
    ninput = 2 * NSTAND
    bf = HipBackend()
    chan = ninput * ninput * 8
    din = ffi.DeviceBuffer(NFINE * chan)
    for c in range(NFINE):              # (one random channel, rolled: the kernels' time does not depend on the values)
        v = rng.standard_normal(2 * ninput * ninput).astype(np.float32) if c < 4 else v
        din.upload(np.roll(v, c), c * chan)
    ffi.check("xengFlagInitialize", bf.flag_initialize(0, NSTAND, NFINE))
    mask_bytes, stats_bytes, chan_bytes, lds = bf.flag_info()
    stats_offset = (mask_bytes + 15) & ~15
    chan_offset = stats_offset + stats_bytes
    dout = ffi.DeviceBuffer(chan_offset + chan_bytes)
    reps = 50

    def run(n):
        for _ in range(n):
            ffi.call("xengFlagRun", din.ptr, dout.ptr, dout.ptr + stats_offset, dout.ptr + chan_offset)
        ffi.call("xengFlagSync")
    run(3)
    t0 = time.perf_counter()
    run(reps)
    us = (time.perf_counter() - t0) / reps * 1e6
    low = float(NFINE) * ninput * (ninput + 1) / 2 * 8
    ntile = (NSTAND + 31) // 32
    print(json.dumps({"what": "xengFlagRun x %d back to back (host view, ends in a synchronise)" % reps, "nstand": NSTAND, "nfine": NFINE,
                      "us_per_integration_host": us, "lower_triangle_bytes": low, "hbm_bound_us": low / (HBM_TBS * 1e12) * 1e6,
                      "ratio_to_hbm_bound": us / (low / (HBM_TBS * 1e12) * 1e6), "lds_bytes": lds,
                      "work_groups": [ntile * (ntile + 1) // 2 * NFINE, 2 * NFINE, 2]}), flush=True)
    ffi.call("xengFlagDestroy")
    din.free()
    dout.free()


if __name__ == "__main__":
    main()
