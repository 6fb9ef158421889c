"""UpchanPeel's kernels (xengPeel*, csrc/peel_kernels.h) at the point of their issue: 704 inputs (352 stands) x 96 fine channels x 8
directions.  tol = 0, so a run takes exactly niter sweeps; two sweep counts give the time per sweep as a difference, free of the
launch, the tables and the subtraction; niter = 0 gives the subtraction (and the solve's prologue and epilogue) alone.  Prints one
JSON line per count (the host view of back-to-back runs ending in a synchronise) and one with the difference beside the bounds: the
bytes of V one sweep fetches (the pp words lie 16 bytes apart, so every cache line of the matrix is fetched once per sweep: nfine *
ninput^2 * 8) over the measured HBM and Infinity Cache bandwidths, and the MFMA time of the sweep's contraction.  For the device time
of the kernels run it, in a run of its own, under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- timeout -k 10 300 python3 profiles/peel_probe.py
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

NSTAND, NFINE, NDIR = 352, 96, 8
HBM_TBS, MALL_TBS = 6.3, 7.4            # measured (MI355X_MICROARCH.md: HBM3E; random rows of a table of 151 MB, the Infinity Cache's reach)
MFMA_TFS = 155.0                        # fp32 MFMA, measured


def geometry(rng):
    lm = rng.uniform(-0.65, 0.65, (NDIR, 2))
    lmn = np.concatenate([lm, np.sqrt(1 - (lm ** 2).sum(axis=1, keepdims=True))], axis=1)
    r = 1200.0 * np.sqrt(rng.uniform(size=NSTAND))
    a = rng.uniform(0, 2 * np.pi, NSTAND)
    pos = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-5, 5, NSTAND)], axis=-1)
    return steering_delays(pos, lmn)


def point(din, dout, dsol, niter, reps):
    ffi.call("xengPeelSetSolver", niter, 0.0)

    def run(n):
        for _ in range(n):
            ffi.call("xengPeelRun", din.ptr, dout.ptr, dsol.ptr, dsol.ptr + NFINE * 2 * NDIR * NSTAND * 8, 0)
        ffi.call("xengPeelSync")
    run(1)
    t0 = time.perf_counter()
    run(reps)
    ms = (time.perf_counter() - t0) / reps * 1e3
    print(json.dumps({"what": "xengPeelRun x %d back to back (host view, ends in a synchronise)" % reps, "nstand": NSTAND, "nfine": NFINE, "ndir": NDIR,
                      "niter": niter, "ms_per_run_host": ms, "reps": reps}), flush=True)
    return ms


def main():
    rng = np.random.default_rng(1)
    ninput = 2 * NSTAND
    bf = HipBackend()
    tau = geometry(rng)
    chan = ninput * ninput * 8
    din, dout = ffi.DeviceBuffer(NFINE * chan), ffi.DeviceBuffer(NFINE * chan)
    dsol = ffi.DeviceBuffer(NFINE * 2 * NDIR * NSTAND * 8 + NFINE * 2 * 4 * 4)
    for c in range(NFINE):              # (one random channel, rolled: the kernels' time does not depend on the values)
        v = rng.standard_normal(2 * ninput * ninput).astype(np.float32) if c < 4 else v
        din.upload(np.roll(v, c), c * chan)
    ffi.check("xengPeelInitialize", bf.peel_initialize(0, NSTAND, NFINE, NDIR))
    ffi.check("xengPeelSetModel", bf.peel_set_model(tau, np.ascontiguousarray(50e6 + 11962.890625 * np.arange(NFINE)),
                                                    np.ascontiguousarray(rng.uniform(1, 10, (NFINE, NDIR)), np.float32)))
    ffi.check("xengPeelSetWeights", bf.peel_set_weights(np.ones(NSTAND, np.float32), 0))
    lo, hi = 10, 40
    t_0, t_lo, t_hi = point(din, dout, dsol, 0, 3), point(din, dout, dsol, lo, 3), point(din, dout, dsol, hi, 3)
    vbytes = float(NFINE) * chan
    nsp = (NSTAND + 31) // 32 * 32
    flop_mfma = 4.0 * 2 * 16 * 16 * 4 * (nsp // 4) * (nsp // 16) * NFINE * 2
    print(json.dumps({"what": "one sweep, (t[%d] - t[%d]) / %d" % (hi, lo, hi - lo), "us_per_sweep_host": (t_hi - t_lo) / (hi - lo) * 1e3,
                      "us_subtraction_and_launches_host": t_0 * 1e3, "vis_bytes_per_sweep": vbytes, "hbm_bound_us": vbytes / (HBM_TBS * 1e12) * 1e6,
                      "infinity_cache_bound_us": vbytes / (MALL_TBS * 1e12) * 1e6, "gflop_mfma_per_sweep": flop_mfma / 1e9,
                      "mfma_floor_us": flop_mfma / (MFMA_TFS * 1e12) * 1e6, "subtraction_bytes": 1.5 * vbytes, "subtraction_floor_us": 1.5 * vbytes / (HBM_TBS * 1e12) * 1e6,
                      "lds_bytes": bf.peel_info()[0], "work_groups": NFINE * 2}), flush=True)
    ffi.call("xengPeelDestroy")
    for b in (din, dout, dsol):
        b.free()


if __name__ == "__main__":
    main()
