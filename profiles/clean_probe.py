"""UpchanClean's kernel (xengClean*, csrc/clean_kernels.h) at the point of its issue: 352 stands (704 inputs) x 192 fine channels in
groups of 8 x 4096 pixels, niter 10 and 100.  Prints one JSON line per point: the host view of back-to-back Runs ending in a
synchronise, the host time of the enqueue alone (niter + 2 launches), and the work beside it -- npix * nstand * nfine phase factors
(one fp64 multiply, round and subtract, one sincospif and two fused multiply-adds each) per iteration.  The image is noise plus a few
bright pixels and nothing stops the loop early, so every Run does its niter iterations.  For the device time of the launches run it, in
a run of its own, under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- timeout -k 10 300 python3 profiles/clean_probe.py
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
from caltech_bifrost_dsp_amd.blocks.imaging import clean_components  # noqa: E402
from profiles.image_probe import NFINE, NPIX, NSTAND, geometry  # noqa: E402

NFAVG = 8


def point(bf, din, dout, niter, reps):
    ffi.check("xengCleanSetControl", bf.clean_set_control(niter, 0.1, 0.0, 0.0))
    ngroup, tile, comp_offset, stats_offset, span_bytes, norm = bf.clean_info()

    def run(n):
        t0 = time.perf_counter()
        for _ in range(n):
            ffi.call("xengCleanRun", din.ptr, dout.ptr)
        t1 = time.perf_counter()
        ffi.call("xengCleanSync")
        return t1 - t0
    run(1)
    t0 = time.perf_counter()
    enq = run(reps)
    dt = time.perf_counter() - t0
    comps, stats, _ = clean_components(dout.download(np.uint8)[:span_bytes], ngroup, niter, NPIX)
    factors = float(NPIX) * NSTAND * NFINE
    ms = dt / reps * 1e3
    print(json.dumps({"what": "xengCleanRun x %d back to back (host view, ends in a synchronise)" % reps, "nstand": NSTAND, "nfine": NFINE, "nfavg": NFAVG,
                      "npix": NPIX, "ngroup": ngroup, "pixel_tile": tile, "niter": niter, "launches_per_run": niter + 2, "ms_per_run_host": ms,
                      "ms_enqueue_per_run_host": enq / reps * 1e3, "ms_per_iteration": ms / max(niter, 1), "phase_factors_per_iteration": factors,
                      "gfactors_per_s": factors * niter / (ms * 1e-3) / 1e9, "ncomp_min": int(stats['ncomp'].min()), "reasons": sorted(set(stats['reason'].tolist())),
                      "span_bytes": span_bytes, "reps": reps}), flush=True)


def main():
    rng = np.random.default_rng(1)
    bf = HipBackend()
    tau = geometry(rng)
    ngroup = NFINE // NFAVG
    img = rng.standard_normal((ngroup, 4, NPIX)).astype(np.float32)
    img[:, :2, ::512] += 50.0                       # (a few bright pixels)
    ffi.check("xengCleanInitialize", bf.clean_initialize(0, NSTAND, NFINE, NFAVG, NPIX, 100))
    ffi.check("xengCleanSetGeometry", bf.clean_set_geometry(tau, np.ascontiguousarray(50e6 + 11962.890625 * np.arange(NFINE))))
    din = ffi.DeviceBuffer(img.nbytes).upload(img)
    dout = ffi.DeviceBuffer(ngroup * (16 * NPIX + 32 * 100 + 16))
    for niter in (10, 100):
        point(bf, din, dout, niter, 3)
    assert bf.clean_guards_intact()
    ffi.call("xengCleanDestroy")
    din.free()
    dout.free()


if __name__ == "__main__":
    main()
