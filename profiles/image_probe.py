"""UpchanImage's kernel (xengImage*, csrc/image_kernels.h) at the point of its issue: 704 inputs (352 stands) x 192 fine channels x
4096 pixels, nfavg 1 and 8.  Prints one JSON line per point: the host view of back-to-back runs ending in a synchronise, the FLOP
of the contract (8 ninput^2 per pixel and fine channel), what the MFMAs compute (three of the four polarisation blocks, stands
padded to the k loop's step and to whole column tiles) and the compute floor at the measured fp32-MFMA peak.  For the device time of
the kernel run it, in a run of its own, under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- timeout -k 10 300 python3 profiles/image_probe.py
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
from caltech_bifrost_dsp_amd.blocks.imaging import direction_list, pixel_grid, steering_delays  # noqa: E402

NSTAND, NFINE, SIDE = 352, 192, 72      # (72 x 72 pixel centres across the sky: 4060 above the horizon, padded to 4096 with patches)
NPIX = 4096
MFMA_TFS = 155.0        # fp32 MFMA, measured (MI355X_MICROARCH.md, Matrix cores)


def geometry(rng):
    l, m, n, mask = pixel_grid(SIDE, 180.0)
    lmn = direction_list(l, m, n, mask)
    assert len(lmn) <= NPIX
    extra = rng.uniform(-0.5, 0.5, (NPIX - len(lmn), 2))
    lmn = np.concatenate([lmn, np.concatenate([extra, np.sqrt(1 - (extra ** 2).sum(axis=1, keepdims=True))], axis=1)])
    r = 1200.0 * np.sqrt(rng.uniform(size=NSTAND))
    a = rng.uniform(0, 2 * np.pi, NSTAND)
    pos = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-5, 5, NSTAND)], axis=-1)
    return steering_delays(pos, lmn)


def point(bf, din, dout, tau, nfavg, reps):
    ninput = 2 * NSTAND
    ffi.check("xengImageInitialize", bf.image_initialize(0, NSTAND, NFINE, nfavg, NPIX))
    ffi.check("xengImageSetGeometry", bf.image_set_geometry(tau, np.ascontiguousarray(50e6 + 11962.890625 * np.arange(NFINE))))
    ngroup, tile, lds, norm = bf.image_info()

    def run(n):
        for _ in range(n):
            ffi.call("xengImageRun", din.ptr, dout.ptr)
        ffi.call("xengImageSync")
    run(1)
    t0 = time.perf_counter()
    run(reps)
    dt = time.perf_counter() - t0
    flop = 8.0 * ninput * ninput * NPIX * NFINE
    ktrips = (NSTAND + 7) // 8 * 8
    ntile = (NSTAND + 31) // 32
    flop_mfma = 12.0 * 4096 * (ktrips // 2) * ntile * ((NPIX + tile - 1) // tile) * NFINE
    print(json.dumps({"what": "xengImageRun x %d back to back (host view, ends in a synchronise)" % reps, "nstand": NSTAND, "nfine": NFINE, "nfavg": nfavg,
                      "npix": NPIX, "ngroup": ngroup, "pixel_tile": tile, "lds_bytes": lds, "ms_per_run_host": dt / reps * 1e3, "gflop_contract": flop / 1e9,
                      "gflop_mfma": flop_mfma / 1e9, "compute_floor_ms": flop / (MFMA_TFS * 1e12) * 1e3, "mfma_floor_ms": flop_mfma / (MFMA_TFS * 1e12) * 1e3,
                      "vis_bytes": float(din.nbytes), "reps": reps}), flush=True)
    ffi.call("xengImageDestroy")


def main():
    rng = np.random.default_rng(1)
    ninput = 2 * NSTAND
    bf = HipBackend()
    tau = geometry(rng)
    chan = ninput * ninput * 8
    din, dout = ffi.DeviceBuffer(NFINE * chan), ffi.DeviceBuffer(NFINE * 4 * NPIX * 4)
    for c in range(NFINE):              # (one random Hermitian-free channel, rolled: the kernel's time does not depend on the values)
        v = rng.standard_normal(2 * ninput * ninput).astype(np.float32) if c < 4 else v
        din.upload(np.roll(v, c), c * chan)
    for nfavg in (1, 8):
        point(bf, din, dout, tau, nfavg, 3)
    din.free()
    dout.free()


if __name__ == "__main__":
    main()
