"""UpchanImageSearch (xengImsearchRun) at the all-sky size: 65 536 pixels, 24 channel groups, 64 DM trials, 5 boxcar widths, S = 128,
baseline blocks of 64 integrations.  WARM integrations first -- more than nstat + S, so that every delayed term and every boxcar is
live and nothing is left out by index -- then REPS integrations back to back over four images of noise in turn, ending in a
synchronise; one JSON line with the host view, the compulsory bytes of an integration (the image words read, one U row set
written, Z written, the T earlier Z rows read, the plane written) and their HBM floor, and a second line with the ndm * ngroup *
npix * 4 bytes of U re-reads if none of them hit a cache.  The state words the ingest kernel reads and writes (3 + 3 read, 3 written,
7 at a block's end) are given beside them: they are not compulsory in the sense above, a fused pass could keep them elsewhere.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/imsearch_probe.py

(a run of its own: no counters in it) then `python3 profiles/imsearch_probe.py --summarize OUT`: the median device time of the
timed launches of imsearch_ingest_kernel and imsearch_search_kernel, from the kernel trace."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPIX, NGROUP, NDM, NWIDTH, NSTAT, S = 65536, 24, 64, 5, 64, 128
WARM, REPS = 200, 100
HBM_TBS = 6.3                           # measured float4 copy (MI355X_MICROARCH.md: HBM3E)
T = (1 << (NWIDTH - 1)) - 1


def byte_counts():
    compulsory = NGROUP * 2 * NPIX * 4 + NGROUP * NPIX * 4 + NDM * NPIX * 4 + T * NDM * NPIX * 4 + NPIX * 8
    return compulsory, NDM * NGROUP * NPIX * 4, NGROUP * NPIX * 4 * 9


def run_point():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi

    rng = np.random.default_rng(0)
    imgs = []
    for _ in range(4):
        x = rng.normal(1000.0, 15.0, NGROUP * 4 * NPIX).astype(np.float32)
        imgs.append(ffi.DeviceBuffer(x.nbytes).upload(x))
    dout = ffi.DeviceBuffer(NPIX * 8)
    d = np.arange(NDM)[:, None] * (NGROUP - 1 - np.arange(NGROUP))[None, :]
    delays = np.ascontiguousarray(np.round(d * (S / d.max())).astype(np.int32))
    assert delays.max() == S
    ffi.call("xengImsearchInitialize", 0, NPIX, NGROUP, NDM, S, NWIDTH, NSTAT)
    ffi.call("xengImsearchSetDelays", delays.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    for k in range(WARM):
        ffi.call("xengImsearchRun", imgs[k % 4].ptr, dout.ptr)
    ffi.call("xengImsearchSync")
    t0 = time.perf_counter()
    for k in range(REPS):
        ffi.call("xengImsearchRun", imgs[k % 4].ptr, dout.ptr)
    ffi.call("xengImsearchSync")
    dt = (time.perf_counter() - t0) / REPS
    rec = dout.download(np.uint8).view(np.dtype([('snr', '<f4'), ('idm', '<i2'), ('iw', '<i2')]))
    compulsory, rereads, state = byte_counts()
    print(json.dumps({"what": "xengImsearchRun back to back (host view, ends in a synchronise)", "us_per_integration": dt * 1e6, "launches": 2 * (WARM + REPS),
                      "npix": NPIX, "ngroup": NGROUP, "ndm": NDM, "nwidth": NWIDTH, "nstat": NSTAT, "S": S, "scored_pixels": int((rec['idm'] >= 0).sum()),
                      "compulsory_bytes": compulsory, "hbm_floor_us": compulsory / (HBM_TBS * 1e12) * 1e6, "state_bytes_ingest": state}), flush=True)
    print(json.dumps({"what": "U re-reads of the search kernel if none hit a cache", "bytes": rereads, "hbm_us": rereads / (HBM_TBS * 1e12) * 1e6,
                      "floor_with_rereads_us": (compulsory + rereads) / (HBM_TBS * 1e12) * 1e6}), flush=True)
    ffi.call("xengImsearchDestroy")


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    compulsory, rereads, _ = byte_counts()
    total = 0.0
    for name in ("imsearch_ingest_kernel", "imsearch_search_kernel"):
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
        assert len(t) == WARM + REPS, "%d %s launches in the trace, %d expected" % (len(t), name, WARM + REPS)
        u = t[WARM:]
        total += float(np.median(u)) / 1e3
        print(json.dumps({"kernel": name, "median_us": float(np.median(u)) / 1e3, "min_us": min(u) / 1e3, "max_us": max(u) / 1e3, "launches": len(u)}))
    print(json.dumps({"both_kernels_median_us": total, "hbm_floor_us": compulsory / (HBM_TBS * 1e12) * 1e6,
                      "floor_with_rereads_us": (compulsory + rereads) / (HBM_TBS * 1e12) * 1e6,
                      "times_the_floor": total / (compulsory / (HBM_TBS * 1e12) * 1e6)}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_point()
