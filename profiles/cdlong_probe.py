"""BeamCoherentDedisperseLong (xengCdlongRun) at the live size: 96 channels x 32 beams (16 pairs), gulps of 480 samples, NFFT 2^15
with an overlap of 8908 (20 MHz at DM 10) and NFFT 2^17 with 40000.  Every point streams WARM warm-up blocks and then REPS blocks
over the same gulp of noise, ending in a synchronise; one JSON line per point with the host view and the bytes a block moves
(cdlong_kernels.h: 8.5 NFFT - M words of 8 bytes per row, the table counted once per pair).  The state at 2^17 is 8 GB.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/cdlong_probe.py

(a run of its own: no counters in it) then `python3 profiles/cdlong_probe.py --summarize OUT`: the median device time of the timed
launches of each kernel at each point, from the kernel trace (the points run one after another, so the launches split by count).

Per-launch times on the MI355X: DESIGN.md 4.30, "Bound versus measured" (one trace run; 10.8 ms of device time per block at 2^17,
more than half of it in cdlong_rows_kernel)."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCHAN, NBEAM, NTIME = 96, 32, 480
WARM, REPS = 2, 8                                                       # blocks
POINTS = [(1 << 15, 8908), (1 << 17, 40000)]                            # (nfft, overlap), in launch order
PER_BLOCK = ("cdlong_cols_fwd_kernel", "cdlong_tail_kernel", "cdlong_rows_kernel", "cdlong_cols_inv_kernel")


def calls_for(nfft, overlap, nblk):
    """Calls of NTIME samples that complete exactly nblk blocks from a reset, and the ingest launches they make."""
    fill, calls, ingests, done = 0, 0, 0, 0
    while done < nblk:
        calls += 1
        t = 0
        while t < NTIME:
            k = min(NTIME - t, nfft - fill)
            ingests += 1
            t += k
            fill += k
            if fill == nfft:
                done += 1
                fill = overlap
    assert done == nblk, "the last call completed more than one block: choose other counts"
    return calls, ingests


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.blocks import chirp_table

    rng = np.random.default_rng(0)
    nb = ctypes.c_int()
    x = (rng.standard_normal((NCHAN, NBEAM, NTIME)) + 1j * rng.standard_normal((NCHAN, NBEAM, NTIME))).astype(np.complex64)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    freqs = 20e6 + 23925.78125 * np.arange(NCHAN)
    for nfft, overlap in POINTS:
        step, npair = nfft - overlap, NBEAM // 2
        ffi.call("xengCdlongInitialize", 0, NCHAN, NBEAM, NTIME, 0, npair, nfft, overlap)
        for p, dm in enumerate(np.linspace(1.0, 10.0, npair) * nfft / (1 << 15)):
            table = np.ascontiguousarray(chirp_table(freqs, 23925.78125, [dm], nfft)[0])
            ffi.call("xengCdlongSetChirp", p, table.view(np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        dout = ffi.DeviceBuffer(-(-NTIME // step) * NCHAN * NBEAM * step * 8)
        total, _ = calls_for(nfft, overlap, WARM + REPS)
        warm, _ = calls_for(nfft, overlap, WARM)

        def calls(n):
            for _ in range(n):
                ffi.call("xengCdlongRun", din.ptr, dout.ptr, ctypes.byref(nb))
            ffi.call("xengCdlongSync")

        calls(warm)
        t0 = time.perf_counter()
        calls(total - warm)
        dt = (time.perf_counter() - t0) / REPS
        nrow = NCHAN * NBEAM
        moved = nrow * (8 * nfft - overlap) * 8 + npair * NCHAN * nfft * 8
        print(json.dumps({"what": "xengCdlongRun, one block of nfft samples in calls of ntime (host view, ends in a synchronise)", "ms_per_block": dt * 1e3,
                          "blocks": WARM + REPS, "nchan": NCHAN, "nbeam": NBEAM, "ntime": NTIME, "nfft": nfft, "overlap": overlap, "rows": nrow,
                          "bytes_per_block": moved}), flush=True)
        ffi.call("xengCdlongDestroy")
        dout.free()
    din.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("cdlong_ingest_kernel",) + PER_BLOCK:
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        at = 0
        for nfft, overlap in POINTS:
            _, ing_all = calls_for(nfft, overlap, WARM + REPS)
            _, ing_warm = calls_for(nfft, overlap, WARM)
            n_all, n_warm = (ing_all, ing_warm) if "ingest" in kernel else (WARM + REPS, WARM)
            u = t[at + n_warm:at + n_all]
            at += n_all
            print(json.dumps({"kernel": kernel, "nfft": nfft, "overlap": overlap, "median_us": float(np.median(u)) / 1e3, "min_us": min(u) / 1e3,
                              "max_us": max(u) / 1e3, "n": len(u)}))
        assert at == len(t), "%d %s launches in the trace, %d expected" % (len(t), kernel, at)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
