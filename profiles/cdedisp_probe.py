"""BeamCoherentDedisperse (xengCdedispRun) at the live size: 96 channels x 32 beams (16 pairs), gulps of 480 samples, NFFT 4096 with
an overlap of 1216 and NFFT 8192 with 2432.  Every point streams WARM warm-up blocks and then REPS blocks over the same gulp of
noise, ending in a synchronise; one JSON line per point with the host view and the bytes a block moves (the gulps' samples read and
written into the time buffer, the block read, its overlap written back, the output written, the table read once per pair).

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/cdedisp_probe.py

(a run of its own: no counters in it) then `python3 profiles/cdedisp_probe.py --summarize OUT`: the median device time of the timed
launches of cdedisp_ingest_kernel and cdedisp_filter_kernel at each point, from the kernel trace (the points run one after
another, so the launches split by count)."""
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
WARM, REPS = 4, 24                                                      # blocks
POINTS = [(4096, 1216), (8192, 2432)]                                   # (nfft, overlap), in launch order


def calls_for(nfft, overlap, nblk):
    """Calls of NTIME samples that complete exactly nblk blocks from a reset, and the ingest launches they make."""
    step, n, fill, calls, ingests, done = nfft - overlap, 0, 0, 0, 0, 0
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
        n += NTIME
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
    for nfft, overlap in POINTS:
        step, npair = nfft - overlap, NBEAM // 2
        table = chirp_table(40e6 + 23925.78125 * np.arange(NCHAN), 23925.78125, np.linspace(1.0, 10.0, npair) * nfft / 4096, nfft)
        ffi.call("xengCdedispInitialize", 0, NCHAN, NBEAM, NTIME, 0, npair, nfft, overlap)
        ffi.call("xengCdedispSetChirp", np.ascontiguousarray(table).view(np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        dout = ffi.DeviceBuffer(-(-NTIME // step) * NCHAN * NBEAM * step * 8)
        total, _ = calls_for(nfft, overlap, WARM + REPS)
        warm, _ = calls_for(nfft, overlap, WARM)

        def calls(n):
            for _ in range(n):
                ffi.call("xengCdedispRun", din.ptr, dout.ptr, ctypes.byref(nb))
            ffi.call("xengCdedispSync")

        calls(warm)
        t0 = time.perf_counter()
        calls(total - warm)
        dt = (time.perf_counter() - t0) / REPS
        nrow = NCHAN * NBEAM
        moved = nrow * (2 * step + nfft + overlap + step) * 8 + npair * NCHAN * nfft * 8
        print(json.dumps({"what": "xengCdedispRun, one block of nfft samples in calls of ntime (host view, ends in a synchronise)", "ms_per_block": dt * 1e3,
                          "blocks": WARM + REPS, "nchan": NCHAN, "nbeam": NBEAM, "ntime": NTIME, "nfft": nfft, "overlap": overlap, "work_groups": nrow,
                          "bytes_per_block": moved, "lds_bytes_per_block": nrow * (4 * -(-(nfft.bit_length() - 1) // 2) + 2) * nfft * 8}), flush=True)
        ffi.call("xengCdedispDestroy")
        dout.free()
    din.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("cdedisp_ingest_kernel", "cdedisp_filter_kernel"):
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
