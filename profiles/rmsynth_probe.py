"""BeamRmSynth (xengRmsynthRun) at the live shape: 16 pairs x 3072 channel groups x 1024 depths, at 256 and at 1024 bins, linear
feeds, every group used, the middle eighth of the bins on-pulse and the rest off-pulse.  Per shape WARM calls, then REPS calls timed
as one batch that ends in a synchronise; one JSON line per shape with the host view of a call.

Counted work: the contraction does 4 fmaf per (pair, group, bin, depth): 206 G at 1024 bins, 51.5 G at 256.  The fp32 vector rate
without packed instructions is half the guide's 157.3 TFLOPS (which counts v_pk_fma_f32 at 4 flops a lane and clock): 39.3 T fmaf
a second, so 5.2 ms at 1024 bins is the least the contraction can take.  Counted traffic of a 64 x 64 tile: per chunk of 8 groups
8 x 64 x 3 words of the cube (linear feeds) and 8 x 64 x 2 words of the table, 10 KiB for 8 x 64 x 64 x 4 = 131 k fmaf; over a
call every cube word is fetched nphi / 64 times and every table word nbin / 64 times per pair (L2 traffic after the first).  The
base and the profile kernels read the cube once each (805 MB at 1024 bins, 128 us at 6.3 TB/s).

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/rmsynth_probe.py

(a run of its own: no counters in it) then `python3 profiles/rmsynth_probe.py --summarize OUT`: the device time of the timed launches
of each kernel from the kernel trace, per shape in the order run."""
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NCHG, NPHI = 16, 3072, 1024
NBINS = (256, 1024)
WARM, REPS = 2, 5
KERNELS = ("rmsynth_base_kernel", "rmsynth_contract_kernel", "rmsynth_pick_kernel", "rmsynth_profile_kernel")
FMAF_PER_S = 157.3e12 / 4
HBM_BYTES_PER_S = 6.3e12


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.backend import HipBackend
    from caltech_bifrost_dsp_amd.blocks import RM_RECORD, rm_plan, rm_table

    freqs = 30e6 + (50e6 / NCHG) * (np.arange(NCHG) + 0.5)
    plan = rm_plan(freqs, 50e6 / NCHG, 1.0, 4)
    phis = plan['dphi'] * (np.arange(NPHI) - NPHI // 2)
    T, w, use, _ = rm_table(freqs, phis)
    be = HipBackend()
    rng = np.random.default_rng(0)
    for nbin in NBINS:
        one = rng.standard_normal((4, NCHG, nbin)).astype(np.float32)
        one[:2] = one[:2] ** 2 * 100.0
        din = ffi.DeviceBuffer(NPAIR * one.nbytes)
        for p in range(NPAIR):
            din.upload(one, p * one.nbytes)
        on = np.zeros((NPAIR, nbin), np.uint8)
        on[:, 7 * nbin // 16:9 * nbin // 16] = 1
        ffi.check("xengRmsynthInitialize", be.rmsynth_initialize(0, NPAIR, NCHG, nbin, NPHI, 0))
        ffi.check("xengRmsynthSetTable", be.rmsynth_set_table(T, w, use))
        ffi.check("xengRmsynthSetMasks", be.rmsynth_set_masks(np.ascontiguousarray(1 - on), on))
        nbytes = be.rmsynth_info()[4]
        dout = ffi.DeviceBuffer(nbytes)

        def calls(n):
            for _ in range(n):
                ffi.check("xengRmsynthRun", be.rmsynth_run(din, dout))
            be.rmsynth_sync()

        calls(WARM)
        t0 = time.perf_counter()
        calls(REPS)
        t_call = (time.perf_counter() - t0) / REPS
        rec = dout.download(np.uint8)[:16 * NPAIR].view(RM_RECORD)
        fmaf = 4 * NPAIR * NCHG * nbin * NPHI
        print(json.dumps(dict(npair=NPAIR, nchg=NCHG, nbin=nbin, nphi=NPHI, what="xengRmsynthRun, one call (host view, REPS calls and a synchronise)",
                              ms_per_call=t_call * 1e3, fmaf_per_call=fmaf, counted_ms_at_39_3_Tfmaf=fmaf / FMAF_PER_S * 1e3,
                              cube_mb=NPAIR * one.nbytes / 1e6, counted_us_one_cube_read_at_6_3TBs=NPAIR * one.nbytes / HBM_BYTES_PER_S * 1e6,
                              out_bytes=nbytes, k=rec['k'].tolist()[:2], guards=bool(be.rmsynth_guards_intact()))), flush=True)
        ffi.call("xengRmsynthDestroy")
        for b in (din, dout):
            b.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + REPS
    for kernel in KERNELS:
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        for i, nbin in enumerate(NBINS):
            u = t[i * per + WARM:(i + 1) * per]
            if not u:
                continue
            line = {"kernel": kernel, "nbin": nbin, "timed_launches": len(u), "median_us_per_launch": float(np.median(u)) / 1e3, "max_us_per_launch": max(u) / 1e3}
            if kernel == "rmsynth_contract_kernel":
                line["counted_us_at_39.3_Tfmaf"] = 4 * NPAIR * NCHG * nbin * NPHI / FMAF_PER_S * 1e6
            print(json.dumps(line))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
