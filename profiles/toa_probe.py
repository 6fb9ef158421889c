"""BeamToa (xengToaRun) at the live shape: 16 pairs x 3072 channel groups x 32 sub-bands x 4096 lags, at 256 and at 1024 bins, at
nprod 1 and 4, every group used, the middle eighth of the bins left out of the off-pulse mask.  The harmonics are min(512,
(nbin - 1) / 2): 127 at 256 bins and 511 at 1024 (the library takes no harmonic at or above Nyquist).  Per shape WARM calls, then
REPS calls timed as one batch that ends in a synchronise; one JSON line per shape with the host view of a call.

Counted work.  The scrunch reads the planes it needs once: npair nprod' nchg nbin 4 bytes with nprod' = 1 or 2 (201 or 402 MB at
1024 bins), 32 or 64 us at 6.3 TB/s.  The DFT does 2 fmaf per (row, harmonic, bin) and the correlation 2 per (row, harmonic, lag),
rows = npair (nsub + 1) = 528: 553 M and 2.2 G at 1024 bins.  The fp32 vector rate without packed instructions is half the guide's
157.3 TFLOPS (which counts v_pk_fma_f32 at 4 flops a lane and clock): 39.3 T fmaf a second, 14 and 56 us.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/toa_probe.py

(a run of its own: no counters in it) then `python3 profiles/toa_probe.py --summarize OUT`: the device time of the timed launches
of each kernel from the kernel trace, per shape in the order run."""
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NCHG, NSUB, NLAG = 16, 3072, 32, 4096
SHAPES = ((256, 1), (256, 4), (1024, 1), (1024, 4))       # (nbin, nprod)
WARM, REPS = 2, 5
KERNELS = ("toa_scrunch_kernel", "toa_band_kernel", "toa_base_kernel", "toa_dft_kernel", "toa_corr_kernel", "toa_pick_kernel")
FMAF_PER_S = 157.3e12 / 4
HBM_BYTES_PER_S = 6.3e12


def nharm_of(nbin):
    return min(512, (nbin - 1) // 2)


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.backend import HipBackend
    from caltech_bifrost_dsp_amd.blocks import TOA_RECORD, toa_subbands, toa_tables, toa_template

    be = HipBackend()
    rng = np.random.default_rng(0)
    for nbin, nprod in SHAPES:
        nharm = nharm_of(nbin)
        d = (np.arange(nbin) - 0.4 * nbin + nbin / 2.0) % nbin - nbin / 2.0
        shape = np.exp(-0.5 * (d / (nbin / 50.0)) ** 2)
        one = rng.standard_normal((nprod, NCHG, nbin)).astype(np.float32)
        one[:2] = one[:2] ** 2 + 5.0 * np.roll(shape, 7)[None, None, :]
        din = ffi.DeviceBuffer(NPAIR * one.nbytes)
        for p in range(NPAIR):
            din.upload(one, p * one.nbytes)
        off = np.ones((NPAIR, nbin), np.uint8)
        off[:, 7 * nbin // 16:9 * nbin // 16] = 0
        ffi.check("xengToaInitialize", be.toa_initialize(0, NPAIR, nprod, NCHG, nbin, NSUB, nharm, NLAG))
        ffi.check("xengToaSetBands", be.toa_set_bands(toa_subbands(NCHG, NSUB), None))
        ffi.check("xengToaSetTables", be.toa_set_tables(*toa_tables(nbin, nharm, NLAG)))
        ffi.check("xengToaSetTemplate", be.toa_set_template(toa_template(np.tile(shape, (NPAIR, 1)), nharm, NSUB)))
        ffi.check("xengToaSetMask", be.toa_set_mask(off))
        nbytes = be.toa_info()[5]
        dout = ffi.DeviceBuffer(nbytes)

        def calls(n):
            for _ in range(n):
                ffi.check("xengToaRun", be.toa_run(din, dout))
            be.toa_sync()

        calls(WARM)
        t0 = time.perf_counter()
        calls(REPS)
        t_call = (time.perf_counter() - t0) / REPS
        nrow = NPAIR * (NSUB + 1)
        rec = dout.download(np.uint8)[:16 * nrow].view(TOA_RECORD)
        read = NPAIR * min(nprod, 2) * NCHG * nbin * 4
        print(json.dumps(dict(npair=NPAIR, nprod=nprod, nchg=NCHG, nbin=nbin, nsub=NSUB, nharm=nharm, nlag=NLAG,
                              what="xengToaRun, one call (host view, REPS calls and a synchronise)", ms_per_call=t_call * 1e3,
                              cube_mb_read=read / 1e6, counted_us_scrunch_at_6_3TBs=read / HBM_BYTES_PER_S * 1e6,
                              counted_us_dft_at_39_3_Tfmaf=2 * nrow * nharm * nbin / FMAF_PER_S * 1e6,
                              counted_us_corr_at_39_3_Tfmaf=2 * nrow * nharm * NLAG / FMAF_PER_S * 1e6, out_bytes=nbytes, l=rec['l'].tolist()[:3],
                              guards=bool(be.toa_guards_intact()))), flush=True)
        ffi.call("xengToaDestroy")
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
        for i, (nbin, nprod) in enumerate(SHAPES):
            u = t[i * per + WARM:(i + 1) * per]
            if not u:
                continue
            nrow, nharm = NPAIR * (NSUB + 1), nharm_of(nbin)
            line = {"kernel": kernel, "nbin": nbin, "nprod": nprod, "timed_launches": len(u), "median_us_per_launch": float(np.median(u)) / 1e3,
                    "max_us_per_launch": max(u) / 1e3}
            if kernel == "toa_scrunch_kernel":
                line["counted_us_at_6.3_TBs"] = NPAIR * min(nprod, 2) * NCHG * nbin * 4 / HBM_BYTES_PER_S * 1e6
            if kernel == "toa_dft_kernel":
                line["counted_us_at_39.3_Tfmaf"] = 2 * nrow * nharm * nbin / FMAF_PER_S * 1e6
            if kernel == "toa_corr_kernel":
                line["counted_us_at_39.3_Tfmaf"] = 2 * nrow * nharm * NLAG / FMAF_PER_S * 1e6
            print(json.dumps(line))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
