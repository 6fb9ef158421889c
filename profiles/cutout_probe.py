"""BeamPulseCutout (xengCutoutRun) at the live shape: 16 pairs x 3072 fine channels, calls of NWIN = 30 windows, a fine grid of NDMF
trials whose largest delay is S = 107 windows, nband 64, nt 256 x tscr 4 (ntu = 1024 windows), ndmc 64, 8 widths, and a history of
ntu + S + 2 NWIN - 1 windows.  WARM warm-up calls fill the history; then REPS calls that serve nothing (the ingest alone) and REPS
calls that serve one request each are timed, each batch ending in a synchronise; one JSON line with the host view of both.

Counted traffic: the ingest reads the span (nwin npair nfine 16 bytes) and writes a quarter of it into the ring -- the bytes
dedisp_ingest_kernel<1> moves in xengDedispRun at the same shape: it is the same kernel (profiles/dedisp_probe.py times it; read the
two side by side from one run).  A served request reads, per row, ntu + S windows of nfine channels of one pair at most (4.2 MB of
history for 64 rows that overlap: L2 traffic after the first row), nfine delays per row, and writes (nband + ndmc) nt words; its
work is ndmc ntu nfine fused multiply-adds (201 M).

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/cutout_probe.py

(a run of its own: no counters in it) then `python3 profiles/cutout_probe.py --summarize OUT`: the device time of the timed launches
of each kernel from the kernel trace, beside the duration of one 30-window span at TSAMP."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NFINE, NWIN, NDMF, S = 16, 3072, 30, 256, 107
NBAND, NT, TSCR, NDMC, NWIDTH, NREQ = 64, 256, 4, 64, 8, 4
NTU = NT * TSCR
NHIST = NTU + S + 2 * NWIN - 1
WARM, REPS = 45, 100
TSAMP = 1.31072e-3                                                      # s: 8192 samples of 6.25 MHz a window, the live header's
KERNELS = ("dedisp_ingest_kernel", "cutout_partials_kernel", "cutout_score_kernel", "cutout_pick_kernel")
SPAN_BYTES = NWIN * NPAIR * NFINE * 16
HBM_BYTES_PER_S = 6.3e12


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi
    from caltech_bifrost_dsp_amd.backend import HipBackend
    from caltech_bifrost_dsp_amd.blocks import CUTOUT_RECORD, CUTOUT_REQUEST, cutout_k_mad

    rng = np.random.default_rng(0)
    x = ((rng.standard_normal((NWIN, NPAIR, NFINE, 4)) ** 2) * 100.0).astype(np.float32)
    d = np.arange(NDMF)[:, None] / float(NDMF - 1)
    u = (NFINE - 1 - np.arange(NFINE))[None, :] / float(NFINE - 1)
    delays = np.ascontiguousarray(np.rint(S * d * u * u), np.int32)
    be = HipBackend()
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    ffi.check("xengCutoutInitialize", be.cutout_initialize(0, NPAIR, NFINE, NWIN, NDMF, NHIST, NBAND, NT, TSCR, NDMC, NWIDTH, NREQ, cutout_k_mad()))
    ffi.check("xengCutoutSetDelays", be.cutout_set_delays(delays))
    nbytes = be.cutout_info()[2]
    dout = ffi.DeviceBuffer(nbytes)

    def calls(n, serve):
        nserved = 0
        for _ in range(n):
            if serve:
                # the request whose last window is the last of the call to come (centre trial NDMF - 1 - NDMC / 2: the largest delays)
                end = be.cutout_info()[0] + NWIN
                ic = NDMF - 1 - NDMC // 2
                n_c = end - 1 - int(delays[min(NDMF - 1, ic + (NDMC - 1 - NDMC // 2))].max()) - (NTU - 1) + NTU // 2
                ffi.check("xengCutoutRequest", be.cutout_request(np.array([(nserved, 3, n_c, ic, 1)], CUTOUT_REQUEST)))
            rv, served, expired = be.cutout_run(din, NWIN, dout, NREQ)
            ffi.check("xengCutoutRun", rv)
            assert not expired and len(served) == int(serve)
            nserved += len(served)
        be.cutout_sync()
        return nserved

    calls(WARM, False)
    t0 = time.perf_counter()
    calls(REPS, False)
    t_ingest = (time.perf_counter() - t0) / REPS
    t0 = time.perf_counter()
    nserved = calls(REPS, True)
    t_serve = (time.perf_counter() - t0) / REPS
    rec = dout.download(np.uint8)[:32 * NREQ].view(CUTOUT_RECORD)
    print(json.dumps(dict(npair=NPAIR, nfine=NFINE, nwin=NWIN, ndmf=NDMF, S=S, nband=NBAND, nt=NT, tscr=TSCR, ndmc=NDMC, nhist=NHIST,
                          what="xengCutoutRun, one call of NWIN windows (host view, REPS calls and a synchronise)", us_per_ingest_call=t_ingest * 1e6,
                          us_per_serving_call=t_serve * 1e6, served=nserved, span_us_at_tsamp=NWIN * TSAMP * 1e6, counted_mb_per_ingest=1.25 * SPAN_BYTES / 1e6,
                          fma_per_request=NDMC * NTU * NFINE, out_bytes=nbytes, last_status=int(rec[0]['status']), last_S=float(rec[0]['S']))), flush=True)
    ffi.call("xengCutoutDestroy")
    for b in (din, dout):
        b.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel in KERNELS:
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        if not t:
            continue
        u = t[WARM:] if kernel == "dedisp_ingest_kernel" else t
        line = {"kernel": kernel, "launches": len(t), "timed_launches": len(u), "median_us_per_launch": float(np.median(u)) / 1e3, "max_us_per_launch": max(u) / 1e3,
                "span_us_at_tsamp": NWIN * TSAMP * 1e6}
        if kernel == "dedisp_ingest_kernel":
            line["counted_us_at_6.3TBs"] = 1.25 * SPAN_BYTES / HBM_BYTES_PER_S * 1e6
        print(json.dumps(line))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
