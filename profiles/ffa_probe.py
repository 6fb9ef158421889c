"""BeamFfaSearch (xengFfaRun) at the live size: 16 pairs x 256 DM trials = 4096 series, segments of NT = 2^14 samples (nds = 1),
nprod = 1, 4 octaves, base periods 256..512 and 8 boxcar widths.  WARM warm-up segments and then REPS segments are streamed, each
as NT / NWIN calls of NWIN = 1024 windows over the same span of noise, ending in a synchronise; one JSON line with the host view
and the LDS words a segment moves, counted: per (series, octave, base period) M * p words come in (one store), every one of the
log2 M fold stages reads two words and stores one per word, every boxcar width reads each word once for its score and, but for the
last, reads a second and stores one.

Device time: run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/ffa_probe.py

(a run of its own: no counters in it) then `python3 profiles/ffa_probe.py --summarize OUT`: the median device time of the timed
launches of each kernel from the kernel trace, the fold kernel per octave (its launches go round the octaves in order), and
their sum per segment."""
import ctypes
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NPAIR, NDM, NT, NWIN, NDS, NOCT, PMIN, PMAX, NWIDTH = 16, 256, 1 << 14, 1024, 1, 4, 256, 512, 8
WARM, REPS = 1, 3                                                       # segments


def lds_words():
    """LDS words read or written per series and segment, and the folded words times stages among them."""
    total = folded = 0
    for o in range(NOCT):
        for p in range(PMIN, PMAX + 1):
            lm = 1
            while p << (lm + 1) <= NT >> o:
                lm += 1
            w = p << lm
            total += w * (1 + 3 * lm + NWIDTH + 2 * (NWIDTH - 1))
            folded += w * lm
    return total, folded


def run_points():
    import caltech_bifrost_dsp_amd  # noqa: F401
    from caltech_bifrost_dsp_amd import ffi

    rng = np.random.default_rng(0)
    done = ctypes.c_int()
    nser = NPAIR * NDM
    x = rng.chisquare(4 * 3072, NWIN * nser).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    dout = ffi.DeviceBuffer(nser * NOCT * NWIDTH * 16)
    ffi.call("xengFfaInitialize", 0, NPAIR, NDM, NWIN, 1, NDS, NT, NOCT, PMIN, PMAX, NWIDTH)

    def segments(n):
        for _ in range(n * (NT * NDS // NWIN)):
            ffi.call("xengFfaRun", din.ptr, NWIN, dout.ptr, ctypes.byref(done))
        ffi.call("xengFfaSync")

    segments(WARM)
    t0 = time.perf_counter()
    segments(REPS)
    dt = (time.perf_counter() - t0) / REPS
    words, folded = lds_words()
    print(json.dumps({"what": "xengFfaRun, one segment of NT samples in calls of NWIN windows (host view, ends in a synchronise)", "ms_per_segment": dt * 1e3,
                      "segments": WARM + REPS, "npair": NPAIR, "ndm": NDM, "nt": NT, "nwin": NWIN, "nds": NDS, "noct": NOCT, "pmin": PMIN, "pmax": PMAX,
                      "nwidth": NWIDTH, "fold_work_groups": nser * NOCT * (PMAX - PMIN + 1), "lds_bytes_per_segment": 4 * words * nser,
                      "folded_word_stages_per_segment": folded * nser, "lds_words_per_folded_word_and_stage": words / folded}), flush=True)
    ffi.call("xengFfaDestroy")
    din.free()
    dout.free()


def summarize(out):
    import csv
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    total = 0.0
    for kernel, per_seg in (("ffa_ingest_kernel", NT * NDS // NWIN), ("ffa_prepare_kernel", 1), ("ffa_fold_kernel", NOCT), ("ffa_reduce_kernel", 1)):
        t = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if kernel in r["Kernel_Name"]]
        assert len(t) == (WARM + REPS) * per_seg, "%d %s launches in the trace, %d expected" % (len(t), kernel, (WARM + REPS) * per_seg)
        u = t[WARM * per_seg:]
        groups = {"octave %d" % o: u[o::NOCT] for o in range(NOCT)} if kernel == "ffa_fold_kernel" else {"all": u}
        for which, v in groups.items():
            print(json.dumps({"kernel": kernel, "launches": which, "median_us": float(np.median(v)) / 1e3, "min_us": min(v) / 1e3, "max_us": max(v) / 1e3,
                              "n": len(v)}))
        total += sum(u) / REPS
    words, _ = lds_words()
    print(json.dumps({"device_ms_per_segment": total / 1e6, "lds_bytes_per_segment": 4 * words * NPAIR * NDM,
                      "lds_TB_per_s": 4 * words * NPAIR * NDM / (total * 1e-9) / 1e12}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run_points()
