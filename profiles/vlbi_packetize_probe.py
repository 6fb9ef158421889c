"""BeamformVlbiOutput at config-4 size (96 channels, 32 beams, 960 samples per gulp): the packetiser kernel alone, 2 and 32
beams selected (run under `rocprofv3 --kernel-trace --stats` for its device time), and one gulp of the block end to end --
kernel, copy to pinned memory and send to a sink that only counts -- on a device ring that already holds every gulp, throttle
sleep switched off.  Prints one JSON line per measurement.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 profiles/vlbi_packetize_probe.py
"""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamformVlbiOutput  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests.pipeline_util import LOG, Source  # noqa: E402

NCHAN, NBEAM, NTIME, NINPUT = 96, 32, 960, 704


def kernel_loop(din, nsel, reps):
    stride = -(-(16 + 8 * NCHAN * nsel) // 16) * 16
    dout = ffi.DeviceBuffer(NTIME * stride)
    args = (din.ptr, dout.ptr, NCHAN, NBEAM, NTIME, 0, nsel, stride, 1, 1, max(nsel // 2, 1), 16, 0)
    for k in range(10):
        ffi.call("xengBeamformPacketizeVoltages", *args, k)
    ffi.call("xengBeamformSync")
    t0 = time.perf_counter()
    for k in range(reps):
        ffi.call("xengBeamformPacketizeVoltages", *args, k)
    ffi.call("xengBeamformSync")
    dt = (time.perf_counter() - t0) / reps
    print(json.dumps({"what": "kernel, back to back (host view)", "nbeam_selected": nsel, "us_per_call": dt * 1e6,
                      "bytes_moved": 2 * NCHAN * nsel * NTIME * 8}), flush=True)


def block_gulps(nbeam_send, ngulp):
    gulp = NCHAN * NBEAM * NTIME * 8
    data = np.random.default_rng(1).standard_normal(ngulp * gulp // 4).astype(np.float32)
    r = Ring("bf-output", space="cuda")
    r.resize(gulp, (ngulp + 1) * gulp)
    hdr = {'nchan': NCHAN, 'nbeam': NBEAM, 'npol': 1, 'nbit': 32, 'complex': True, 'seq0': 0, 'chan0': 0, 'system_nchan': 16 * NCHAN}
    counted = [0, 0]

    def sink(p):
        counted[0] += 1
        counted[1] += len(p)
    vl = BeamformVlbiOutput(LOG, r, ntime_gulp=NTIME, nbeam_send=nbeam_send, gpu=0, sink=sink)
    vl._sleep = lambda s: None
    gen = r.read(guarantee=True)            # (a reader registered before anything is written: every gulp stays for it)
    vl.iring = type("PreRead", (), {"read": lambda self, guarantee=True: gen, "span_memory_outlives_release": True})()
    src = Source(r, [(hdr, data, gulp)], wait_readers=1)
    src.start()
    src.join(120)
    th = threading.Thread(target=vl.main)
    t0 = time.perf_counter()
    th.start()
    th.join(120)
    dt = time.perf_counter() - t0
    assert counted[0] == ngulp * NTIME, counted
    print(json.dumps({"what": "block, per gulp end to end (kernel + copy + send to a counting sink)", "nbeam_send": nbeam_send,
                      "nbeam_selected": 2 * nbeam_send, "gulps": ngulp, "ms_per_gulp": dt / ngulp * 1e3,
                      "packet_bytes_per_gulp": counted[1] // ngulp}), flush=True)


def main():
    ffi.call("xengBeamformInitialize", 0, NINPUT, NCHAN, NTIME, NBEAM, 0)
    x = np.random.default_rng(0).standard_normal(NCHAN * NBEAM * NTIME * 2).astype(np.float32)
    din = ffi.DeviceBuffer(x.nbytes).upload(x)
    for nsel in (2, 32):
        kernel_loop(din, nsel, 200)
    for nbeam_send in (1, 16):
        block_gulps(nbeam_send, 16)
    ffi.call("xengBeamformDestroy")


if __name__ == "__main__":
    main()
