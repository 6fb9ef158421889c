"""The object the blocks call where the reference calls `_bf` / `bifrost.device` / `bifrost.map`.

`HipBackend` forwards to libxeng.so (include/xeng.h) and is the only backend the product ships:
constructing it without the HIP library or without a GPU raises.  Tests may inject a different
object with the same methods (tests/fake_backend.py wraps the CPU oracle) to exercise the block
state machines without a GPU -- that is test infrastructure, never a fallback.
"""
import ctypes

import numpy as np

from . import ffi


def _dev(a):
    """Device address behind an `as_BFarray()` reference (or a plain ctypes pointer to an XENGarray)."""
    d = getattr(a, "data", None)
    return d if d is not None else a.contents.data


def _host_floats(a):
    """float* to a host float32 array (kept alive by the caller for the call), or NULL for None."""
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _host_array(who, what, a, dtype):
    """What the setters of host tables ask of an argument before they hand its address to the library: a C-contiguous numpy
    array of `dtype`.  `who` is the calling method, `what` names the argument in the TypeError."""
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags['C_CONTIGUOUS']):
        raise TypeError("%s: %s must be a C-contiguous %s array" % (who, what, np.dtype(dtype).name))
    return a


class HipBackend:
    BF_STATUS_SUCCESS = ffi.STATUS_SUCCESS
    space_in = "cuda"          # memory space the compute entry points expect

    def __init__(self):
        self._lib = ffi.lib()   # raises ImportError if libxeng.so has not been built
        self._enq = ffi.enqueue_lib()   # enqueue-only calls, made without giving up the interpreter lock (ffi.ENQUEUE_ONLY)
        # ... and the ones a block makes per gulp bound directly (csrc/pyext/xfast.cpp): ctypes spends more on converting
        # their arguments than the library spends on the call
        from .ring import _xfast
        self._x = _xfast()

    # ---- device plumbing (bifrost.device.set_device / get_device / stream_synchronize)
    def set_device(self, gpu):
        ffi.call("xengSetDevice", int(gpu))

    def get_device(self):
        import ctypes
        g = ctypes.c_int()
        ffi.call("xengGetDevice", ctypes.byref(g))
        return g.value

    def stream_synchronize(self):
        """Every library stream of the device (bifrost.device.stream_synchronize has one stream to wait for; here each
        block works on its own, so the blocks use the per-stream waits below and leave the others running)."""
        ffi.call("xengStreamSynchronize")

    def map_sync(self):
        """CorrAcc's stream (corr_acc_block.py:317)."""
        ffi.call("xengMapSync")

    def beam_sync(self):
        """The beamformer's stream: Beamform / BeamformSumBeams (beamform_block.py:450, beamform_sum_beams_block.py:247)."""
        ffi.call("xengBeamformSync")

    def beam_mark(self):
        """Ticket for everything enqueued on the beamformer's stream so far (beam_wait waits for it)."""
        t = self._x.beam_mark()
        if t < 0:
            ffi.check("xengBeamformMark", -t)
        return t

    def beam_wait(self, ticket):
        # ask first, without giving up the interpreter lock; only a ticket the GPU has not reached yet is worth a blocking call
        d = self._x.beam_ticket_done(ticket)
        if d < 0:
            ffi.check("xengBeamformTicketDone", -d)
        if not d:
            ffi.call("xengBeamformWait", ticket)

    # ---- X-engine (corr_block.py:253,331,445)
    def xgpu_configure(self, nstand, npol, nchan, ntime_gulp, max_gulps=0):
        """xGPU's compile-time NSTATION/NFREQUENCY/NTIME (install_xgpu.sh:5) are runtime here."""
        return self._lib.xengXgpuConfigure(nstand, npol, nchan, ntime_gulp, max_gulps)

    def bfXgpuInitialize(self, in_arr, out_arr, gpu):
        return self._lib.bfXgpuInitialize(in_arr, out_arr, int(gpu))

    def bfXgpuKernel(self, in_arr, out_arr, do_dump):
        return self._lib.bfXgpuKernel(in_arr, out_arr, int(do_dump))

    def bfXgpuKernelAsync(self, in_arr, out_arr, do_dump):
        """Enqueue only: the gulp is read in place at dump time, so the caller keeps it alive and unchanged until
        xgpu_sync() (include/xeng.h: xengXgpuKernelAsync).  No reference counterpart."""
        return self._x.xgpu_kernel_async(_dev(in_arr), _dev(out_arr), int(do_dump))

    def bfXgpuKernelAsyncAcc(self, in_arr, out_arr, do_dump, acc, acc_mode):
        """bfXgpuKernelAsync whose dump also assigns (acc_mode 1) / adds (2) every stored word to the long accumulator
        `acc` -- CorrAcc's "a = b" / "a += b" (corr_acc_block.py:304-306) done by the contraction's epilogue."""
        return self._x.xgpu_kernel_async_acc(_dev(in_arr), _dev(out_arr), int(do_dump), acc.ptr, int(acc_mode))

    def bfXgpuKernelSlab(self, slab, npkt, pkt_stride, seq0, chan0, out_arr, do_dump, acc=None, acc_mode=0):
        """bfXgpuKernelAsync[Acc] on a gulp handed over as the slab of SNAP2 packets it arrived in (include/xeng.h
        xengXgpuKernelAsyncSlab): read in place when the slab is complete and in order, scattered on the device otherwise.
        No reference counterpart: bifrost's capture scatters on the CPU (capture_block.py:221-305)."""
        return self._x.xgpu_kernel_slab(slab.ptr, int(npkt), int(pkt_stride), int(seq0), int(chan0), _dev(out_arr), int(do_dump),
                                        acc.ptr if acc is not None else 0, int(acc_mode))

    def xgpu_fused_acc_supported(self):
        """True when the live X-engine context runs the default (fused corner turn) contraction kernel, the one whose
        epilogue can feed a long accumulator; other gulp shapes take the two-pass path and CorrAcc keeps its map."""
        import ctypes
        fused, fp6 = ctypes.c_int(), ctypes.c_int()
        rc = self._lib.xengXgpuGetPath(ctypes.byref(fused), ctypes.byref(fp6))
        return rc == ffi.STATUS_SUCCESS and fused.value == 1 and fp6.value == 0

    def xgpu_sync(self):
        return self._lib.xengXgpuSync()

    def xgpu_sync_lag(self, lag):
        """Wait until the dump issued `lag` dumps before the latest one is complete (lag 0 = the latest)."""
        d = self._x.xgpu_dump_done(int(lag))       # (asked without giving up the interpreter lock)
        if d:
            return ffi.STATUS_SUCCESS if d > 0 else -d
        return self._lib.xengXgpuSyncLag(int(lag))

    def bfXgpuGetOrder(self, antpol_to_input, antpol_to_bl, is_conj):
        return self._lib.bfXgpuGetOrder(antpol_to_input, antpol_to_bl, is_conj)

    def bfXgpuSubSelect(self, in_arr, out_arr, vismap, conj, nchan_sum, unused=0):
        return self._lib.bfXgpuSubSelect(in_arr, out_arr, vismap, conj, int(nchan_sum), int(unused))

    def xgpu_packetize(self, in_arr, out_arr, antpol_to_bl, is_conj, fmt):
        """Device reorder + per-baseline payloads of CorrOutputFull (corr_output_full_block.py:669, 461-467, 512-519)."""
        return self._lib.xengXgpuPacketize(in_arr.ptr, out_arr.ptr, antpol_to_bl.ptr, is_conj.ptr, int(fmt))

    def xgpu_reset(self):
        """Drop staged gulps / partial sums of an aborted integration (no reference counterpart)."""
        return self._lib.xengXgpuReset()

    # ---- ingest: SNAP2 packets -> gulp (the scatter bifrost's UDP capture does on the CPU; capture_block.py:296-305)
    def snap2_unpack(self, packets, npkt, pkt_stride, out, seq0, ntime, chan0, nchan_tot, npol_tot, clear=True):
        """Returns (status, packets placed, packets dropped)."""
        import ctypes
        placed, dropped = ctypes.c_int(), ctypes.c_int()
        rc = self._lib.xengSnap2Unpack(packets.ptr, int(npkt), int(pkt_stride), out.ptr, int(seq0), int(ntime), int(chan0),
                                       int(nchan_tot), int(npol_tot), int(bool(clear)), ctypes.byref(placed), ctypes.byref(dropped))
        return rc, placed.value, dropped.value

    # ---- CorrAcc (corr_acc_block.py:304,306: BFMap "a = b" / "a += b")
    def map_assign_i32(self, a, b):
        return self._x.map_i32(a.ptr, b.ptr, a.nbytes // 4, False)

    def map_add_i32(self, a, b):
        return self._x.map_i32(a.ptr, b.ptr, a.nbytes // 4, True)

    def map_sum_i32(self, a, srcs, add):
        """a = (add ? a : 0) + srcs[0] + ... + srcs[-1] in one pass (include/xeng.h xengMapSumI32): the long accumulation of a
        GROUP of dumps, their spans read once each.  Enqueued on the map stream like the two calls above; the caller may let go of
        the source spans at once on in-repo rings (released memory is reissued only behind its stamp)."""
        n = len(srcs)
        arr = (ctypes.c_void_p * n)(*[x.ptr for x in srcs])
        return self._enq.xengMapSumI32(a.ptr, arr, n, a.nbytes // 4, int(bool(add)))

    # ---- a copy that is only enqueued (CorrAcc's publish of a long integration: 383 MB over PCIe, 7 ms)
    def copy_async(self, dst, src):
        """Enqueue dst <- src on the library's copy stream; returns the stamp that completes when the copy has (copy_done /
        copy_wait).  The caller keeps both arrays alive and unchanged until then."""
        assert dst.nbytes == src.nbytes
        return self._x.copy_async(dst.ptr, src.ptr, dst.nbytes)

    def copy_done(self, stamp):
        return self._x.stamp_done(stamp)

    def copy_wait(self, stamp):
        self._x.stamp_wait(stamp)

    # ---- beamformer (beamform_block.py:251,449; beamform_sum_beams_block.py:245)
    _beam_row_bytes = 0

    def bfBeamformInitialize(self, gpu, ninput, nchan, ntime, nbeam, ntime_blocks):
        self._beam_row_bytes = int(ninput) * int(nchan)         # bytes per sample of a gulp (4+4 bit per input)
        return self._lib.bfBeamformInitialize(int(gpu), ninput, nchan, ntime, nbeam, ntime_blocks)

    def bfBeamformRun(self, in_arr, out_arr, weights, version=0):
        """`version` != 0 lets the library reuse its bf16-split copy of the weights while the caller has
        not changed them (the reference call shape has no such argument: version 0 = always re-split)."""
        if version:
            return self._x.beam_run(_dev(in_arr), _dev(out_arr), _dev(weights), int(version))
        return self._lib.bfBeamformRun(in_arr, out_arr, weights)

    def bfBeamformRunParts(self, part0, part1, out_arr, weights, version=0):
        """One beamformer gulp out of two consecutive spans of the input ring (arrays `part0`, `part1`: whole samples each),
        one launch, no gathered copy (include/xeng.h xengBeamformRunParts).  No reference counterpart: bifrost's circular ring
        hands the reference's 2-gulp read (lwa352-pipeline.py:172,279-282) out contiguously."""
        ntime0 = part0.nbytes // (self._beam_row_bytes or 1)
        return self._x.beam_run_parts(part0.ptr, ntime0, part1.ptr, _dev(out_arr), _dev(weights), int(version))

    def bfBeamformRunSlabs(self, slab0, npkt0, ntime0, slab1, npkt1, pkt_stride, seq0, chan0, out_arr, weights, version=0):
        """bfBeamformRun on a gulp handed over as one (slab1 None) or two consecutive slabs of SNAP2 packets (include/xeng.h
        xengBeamformRunSlabs)."""
        return self._x.beam_run_slabs(slab0.ptr, int(npkt0), int(ntime0), slab1.ptr if slab1 is not None else 0, int(npkt1), int(pkt_stride),
                                      int(seq0), int(chan0), _dev(out_arr), _dev(weights), int(version))

    def beam_pump(self, iring, reader, oring, oseq_id, igulp, ogulp, mode, row_bytes=0, ntime_sum=0, depth=8, staged=False):
        """The steady-state per-gulp loop of Beamform (mode 0) / BeamformSumBeams (mode 1) between two NATIVE rings as an object
        whose run() works without the interpreter lock (csrc/pyext/xfast.cpp BeamPump); None when the rings are not native
        or XENG_PUMP=0."""
        import os
        if os.environ.get("XENG_PUMP") == "0" or not (hasattr(iring, "_h") and hasattr(oring, "_h")):
            return None
        return self._x.beam_pump(iring, iring._h, int(reader), oring, oring._h, int(oseq_id), int(igulp), int(ogulp), int(mode), int(row_bytes),
                                 int(ntime_sum), int(depth), int(bool(staged)))

    def corr_pump(self, iring, reader, oring, igulp, ogulp, ntime_gulp):
        """The per-gulp loop of Corr while it integrates, between two NATIVE rings, as an object whose run() works without the
        interpreter lock (csrc/pyext/xfast.cpp CorrPump); None when the rings are not native or XENG_PUMP=0."""
        import os
        if os.environ.get("XENG_PUMP") == "0" or not (hasattr(iring, "_h") and hasattr(oring, "_h")):
            return None
        return self._x.corr_pump(iring, iring._h, int(reader), oring, oring._h, int(igulp), int(ogulp), int(ntime_gulp))

    def bfBeamformIntegrate(self, in_arr, out_arr, ntime_sum):
        # (bfBeamformIntegrate reads only the two data pointers from its structs: the raw entry point, no structs built per gulp)
        return self._x.beam_integrate(_dev(in_arr), _dev(out_arr), int(ntime_sum))

    def beam_packetize_voltages(self, in_arr, out_arr, nchan, nbeam, ntime, beam0, nbeam_pkt, pkt_stride, server, gbe, nbeam_hdr, nserver,
                                chan0, seq0):
        """BeamformVlbiOutput's gulp -> "ibeam" packets on the beamformer's stream (include/xeng.h xengBeamformPacketizeVoltages;
        beamform_vlbi_output_block.py:258-276 does it on the host).  Enqueue only: beam_mark / beam_wait cover it."""
        return self._enq.xengBeamformPacketizeVoltages(in_arr.ptr, out_arr.ptr, int(nchan), int(nbeam), int(ntime), int(beam0), int(nbeam_pkt),
                                                       int(pkt_stride), int(server), int(gbe), int(nbeam_hdr), int(nserver), int(chan0), int(seq0))

    # ---- upchannelising beamformer (UpchanBeamform; include/xeng.h "Upchannelising beamformer"): a context of its own, its
    # kernel on the beamformer's stream
    def upchan_initialize(self, gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum):
        return self._lib.xengUpchanInitialize(int(gpu), int(ninput), int(nchan), int(ntime), int(nupchan), int(nbeam), int(nframe_sum))

    def upchan_initialize_dual_pol(self, gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum):
        """The same context in dual-pol mode: beams 2p / 2p+1 are X / Y, and each run writes [XX, YY, Re(XY*), Im(XY*)] per pair
        and window (include/xeng.h xengUpchanInitializeDualPol); run, mark, wait and sync are the calls above."""
        return self._lib.xengUpchanInitializeDualPol(int(gpu), int(ninput), int(nchan), int(ntime), int(nupchan), int(nbeam), int(nframe_sum))

    def upchan_run(self, in_arr, out_arr, weights, version=0):
        """Enqueue only: upchan_mark / upchan_wait cover it."""
        return self._enq.xengUpchanRun(in_arr.ptr, out_arr.ptr, weights.ptr, int(version))

    def upchan_run_parts(self, part0, ntime0, part1, out_arr, weights, version=0):
        """One gulp out of two consecutive spans of the input ring (samples [0, ntime0) in part0), one launch, no gathered copy."""
        return self._enq.xengUpchanRunParts(part0.ptr, int(ntime0), part1.ptr, out_arr.ptr, weights.ptr, int(version))

    def upchan_set_pfb(self, ntap, coeffs):
        """The PFB front end (include/xeng.h xengUpchanSetPfb): coeffs float32 [ntap * nupchan] on the host, or None with ntap 1
        (the plain FFT).  Waits for the context's work in flight; the history starts empty."""
        return self._lib.xengUpchanSetPfb(int(ntap), _host_floats(coeffs))

    def upchan_reset(self):
        """The next run sees zeros before its gulp (host state only)."""
        ffi.check("xengUpchanReset", self._enq.xengUpchanReset())

    # ---- upchannelised correlator (UpchanCorr; include/xeng.h "Upchannelised correlator"): a context of its own, its kernels
    # on the beamformer's stream
    def upchan_corr_initialize(self, gpu, ninput, nchan, ntime, nupchan, fine_lo, fine_hi, nstage=0):
        return self._lib.xengUpchanCorrInitialize(int(gpu), int(ninput), int(nchan), int(ntime), int(nupchan), int(fine_lo), int(fine_hi), int(nstage))

    def upchan_corr_accumulate(self, in_arr):
        """Enqueue only: upchan_corr_mark / upchan_corr_wait cover it."""
        return self._enq.xengUpchanCorrAccumulate(in_arr.ptr)

    def upchan_corr_accumulate_parts(self, part0, ntime0, part1):
        """One gulp out of two consecutive spans of the input ring (samples [0, ntime0) in part0), no gathered copy."""
        return self._enq.xengUpchanCorrAccumulateParts(part0.ptr, int(ntime0), part1.ptr)

    def upchan_corr_dump(self, out_arr):
        """Enqueue only: the integration so far into out_arr (cf32 [nfine][ninput][ninput]); the next one starts from zero."""
        return self._enq.xengUpchanCorrDump(out_arr.ptr)

    def upchan_corr_reset(self):
        """Drops the integration in progress and the PFB history."""
        ffi.check("xengUpchanCorrReset", self._enq.xengUpchanCorrReset())

    def upchan_corr_set_pfb(self, ntap, coeffs):
        """As upchan_set_pfb, for the UpchanCorr context (include/xeng.h xengUpchanCorrSetPfb)."""
        return self._lib.xengUpchanCorrSetPfb(int(ntap), _host_floats(coeffs))

    def upchan_corr_prime(self, in_arr):
        """Enqueue only: the PFB history from this gulp's tail, nothing accumulated; upchan_corr_mark / wait cover it."""
        return self._enq.xengUpchanCorrPrime(in_arr.ptr)

    def upchan_corr_prime_parts(self, part0, ntime0, part1):
        return self._enq.xengUpchanCorrPrimeParts(part0.ptr, int(ntime0), part1.ptr)

    # ---- fine-channel power beams from live beams (UpchanSumBeams; include/xeng.h "Fine-channel power beams from live beams"):
    # a context of its own, its kernels on the beamformer's stream
    def upchan_sum_beams_initialize(self, gpu, nchan, nbeam, ntime, nupchan, pair0, npair, nframe_sum):
        return self._lib.xengUpchanSumBeamsInitialize(int(gpu), int(nchan), int(nbeam), int(ntime), int(nupchan), int(pair0), int(npair), int(nframe_sum))

    def upchan_sum_beams_info(self):
        """(gulps per window, windows per gulp, gulps of the window in progress already run)"""
        g, w, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ffi.call("xengUpchanSumBeamsGetInfo", ctypes.byref(g), ctypes.byref(w), ctypes.byref(p))
        return g.value, w.value, p.value

    def upchan_sum_beams_run(self, in_arr, out_arr):
        """Enqueue only: out_arr (None on a gulp that completes no window) gets f32 [nwin][npair][nchan][nupchan][4];
        upchan_sum_beams_mark / wait cover it."""
        return self._enq.xengUpchanSumBeamsRun(in_arr.ptr, out_arr.ptr if out_arr is not None else None)

    def upchan_sum_beams_set_pfb(self, ntap, coeffs):
        """As upchan_set_pfb, for the UpchanSumBeams context (include/xeng.h xengUpchanSumBeamsSetPfb)."""
        return self._lib.xengUpchanSumBeamsSetPfb(int(ntap), _host_floats(coeffs))

    def upchan_sum_beams_prime(self, in_arr):
        """Enqueue only: the PFB history from this gulp's tail, nothing summed; upchan_sum_beams_mark / wait cover it."""
        return self._enq.xengUpchanSumBeamsPrime(in_arr.ptr)

    def upchan_sum_beams_reset(self):
        """Drops the window in progress and the PFB history (host state only)."""
        ffi.check("xengUpchanSumBeamsReset", self._enq.xengUpchanSumBeamsReset())

    # ---- per-input fine-channel spectra (UpchanSpectra; include/xeng.h "Per-input fine-channel spectra"): a context of its own,
    # its kernel on the beamformer's stream
    def upchan_spectra_initialize(self, gpu, ninput, nchan, ntime, nupchan, nframe_sum):
        return self._lib.xengUpchanSpectraInitialize(int(gpu), int(ninput), int(nchan), int(ntime), int(nupchan), int(nframe_sum))

    def upchan_spectra_info(self):
        """(gulps per window, windows per gulp, gulps of the window in progress already run)"""
        g, w, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        ffi.call("xengUpchanSpectraGetInfo", ctypes.byref(g), ctypes.byref(w), ctypes.byref(p))
        return g.value, w.value, p.value

    def upchan_spectra_run(self, in_arr, out_arr):
        """Enqueue only: out_arr (None on a gulp that completes no window) gets f32 [nwin][2][nchan][nupchan][ninput];
        upchan_spectra_mark / wait cover it."""
        return self._enq.xengUpchanSpectraRun(in_arr.ptr, out_arr.ptr if out_arr is not None else None)

    def upchan_spectra_run_parts(self, part0, ntime0, part1, out_arr):
        """One gulp out of two consecutive spans of the input ring (samples [0, ntime0) in part0), one launch, no gathered copy."""
        return self._enq.xengUpchanSpectraRunParts(part0.ptr, int(ntime0), part1.ptr, out_arr.ptr if out_arr is not None else None)

    def upchan_spectra_set_pfb(self, ntap, coeffs):
        """As upchan_set_pfb, for the UpchanSpectra context (include/xeng.h xengUpchanSpectraSetPfb)."""
        return self._lib.xengUpchanSpectraSetPfb(int(ntap), _host_floats(coeffs))

    def upchan_spectra_prime(self, in_arr):
        """Enqueue only: the PFB history from this gulp's tail, nothing summed; upchan_spectra_mark / wait cover it."""
        return self._enq.xengUpchanSpectraPrime(in_arr.ptr)

    def upchan_spectra_prime_parts(self, part0, ntime0, part1):
        return self._enq.xengUpchanSpectraPrimeParts(part0.ptr, int(ntime0), part1.ptr)

    def upchan_spectra_reset(self):
        """Drops the window in progress and the PFB history (host state only)."""
        ffi.check("xengUpchanSpectraReset", self._enq.xengUpchanSpectraReset())

    # ---- incoherent dedispersion of fine-channel power beams (BeamDedisperse; include/xeng.h "Incoherent dedispersion of
    # fine-channel power beams"): a context of its own, its kernels on the beamformer's stream
    def dedisp_initialize(self, gpu, npair, nfine, nwin, ndm, max_delay, nprod):
        return self._lib.xengDedispInitialize(int(gpu), int(npair), int(nfine), int(nwin), int(ndm), int(max_delay), int(nprod))

    def dedisp_set_delays(self, delays):
        """delays: host int32 [ndm][nfine], C-contiguous, in windows.  Waits for the context's work in flight; clears the history."""
        return self._lib.xengDedispSetDelays(delays.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def dedisp_set_weights(self, weights):
        """weights: host float32 [nfine] or None (all ones).  Waits for the context's work in flight; the history stays."""
        return self._lib.xengDedispSetWeights(_host_floats(weights))

    def dedisp_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][nfine][4] in, f32 [nwin_call][npair][ndm][nprod] out; dedisp_mark / wait cover it."""
        return self._enq.xengDedispRun(in_arr.ptr, int(nwin_call), out_arr.ptr)

    def dedisp_reset(self):
        """The next input counts as window 0 of an empty history (host state only)."""
        ffi.check("xengDedispReset", self._enq.xengDedispReset())

    def dedisp_info(self):
        """(largest delay of the table in use, -1 without one; windows taken since the last reset)"""
        s, n = ctypes.c_int(), ctypes.c_longlong()
        ffi.call("xengDedispGetInfo", ctypes.byref(s), ctypes.byref(n))
        return s.value, n.value

    # ---- boxcar single-pulse search of the dedispersed beams (BeamPulseSearch; include/xeng.h "Boxcar single-pulse search of the
    # dedispersed beams"): a context of its own, its kernel on the beamformer's stream
    def pulse_initialize(self, gpu, npair, ndm, nwin, nprod, nwidth, nstat):
        return self._lib.xengPulseInitialize(int(gpu), int(npair), int(ndm), int(nwin), int(nprod), int(nwidth), int(nstat))

    def pulse_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][ndm][nprod] in, [npair][ndm] records {f32 snr, i32 n_call, i32 iw, f32 B} out;
        pulse_mark / wait cover it."""
        return self._enq.xengPulseRun(in_arr.ptr, int(nwin_call), out_arr.ptr)

    def pulse_reset(self):
        """The next input counts as window 0: no baseline, no boxcar reaches back (host state only)."""
        ffi.check("xengPulseReset", self._enq.xengPulseReset())

    def pulse_info(self):
        """(windows taken since the last reset, baseline blocks of them complete)"""
        n, k = ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengPulseGetInfo", ctypes.byref(n), ctypes.byref(k))
        return n.value, k.value

    def pulse_baseline(self, npair, ndm):
        """Waits for the context's work; (c, m, var) of the last complete block, float32 [npair][ndm] each."""
        out = [np.empty((npair, ndm), np.float32) for _ in range(3)]
        ffi.call("xengPulseGetBaseline", *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in out])
        return tuple(out)

    # ---- phase-folded profiles of the fine-channel power beams (BeamFold; include/xeng.h "Phase-folded profiles of the
    # fine-channel power beams"): a context of its own, its kernels on the beamformer's stream
    def fold_initialize(self, gpu, npair, nfine, nwin, nbin, nprod):
        return self._lib.xengFoldInitialize(int(gpu), int(npair), int(nfine), int(nwin), int(nbin), int(nprod))

    def fold_set_phase(self, phi0, dphi, ddphi, active, n_ref):
        """Host arrays of npair entries: uint64 phi0 and dphi, int64 ddphi (turns * 2^64 per window, per window^2), uint8 active;
        n_ref the window at which the oscillators have m = 0.  Waits for the context's work in flight; clears nothing."""
        return self._lib.xengFoldSetPhase(phi0.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), dphi.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                                          ddphi.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), active.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                          int(n_ref))

    def fold_set_rotations(self, rot):
        """rot: host int32 [npair][nfine], C-contiguous, each in [0, nbin), or None (all zeros).  Waits; acts on dumps only."""
        return self._lib.xengFoldSetRotations(None if rot is None else rot.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def fold_set_weights(self, weights):
        """weights: host float32 [nfine] or None (all ones).  Waits; acts on dumps only."""
        return self._lib.xengFoldSetWeights(_host_floats(weights))

    def fold_run(self, in_arr, nwin_call):
        """Enqueue only: f32 [nwin_call][npair][nfine][4] folded into the profile on the device; fold_mark / wait cover it."""
        return self._enq.xengFoldRun(in_arr.ptr, int(nwin_call))

    def fold_dump(self, out_arr, hits, nfscr, normalise, clear):
        """out_arr: f32 [npair][nprod][nfine/nfscr][nbin] on the device; hits: host uint32 [npair][nbin] (filled on return) or
        None.  May wait for the context's work in flight; the dump itself is enqueued (fold_sync / mark cover it)."""
        return self._lib.xengFoldDump(out_arr.ptr, None if hits is None else hits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), int(nfscr),
                                      int(bool(normalise)), int(bool(clear)))

    def fold_reset(self):
        """The count back to 0, hits and profile cleared (one enqueued launch)."""
        ffi.check("xengFoldReset", self._enq.xengFoldReset())

    def fold_info(self):
        """(windows taken since the last reset, windows folded since the last clear)"""
        n, f = ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengFoldGetInfo", ctypes.byref(n), ctypes.byref(f))
        return n.value, f.value

    # ---- FFT periodicity search of the dedispersed beams (BeamPeriodSearch; include/xeng.h "FFT periodicity search of the
    # dedispersed beams"): a context of its own, its kernels on the beamformer's stream
    def period_initialize(self, gpu, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kmin):
        return self._lib.xengPeriodInitialize(int(gpu), int(npair), int(ndm), int(nwin), int(nprod), int(nt), int(nstack), int(nlevel), int(nwhite),
                                              int(kmin))

    def period_set_mask(self, keep):
        """keep: host uint8 [nt/2], 0 = zapped, or None (all kept).  Waits for the context's work in flight; holds from the next
        segment to complete."""
        return self._lib.xengPeriodSetMask(None if keep is None else keep.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def period_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][ndm][nprod] in; (status, completed).  out_arr, [npair][ndm][nlevel] records
        {f32 H, i32 k}, is written only when the call completes a stack (completed = 1) and may be None on every other call;
        period_mark / wait cover it."""
        done = ctypes.c_int(0)
        rv = self._enq.xengPeriodRun(in_arr.ptr, int(nwin_call), None if out_arr is None else out_arr.ptr, ctypes.byref(done))
        return rv, done.value

    def period_reset(self):
        """The next input counts as window 0 of a new stack (host state only)."""
        ffi.check("xengPeriodReset", self._enq.xengPeriodReset())

    def period_info(self):
        """(windows taken since the last reset, complete segments of the stack in progress, stacks completed since the reset)"""
        n, s, k = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong()
        ffi.call("xengPeriodGetInfo", ctypes.byref(n), ctypes.byref(s), ctypes.byref(k))
        return n.value, s.value, k.value

    def period_spectrum(self, npair, ndm, nt):
        """Waits for the context's work; (A, nseg): the stack as it stands, float32 [npair][ndm][nt/2], and the segments in it."""
        A, nseg = np.empty((npair, ndm, nt // 2), np.float32), ctypes.c_int()
        ffi.call("xengPeriodGetSpectrum", A.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(nseg))
        return A, nseg.value

    # ---- FFT periodicity search with long segments (BeamPeriodSearchLong; include/xeng.h "FFT periodicity search with long
    # segments"): a context of its own, its kernels on the beamformer's stream
    def plong_initialize(self, gpu, npair, ndm, nwin, nprod, nt, nstack, nlevel, nwhite, kedge):
        """kedge: the nband + 1 band edges, strictly ascending integers."""
        e = np.ascontiguousarray(kedge, np.int32)
        return self._lib.xengPlongInitialize(int(gpu), int(npair), int(ndm), int(nwin), int(nprod), int(nt), int(nstack), int(nlevel), int(nwhite),
                                             int(e.size - 1), e.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def plong_set_mask(self, keep):
        """keep: host uint8 [nt/2], 0 = zapped, or None (all kept).  Waits for the context's work in flight; holds from the next
        segment to complete."""
        return self._lib.xengPlongSetMask(None if keep is None else keep.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def plong_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][ndm][nprod] in; (status, completed).  out_arr, [npair][ndm][nlevel][nband] records
        {f32 H, i32 k}, is written only when the call completes a stack (completed = 1) and may be None on every other call;
        plong_mark / wait cover it."""
        done = ctypes.c_int(0)
        rv = self._enq.xengPlongRun(in_arr.ptr, int(nwin_call), None if out_arr is None else out_arr.ptr, ctypes.byref(done))
        return rv, done.value

    def plong_reset(self):
        """The next input counts as window 0 of a new stack (host state only)."""
        ffi.check("xengPlongReset", self._enq.xengPlongReset())

    def plong_info(self):
        """(windows taken since the last reset, complete segments of the stack in progress, stacks completed since the reset)"""
        n, s, k = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong()
        ffi.call("xengPlongGetInfo", ctypes.byref(n), ctypes.byref(s), ctypes.byref(k))
        return n.value, s.value, k.value

    def plong_spectrum(self, series0, nser, nt):
        """Waits for the context's work; (A, nseg): series [series0, series0 + nser) of the stack as it stands, float32
        [nser][nt/2] in natural k order, and the segments in it."""
        A, nseg = np.empty((nser, nt // 2), np.float32), ctypes.c_int()
        ffi.call("xengPlongGetSpectrum", int(series0), int(nser), A.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(nseg))
        return A, nseg.value

    # ---- acceleration search of the long-segment spectra (BeamAccelSearch; include/xeng.h "Acceleration search of the long-segment
    # spectra"): a context of its own, its kernels on the beamformer's stream
    def accel_initialize(self, gpu, npair, ndm, nwin, nprod, nt, nlevel, nwhite, kedge, alphas):
        """kedge: the nband + 1 band edges, strictly ascending integers; alphas: the ntrial index-map coefficients (float64)."""
        e, a = np.ascontiguousarray(kedge, np.int32), np.ascontiguousarray(alphas, np.float64).reshape(-1)
        return self._lib.xengAccelInitialize(int(gpu), int(npair), int(ndm), int(nwin), int(nprod), int(nt), int(nlevel), int(nwhite), int(e.size - 1),
                                             e.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(a.size), a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))

    def accel_set_mask(self, keep):
        """keep: host uint8 [nt/2], 0 = zapped, or None (all kept).  Waits for the context's work in flight; holds from the next
        segment to complete."""
        return self._lib.xengAccelSetMask(None if keep is None else keep.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def accel_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][ndm][nprod] in; (status, completed).  out_arr, [npair][ndm][nlevel][nband] records
        {f32 H, i32 k, i32 ia, f32 H0}, is written only when the call completes a segment (completed = 1) and may be None on every
        other call; accel_mark / wait cover it."""
        done = ctypes.c_int(0)
        rv = self._enq.xengAccelRun(in_arr.ptr, int(nwin_call), None if out_arr is None else out_arr.ptr, ctypes.byref(done))
        return rv, done.value

    def accel_reset(self):
        """The next input counts as window 0 of a new segment (host state only)."""
        ffi.check("xengAccelReset", self._enq.xengAccelReset())

    def accel_info(self):
        """(windows taken since the last reset, segments completed since the reset)"""
        n, k = ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengAccelGetInfo", ctypes.byref(n), ctypes.byref(k))
        return n.value, k.value

    def accel_trial_records(self, series0, nser, ntrial, nlevel, nband):
        """Waits for the context's work; the trial records of series [series0, series0 + nser) of the segment that completed last:
        a {f32 H, i32 k} array [ntrial][nser][nlevel][nband]."""
        rec = np.empty((ntrial, nser, nlevel, nband), np.dtype([('H', '<f4'), ('k', '<i4')]))
        ffi.call("xengAccelGetTrialRecords", int(series0), int(nser), rec.ctypes.data)
        return rec

    def accel_set_batch(self, nser_batch):
        """The series per batch from the next call on (0: as many as the scratch holds).  Results do not depend on it."""
        ffi.call("xengAccelSetBatch", int(nser_batch))

    def accel_get_batch(self):
        """(series per batch as the launches take it, as the scratch holds it)"""
        a, b = ctypes.c_int(), ctypes.c_int()
        ffi.call("xengAccelGetBatch", ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    # ---- fast-folding search of the dedispersed beams (BeamFfaSearch; include/xeng.h "Fast-folding search of the dedispersed
    # beams"): a context of its own, its kernels on the beamformer's stream
    def ffa_initialize(self, gpu, npair, ndm, nwin, nprod, nds, nt, noct, pmin, pmax, nwidth):
        return self._lib.xengFfaInitialize(int(gpu), int(npair), int(ndm), int(nwin), int(nprod), int(nds), int(nt), int(noct), int(pmin), int(pmax),
                                           int(nwidth))

    def ffa_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][ndm][nprod] in; (status, completed).  out_arr, [npair][ndm][noct][nwidth] records
        {f32 snr, i32 p, i32 i, i32 j}, is written only when the call completes a segment (completed = 1) and may be None on
        every other call; ffa_mark / wait cover it."""
        done = ctypes.c_int(0)
        rv = self._enq.xengFfaRun(in_arr.ptr, int(nwin_call), None if out_arr is None else out_arr.ptr, ctypes.byref(done))
        return rv, done.value

    def ffa_reset(self):
        """The next input counts as window 0 of a new segment (host state only)."""
        ffi.check("xengFfaReset", self._enq.xengFfaReset())

    def ffa_info(self):
        """(windows taken since the last reset, segments completed since the reset)"""
        n, k = ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengFfaGetInfo", ctypes.byref(n), ctypes.byref(k))
        return n.value, k.value

    def ffa_stats(self, npair, ndm, noct):
        """Waits for the context's work; {c, m, v, g} of the last completed segment, float32 [npair][ndm][noct][4]."""
        st = np.empty((npair, ndm, noct, 4), np.float32)
        ffi.call("xengFfaGetStats", st.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        return st

    # ---- folding of search candidates (BeamCandFold; include/xeng.h "Folding of search candidates"): a context of its own, its kernels
    # on the beamformer's stream
    def candfold_initialize(self, gpu, npair, ndm, nwin, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, d1, d2, gains):
        """d1, d2: the trial table in sixteenths of a bin (blocks/cand_fold.py candfold_trials); gains: float32 [nwidth]."""
        d1, d2 = np.ascontiguousarray(d1, np.int32), np.ascontiguousarray(d2, np.int32)
        gains = np.ascontiguousarray(gains, np.float32)
        if d1.shape != d2.shape or d1.ndim != 1 or gains.shape != (int(nwidth),):
            raise ValueError("candfold_initialize: d1 %r and d2 %r are not one table, or gains %r not [nwidth]" % (d1.shape, d2.shape, gains.shape))
        return self._lib.xengCandfoldInitialize(int(gpu), int(npair), int(ndm), int(nwin), int(nprod), int(ncand_max), int(nbin), int(nsub), int(nsubwin),
                                                int(nwidth), d1.size, d1.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                d2.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), gains.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))

    def candfold_set_candidates(self, series, phi0, dphi, ddphi, active):
        """Host arrays of one entry per candidate (blocks/cand_fold.py candfold_oscillators).  Waits for the context's work in
        flight; in force from the next segment boundary, or at once when the window count stands on one."""
        series = np.ascontiguousarray(series, np.int32)
        phi0, dphi = np.ascontiguousarray(phi0, np.uint64), np.ascontiguousarray(dphi, np.uint64)
        ddphi, active = np.ascontiguousarray(ddphi, np.int64), np.ascontiguousarray(active, np.uint8)
        if not series.shape == phi0.shape == dphi.shape == ddphi.shape == active.shape or series.ndim != 1:
            raise ValueError("candfold_set_candidates: the arrays are not one entry per candidate")
        u64 = ctypes.POINTER(ctypes.c_ulonglong)
        return self._lib.xengCandfoldSetCandidates(series.size, series.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), phi0.ctypes.data_as(u64),
                                                   dphi.ctypes.data_as(u64), ddphi.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                                   active.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def candfold_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][ndm][nprod] in; (status, completed).  out_arr, ncand_max records {f32 S, f32 S0, i16 it,
        i16 iw, i16 j, i16 pad} and then f32 [ncand_max][nbin] best profiles, is written only when the call completes a segment
        (completed = 1) and may be None on every other call; candfold_mark / wait cover it."""
        done = ctypes.c_int(0)
        rv = self._enq.xengCandfoldRun(in_arr.ptr, int(nwin_call), None if out_arr is None else out_arr.ptr, ctypes.byref(done))
        return rv, done.value

    def candfold_reset(self):
        """The next input counts as window 0 of a new segment with m = 0; the partial cube is cleared by one launch."""
        ffi.check("xengCandfoldReset", self._enq.xengCandfoldReset())

    def candfold_info(self):
        """(windows taken since the last reset, segments completed since the reset)"""
        n, k = ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengCandfoldGetInfo", ctypes.byref(n), ctypes.byref(k))
        return n.value, k.value

    def candfold_cube(self, ncand_max, nsub, nbin):
        """Waits for the context's work; (cube float32, hits uint32), each [ncand_max][nsub][nbin], of the last completed segment."""
        cube, hits = np.empty((ncand_max, nsub, nbin), np.float32), np.empty((ncand_max, nsub, nbin), np.uint32)
        ffi.call("xengCandfoldGetCube", cube.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), hits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
        return cube, hits

    # ---- cleaning of the fine-channel power beams (BeamRfiClean; include/xeng.h "Cleaning of the fine-channel power beams"): a context
    # of its own, its kernels on the beamformer's stream
    def rfi_initialize(self, gpu, npair, nfine, nwin, nstat):
        return self._lib.xengRfiInitialize(int(gpu), int(npair), int(nfine), int(nwin), int(nstat))

    def rfi_set_control(self, k_chan, t_clip, t_broad, min_count, zerodm):
        """The thresholds as the library takes them (blocks/rfi_clean.py rfi_controls); they hold from the next block to be decided."""
        return self._lib.xengRfiSetControl(float(k_chan), float(t_clip), float(t_broad), int(min_count), int(bool(zerodm)))

    def rfi_set_mask(self, mask):
        """mask: host uint8 [nfine], non-zero = left out, or None (none left out).  Waits for the context's work in flight; holds
        from the next block to be decided."""
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
        return self._lib.xengRfiSetMask(None if mask is None else mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def rfi_run(self, in_arr, nwin_call, out_arr, stats_arr):
        """Enqueue only: f32 [nwin_call][npair][nfine][4] in and out, i32 [nwin_call][npair][4] stats; (status, completed): the call
        decided a block.  The output is the cleaned input nstat windows earlier; rfi_mark / wait cover it."""
        done = ctypes.c_int(0)
        rv = self._enq.xengRfiRun(in_arr.ptr, int(nwin_call), out_arr.ptr, stats_arr.ptr, ctypes.byref(done))
        return rv, done.value

    def rfi_reset(self):
        """The next input counts as window 0 (host state only)."""
        ffi.check("xengRfiReset", self._enq.xengRfiReset())

    def rfi_info(self):
        """(windows taken since the last reset, blocks decided since the reset)"""
        n, k = ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengRfiGetInfo", ctypes.byref(n), ctypes.byref(k))
        return n.value, k.value

    def rfi_block(self, npair, nfine):
        """Waits for the context's work; the newest decided block's tables: (flags uint8, mu, var, r float32, each [npair][nfine],
        gains float32 [npair][nfine][4])."""
        flags = np.empty((npair, nfine), np.uint8)
        mu, var, r = (np.empty((npair, nfine), np.float32) for _ in range(3))
        gains = np.empty((npair, nfine, 4), np.float32)
        pf = ctypes.POINTER(ctypes.c_float)
        ffi.call("xengRfiGetBlock", flags.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), mu.ctypes.data_as(pf), var.ctypes.data_as(pf), r.ctypes.data_as(pf),
                 gains.ctypes.data_as(pf))
        return flags, mu, var, r, gains

    # ---- baseline removal of the dedispersed beams (BeamDetrend; include/xeng.h "Baseline removal of the dedispersed beams"): a context
    # of its own, its kernels on the beamformer's stream
    def detrend_initialize(self, gpu, npair, ndm, nwin, nprod, nblk, normalise, k_mad):
        """k_mad as the library takes it (blocks/detrend.py detrend_k_mad folds in 1.4826)."""
        return self._lib.xengDetrendInitialize(int(gpu), int(npair), int(ndm), int(nwin), int(nprod), int(nblk), int(bool(normalise)), float(k_mad))

    def detrend_run(self, in_arr, nwin_call, out_arr):
        """Enqueue only: f32 [nwin_call][npair][ndm][nprod] in, f32 [nwin_call][npair][ndm] out; (status, completed): the call decided
        a block.  The output is the detrended input 3 nblk / 2 windows earlier; detrend_mark / wait cover it."""
        done = ctypes.c_int(0)
        rv = self._enq.xengDetrendRun(in_arr.ptr, int(nwin_call), out_arr.ptr, ctypes.byref(done))
        return rv, done.value

    def detrend_reset(self):
        """The next input counts as window 0 (host state only)."""
        ffi.check("xengDetrendReset", self._enq.xengDetrendReset())

    def detrend_info(self):
        """(windows taken since the last reset, blocks decided since the reset)"""
        n, k = ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengDetrendGetInfo", ctypes.byref(n), ctypes.byref(k))
        return n.value, k.value

    def detrend_knots(self, npair, ndm):
        """Waits for the context's work; the newest decided block's knots: (M, A float32, valid uint8, each [npair][ndm])."""
        M, A = (np.empty((npair, ndm), np.float32) for _ in range(2))
        valid = np.empty((npair, ndm), np.uint8)
        pf = ctypes.POINTER(ctypes.c_float)
        ffi.call("xengDetrendGetKnots", M.ctypes.data_as(pf), A.ctypes.data_as(pf), valid.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
        return M, A, valid

    # ---- dedispersed cut-outs of single pulses (BeamPulseCutout; include/xeng.h "Dedispersed cut-outs and DM refinement of single
    # pulses"): a context of its own, its kernels on the beamformer's stream
    def cutout_initialize(self, gpu, npair, nfine, nwin, ndmf, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, k_mad):
        """k_mad as the library takes it (blocks/pulse_cutout.py cutout_k_mad folds in 1.4826)."""
        return self._lib.xengCutoutInitialize(int(gpu), int(npair), int(nfine), int(nwin), int(ndmf), int(nhist), int(nband), int(nt), int(tscr), int(ndmc),
                                              int(nwidth), int(nreq_max), float(k_mad))

    def cutout_set_delays(self, delays):
        """delays: host int32 [ndmf][nfine], C-contiguous, in windows.  Waits for the context's work in flight; clears the count and
        the pending requests."""
        return self._lib.xengCutoutSetDelays(delays.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def cutout_set_weights(self, weights):
        """weights: host float32 [nfine] or None (all ones).  Waits for the context's work in flight; acts on the history held."""
        return self._lib.xengCutoutSetWeights(_host_floats(weights))

    def cutout_request(self, reqs):
        """reqs: a host array of CUTOUT_REQUEST {id, pair, n_c, ic, dstep} (blocks/pulse_cutout.py): all taken, or none."""
        reqs = np.ascontiguousarray(reqs)
        if reqs.dtype.itemsize != 24 or reqs.ndim != 1:
            raise ValueError("cutout_request: %r of %r is not a list of 24-byte requests" % (reqs.shape, reqs.dtype))
        return self._enq.xengCutoutRequest(reqs.size, reqs.ctypes.data)

    def cutout_run(self, in_arr, nwin_call, out_arr, nreq_max):
        """Enqueue only: f32 [nwin_call][npair][nfine][4] in; (status, served ids in slot order, expired ids).  out_arr (records, then
        the waterfalls, then the planes: cutout_info's bytes) is written only when the call serves a request and may be None
        otherwise -- the status tells when it was needed; cutout_mark / wait cover it."""
        ns, ne = ctypes.c_int(0), ctypes.c_int(0)
        served, expired = (ctypes.c_int * int(nreq_max))(), (ctypes.c_int * 1024)()
        rv = self._enq.xengCutoutRun(in_arr.ptr, int(nwin_call), None if out_arr is None else out_arr.ptr, ctypes.byref(ns), served, ctypes.byref(ne), expired)
        return rv, list(served[:ns.value]), list(expired[:ne.value])

    def cutout_reset(self):
        """The next input counts as window 0; the pending requests are dropped (host state only)."""
        ffi.check("xengCutoutReset", self._enq.xengCutoutReset())

    def cutout_info(self):
        """(windows taken since the last reset, requests waiting, bytes of a serving call's output)"""
        n, k, b = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong()
        ffi.call("xengCutoutGetInfo", ctypes.byref(n), ctypes.byref(k), ctypes.byref(b))
        return n.value, k.value, b.value

    # ---- Faraday rotation-measure synthesis of folded profiles (BeamRmSynth; include/xeng.h "Faraday rotation-measure synthesis of
    # folded profiles"): a context of its own, its kernels on the beamformer's stream
    def rmsynth_initialize(self, gpu, npair, nchg, nbin, nphi, feeds):
        """feeds: 0 linear, 1 circular."""
        return self._lib.xengRmsynthInitialize(int(gpu), int(npair), int(nchg), int(nbin), int(nphi), int(feeds))

    def rmsynth_set_table(self, T, w=None, use=None):
        """T: host float32 [nchg][nphi][2] = (Tc, Ts), C-contiguous; w: host float32 [nchg] or None (all 1); use: host uint8 [nchg] or
        None (all).  Waits for the context's work in flight."""
        if T.dtype != np.float32 or not T.flags.c_contiguous or (use is not None and (use.dtype != np.uint8 or not use.flags.c_contiguous)):
            raise ValueError("rmsynth_set_table: the table must be C-contiguous float32 and `use` C-contiguous uint8")
        return self._lib.xengRmsynthSetTable(T.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _host_floats(w),
                                             None if use is None else use.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def rmsynth_set_masks(self, off=None, on=None):
        """off, on: host uint8 [npair][nbin], C-contiguous, or None (every bin).  Waits for the context's work in flight."""
        for m in (off, on):
            if m is not None and (m.dtype != np.uint8 or not m.flags.c_contiguous):
                raise ValueError("rmsynth_set_masks: a mask must be C-contiguous uint8")
        pb = ctypes.POINTER(ctypes.c_ubyte)
        return self._lib.xengRmsynthSetMasks(None if off is None else off.ctypes.data_as(pb), None if on is None else on.ctypes.data_as(pb))

    def rmsynth_set_active(self, active=None):
        """active: host uint8 [npair] or None (all).  Waits for the context's work in flight."""
        if active is not None and (active.dtype != np.uint8 or not active.flags.c_contiguous):
            raise ValueError("rmsynth_set_active: the list must be C-contiguous uint8")
        return self._lib.xengRmsynthSetActive(None if active is None else active.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def rmsynth_run(self, in_arr, out_arr):
        """Enqueue only: f32 [npair][4][nchg][nbin] in; records, spec and the profile out (rmsynth_info's offsets); rmsynth_mark /
        wait cover it."""
        return self._enq.xengRmsynthRun(in_arr.ptr, out_arr.ptr)

    def rmsynth_reset(self):
        """The call count starts again (host state only: a call carries nothing over to the next)."""
        ffi.check("xengRmsynthReset", self._enq.xengRmsynthReset())

    def rmsynth_info(self):
        """(calls since the last reset, used channels or -1 without a table, byte offset of spec, of the profile, bytes of the output)"""
        n, k, a, b, c = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengRmsynthGetInfo", ctypes.byref(n), ctypes.byref(k), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return n.value, k.value, a.value, b.value, c.value

    # ---- template-matched arrival phases of folded profiles (BeamToa; include/xeng.h "Template-matched arrival phases of folded
    # profiles"): a context of its own, its kernels on the beamformer's stream
    def toa_initialize(self, gpu, npair, nprod, nchg, nbin, nsub, nharm, nlag):
        self._toa_nsub = int(nsub)
        return self._lib.xengToaInitialize(int(gpu), int(npair), int(nprod), int(nchg), int(nbin), int(nsub), int(nharm), int(nlag))

    def toa_set_bands(self, edges, w=None):
        """edges: host int32 [nsub + 1], ascending group indices, C-contiguous; w: host float32 [nchg] or None (all 1); a group of
        weight 0 is left out.  Waits for the context's work in flight."""
        if edges.dtype != np.int32 or not edges.flags.c_contiguous:
            raise ValueError("toa_set_bands: the edges must be C-contiguous int32")
        return self._lib.xengToaSetBands(edges.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _host_floats(w))

    def toa_set_tables(self, D, L):
        """D: host float32 [nbin][nharm][2], L: host float32 [nharm][nlag][2] (blocks/toa.py toa_tables), C-contiguous.  Waits for
        the context's work in flight."""
        for t in (D, L):
            if t.dtype != np.float32 or not t.flags.c_contiguous:
                raise ValueError("toa_set_tables: a table must be C-contiguous float32")
        pf = ctypes.POINTER(ctypes.c_float)
        return self._lib.xengToaSetTables(D.ctypes.data_as(pf), L.ctypes.data_as(pf))

    def toa_set_template(self, S):
        """S: host float32 [npair][nsub + 1][nharm][2] (blocks/toa.py toa_template), C-contiguous.  Waits for the context's work in
        flight."""
        if S.dtype != np.float32 or not S.flags.c_contiguous:
            raise ValueError("toa_set_template: the template must be C-contiguous float32")
        return self._lib.xengToaSetTemplate(S.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))

    def toa_set_mask(self, off=None):
        """off: host uint8 [npair][nbin], C-contiguous, or None (every bin).  Waits for the context's work in flight."""
        if off is not None and (off.dtype != np.uint8 or not off.flags.c_contiguous):
            raise ValueError("toa_set_mask: the mask must be C-contiguous uint8")
        return self._lib.xengToaSetMask(None if off is None else off.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def toa_set_active(self, active=None):
        """active: host uint8 [npair] or None (all).  Waits for the context's work in flight."""
        if active is not None and (active.dtype != np.uint8 or not active.flags.c_contiguous):
            raise ValueError("toa_set_active: the list must be C-contiguous uint8")
        return self._lib.xengToaSetActive(None if active is None else active.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def toa_run(self, in_arr, out_arr):
        """Enqueue only: f32 [npair][nprod][nchg][nbin] in; records, P, PH and ccf out (toa_info's offsets); toa_mark / wait cover it."""
        return self._enq.xengToaRun(in_arr.ptr, out_arr.ptr)

    def toa_reset(self):
        """The call count starts again (host state only: a call carries nothing over to the next)."""
        ffi.check("xengToaReset", self._enq.xengToaReset())

    def toa_info(self):
        """(calls since the last reset, used groups per sub-band (-1 each before toa_set_bands), byte offset of P, of PH, of ccf,
        bytes of the output)"""
        n, a, b, c, d = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        used = (ctypes.c_int * self._toa_nsub)()
        ffi.call("xengToaGetInfo", ctypes.byref(n), used, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d))
        return n.value, list(used), a.value, b.value, c.value, d.value

    # ---- coherent dedispersion of the voltage beams (BeamCoherentDedisperse; include/xeng.h "Coherent dedispersion of the voltage
    # beams"): a context of its own, its kernels on the beamformer's stream
    def cdedisp_initialize(self, gpu, nchan, nbeam, ntime, pair0, npair, nfft, overlap):
        return self._lib.xengCdedispInitialize(int(gpu), int(nchan), int(nbeam), int(ntime), int(pair0), int(npair), int(nfft), int(overlap))

    def cdedisp_set_chirp(self, table):
        """table: host complex64 [npair][nchan][nfft], C-contiguous, natural DFT order, 1/nfft included.  Waits for the context's
        work in flight; holds from the next block to complete."""
        _host_array("cdedisp_set_chirp", "the table", table, np.complex64)
        return self._lib.xengCdedispSetChirp(table.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))

    def cdedisp_run(self, in_arr, out_arr):
        """Enqueue only: cf32 [nchan][nbeam][ntime] in; (status, nblocks).  out_arr gets cf32 [nblocks][nchan][2 npair][L] and may be
        None on a call that completes no block; cdedisp_mark / wait cover it."""
        n = ctypes.c_int(0)
        rv = self._enq.xengCdedispRun(in_arr.ptr, None if out_arr is None else out_arr.ptr, ctypes.byref(n))
        return rv, n.value

    def cdedisp_reset(self):
        """The next input sample counts as sample 0 (host state only)."""
        ffi.check("xengCdedispReset", self._enq.xengCdedispReset())

    def cdedisp_info(self):
        """(the step L, the most blocks a call completes, samples taken since the last reset, blocks completed since the reset)"""
        s, m, n, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengCdedispGetInfo", ctypes.byref(s), ctypes.byref(m), ctypes.byref(n), ctypes.byref(b))
        return s.value, m.value, n.value, b.value

    # ---- coherent dedispersion with long transforms (BeamCoherentDedisperseLong; include/xeng.h "Coherent dedispersion with long
    # transforms"): xengCdedisp*'s contract for 2^14 to 2^20 points, a context of its own, its kernels on the beamformer's stream
    def cdlong_initialize(self, gpu, nchan, nbeam, ntime, pair0, npair, nfft, overlap):
        return self._lib.xengCdlongInitialize(int(gpu), int(nchan), int(nbeam), int(ntime), int(pair0), int(npair), int(nfft), int(overlap))

    def cdlong_set_chirp(self, pair, table):
        """table: host complex64 [nchan][nfft] of pair `pair`, C-contiguous, natural DFT order, 1/nfft included.  Waits for the
        context's work in flight; holds from the next block to complete."""
        _host_array("cdlong_set_chirp", "the table", table, np.complex64)
        return self._lib.xengCdlongSetChirp(int(pair), table.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))

    def cdlong_run(self, in_arr, out_arr):
        """Enqueue only: cf32 [nchan][nbeam][ntime] in; (status, nblocks).  out_arr gets cf32 [nblocks][nchan][2 npair][L] and may be
        None on a call that completes no block; cdlong_mark / wait cover it."""
        n = ctypes.c_int(0)
        rv = self._enq.xengCdlongRun(in_arr.ptr, None if out_arr is None else out_arr.ptr, ctypes.byref(n))
        return rv, n.value

    def cdlong_reset(self):
        """The next input sample counts as sample 0 (host state only)."""
        ffi.check("xengCdlongReset", self._enq.xengCdlongReset())

    def cdlong_info(self):
        """(the step L, the most blocks a call completes, samples taken since the last reset, blocks completed since the reset)"""
        s, m, n, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengCdlongGetInfo", ctypes.byref(s), ctypes.byref(m), ctypes.byref(n), ctypes.byref(b))
        return s.value, m.value, n.value, b.value

    # ---- dirty images of the fine-channel visibilities (UpchanImage; include/xeng.h "Dirty images of the fine-channel
    # visibilities"): a context of its own, its kernel on the beamformer's stream
    def image_initialize(self, gpu, nstand, nfine, nfavg, npix):
        return self._lib.xengImageInitialize(int(gpu), int(nstand), int(nfine), int(nfavg), int(npix))

    def image_set_geometry(self, tau, freq):
        """tau: host float64 [npix][nstand] seconds, freq: host float64 [nfine] Hz, both C-contiguous.  Waits for the context's work
        in flight."""
        _host_array("image_set_geometry", "tau", tau, np.float64)
        _host_array("image_set_geometry", "freq", freq, np.float64)
        pd = ctypes.POINTER(ctypes.c_double)
        return self._lib.xengImageSetGeometry(tau.ctypes.data_as(pd), freq.ctypes.data_as(pd))

    def image_set_weights(self, weights, autos):
        """weights: host float32 [nstand], finite and >= 0.  Waits for the context's work in flight; holds from the next run."""
        _host_array("image_set_weights", "the weights", weights, np.float32)
        return self._lib.xengImageSetWeights(_host_floats(weights), int(bool(autos)))

    def image_run(self, vis_arr, out_arr):
        """Enqueue only: cf32 [nfine][nstand][2][nstand][2] in, f32 [nfine / nfavg][4][npix] out; image_mark / wait cover it."""
        return self._enq.xengImageRun(vis_arr.ptr, out_arr.ptr)

    def image_info(self):
        """(channel groups, pixels per work-group, LDS bytes per work-group, norm)"""
        g, t, l, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        ffi.call("xengImageGetInfo", ctypes.byref(g), ctypes.byref(t), ctypes.byref(l), ctypes.byref(n))
        return g.value, t.value, l.value, n.value

    # ---- per-stand gains from the fine-channel visibilities (UpchanGainCal; include/xeng.h "Per-stand gains from the fine-channel
    # visibilities"): a context of its own, its kernel on the beamformer's stream
    def gaincal_initialize(self, gpu, nstand, nfine, nsrc):
        return self._lib.xengGaincalInitialize(int(gpu), int(nstand), int(nfine), int(nsrc))

    def gaincal_set_model(self, tau, freq, flux):
        """tau: host float64 [nsrc][nstand] seconds, freq: host float64 [nfine] Hz, flux: host float32 [nfine][nsrc], all
        C-contiguous.  Waits for the context's work in flight; forgets the warm start."""
        for what, a, t in (("tau", tau, np.float64), ("freq", freq, np.float64), ("flux", flux, np.float32)):
            _host_array("gaincal_set_model", what, a, t)
        pd = ctypes.POINTER(ctypes.c_double)
        return self._lib.xengGaincalSetModel(tau.ctypes.data_as(pd), freq.ctypes.data_as(pd), _host_floats(flux))

    def gaincal_set_weights(self, weights, refant):
        """weights: host float32 [nstand], finite and >= 0, that of `refant` > 0.  Waits for the context's work in flight; holds from
        the next run; forgets the warm start."""
        _host_array("gaincal_set_weights", "the weights", weights, np.float32)
        return self._lib.xengGaincalSetWeights(_host_floats(weights), int(refant))

    def gaincal_set_solver(self, niter, tol):
        return self._lib.xengGaincalSetSolver(int(niter), float(tol))

    def gaincal_run(self, vis_arr, out_arr, stats_offset, warm):
        """Enqueue only: cf32 [nfine][nstand][2][nstand][2] in; cf32 [nfine][2][nstand] gains at the start of out_arr and f32
        [nfine][2][4] stats `stats_offset` bytes into it; gaincal_mark / wait cover it."""
        return self._enq.xengGaincalRun(vis_arr.ptr, out_arr.ptr, out_arr.ptr + int(stats_offset), int(bool(warm)))

    def gaincal_info(self):
        """(LDS bytes per work-group, niter, tol, the reference stand)"""
        l, n, t, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_int()
        ffi.call("xengGaincalGetInfo", ctypes.byref(l), ctypes.byref(n), ctypes.byref(t), ctypes.byref(r))
        return l.value, n.value, t.value, r.value

    # ---- calibrated, source-subtracted visibilities (UpchanCalApply; include/xeng.h "Calibrated, source-subtracted visibilities"): a
    # context of its own, its kernels on the beamformer's stream
    def calapply_initialize(self, gpu, nstand, nfine, nsrc):
        return self._lib.xengCalapplyInitialize(int(gpu), int(nstand), int(nfine), int(nsrc))

    def calapply_set_model(self, tau, freq, flux):
        """tau: host float64 [nsrc][nstand] seconds, freq: host float64 [nfine] Hz, flux: host float32 [nfine][nsrc], all
        C-contiguous; tau and flux may be None in a context without sources.  Waits for the context's work in flight."""
        for what, a, t, optional in (("tau", tau, np.float64, True), ("freq", freq, np.float64, False), ("flux", flux, np.float32, True)):
            if not (a is None and optional):
                _host_array("calapply_set_model", what, a, t)
        pd = ctypes.POINTER(ctypes.c_double)
        return self._lib.xengCalapplySetModel(None if tau is None or not tau.size else tau.ctypes.data_as(pd), freq.ctypes.data_as(pd),
                                              None if flux is None or not flux.size else _host_floats(flux))

    def calapply_set_factors(self, h):
        """h: host complex64 [nfine][2][nstand], finite, 0 where a (stand, polarisation) is left out.  Waits for the context's work
        in flight; holds from the next run."""
        _host_array("calapply_set_factors", "the factors", h, np.complex64)
        return self._lib.xengCalapplySetFactors(h.ctypes.data_as(ctypes.c_void_p))

    def calapply_run(self, vis_arr, out_arr):
        """Enqueue only: cf32 [nfine][nstand][2][nstand][2] in and out; calapply_mark / wait cover it."""
        return self._enq.xengCalapplyRun(vis_arr.ptr, out_arr.ptr)

    def calapply_info(self):
        """(tiles of 32 stands per side, work-groups per run, LDS bytes per work-group, bytes of a span)"""
        t, g, l, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        ffi.call("xengCalapplyGetInfo", ctypes.byref(t), ctypes.byref(g), ctypes.byref(l), ctypes.byref(b))
        return t.value, g.value, l.value, b.value

    # ---- direction-dependent gains and peeling (UpchanPeel; include/xeng.h "Direction-dependent gains and peeling"): a context of
    # its own, its kernels on the beamformer's stream
    def peel_initialize(self, gpu, nstand, nfine, ndir):
        return self._lib.xengPeelInitialize(int(gpu), int(nstand), int(nfine), int(ndir))

    def peel_set_model(self, tau, freq, flux):
        """tau: host float64 [ndir][nstand] seconds, freq: host float64 [nfine] Hz, flux: host float32 [nfine][ndir], all
        C-contiguous.  Waits for the context's work in flight; forgets the warm start."""
        for what, a, t in (("tau", tau, np.float64), ("freq", freq, np.float64), ("flux", flux, np.float32)):
            _host_array("peel_set_model", what, a, t)
        pd = ctypes.POINTER(ctypes.c_double)
        return self._lib.xengPeelSetModel(tau.ctypes.data_as(pd), freq.ctypes.data_as(pd), _host_floats(flux))

    def peel_set_weights(self, weights, refant):
        """weights: host float32 [nstand], finite and >= 0, that of `refant` > 0.  Waits for the context's work in flight; holds from
        the next run; forgets the warm start."""
        _host_array("peel_set_weights", "the weights", weights, np.float32)
        return self._lib.xengPeelSetWeights(_host_floats(weights), int(refant))

    def peel_set_solver(self, niter, tol):
        return self._lib.xengPeelSetSolver(int(niter), float(tol))

    def peel_run(self, vis_arr, out_arr, sol_arr, stats_offset, warm):
        """Enqueue only: cf32 [nfine][nstand][2][nstand][2] in and out; cf32 [nfine][2][ndir][nstand] gains at the start of sol_arr
        and f32 [nfine][2][4] stats `stats_offset` bytes into it; peel_mark / wait cover it."""
        return self._enq.xengPeelRun(vis_arr.ptr, out_arr.ptr, sol_arr.ptr, sol_arr.ptr + int(stats_offset), int(bool(warm)))

    def peel_info(self):
        """(LDS bytes per work-group of the solve, niter, tol, the reference stand, bytes of a span)"""
        l, n, t, r, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_int(), ctypes.c_longlong()
        ffi.call("xengPeelGetInfo", ctypes.byref(l), ctypes.byref(n), ctypes.byref(t), ctypes.byref(r), ctypes.byref(b))
        return l.value, n.value, t.value, r.value, b.value

    # ---- Hogbom CLEAN of the dirty images (UpchanClean; include/xeng.h "Hogbom CLEAN of the dirty images"): a context of its own,
    # its kernel on the beamformer's stream
    def clean_initialize(self, gpu, nstand, nfine, nfavg, npix, niter_max):
        return self._lib.xengCleanInitialize(int(gpu), int(nstand), int(nfine), int(nfavg), int(npix), int(niter_max))

    def clean_set_geometry(self, tau, freq):
        """tau: host float64 [npix][nstand] seconds, freq: host float64 [nfine] Hz, both C-contiguous.  Waits for the context's work
        in flight."""
        _host_array("clean_set_geometry", "tau", tau, np.float64)
        _host_array("clean_set_geometry", "freq", freq, np.float64)
        pd = ctypes.POINTER(ctypes.c_double)
        return self._lib.xengCleanSetGeometry(tau.ctypes.data_as(pd), freq.ctypes.data_as(pd))

    def clean_set_weights(self, weights, autos):
        """weights: host float32 [nstand], finite and >= 0.  Waits for the context's work in flight; holds from the next run."""
        _host_array("clean_set_weights", "the weights", weights, np.float32)
        return self._lib.xengCleanSetWeights(_host_floats(weights), int(bool(autos)))

    def clean_set_window(self, mask):
        """mask: host uint8 [npix] (non-zero: a component may sit there), or None for every pixel.  Waits for the context's work in
        flight; holds from the next run."""
        if mask is None:
            return self._lib.xengCleanSetWindow(None)
        _host_array("clean_set_window", "the window", mask, np.uint8)
        return self._lib.xengCleanSetWindow(mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def clean_set_control(self, niter, gain, threshold, fraction):
        return self._lib.xengCleanSetControl(int(niter), float(gain), float(threshold), float(fraction))

    def clean_run(self, image_arr, out_arr):
        """Enqueue only: f32 [ngroup][4][npix] in; the residual, the component records and the stats out (clean_info gives the
        layout); clean_mark / wait cover it."""
        return self._enq.xengCleanRun(image_arr.ptr, out_arr.ptr)

    def clean_info(self):
        """(channel groups, pixels per work-group, comp_offset, stats_offset, span_bytes, norm)"""
        g, t, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        c, s, b = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengCleanGetInfo", ctypes.byref(g), ctypes.byref(t), ctypes.byref(c), ctypes.byref(s), ctypes.byref(b), ctypes.byref(n))
        return g.value, t.value, c.value, s.value, b.value, n.value

    # ---- outlier flags from the fine-channel visibilities (UpchanFlag; include/xeng.h "Outlier flags from the fine-channel
    # visibilities"): a context of its own, its kernels on the beamformer's stream
    def flag_initialize(self, gpu, nstand, nfine):
        return self._lib.xengFlagInitialize(int(gpu), int(nstand), int(nfine))

    def flag_set_weights(self, weights):
        """weights: host float32 [nstand], finite and >= 0, at least 4 of them > 0.  Waits for the context's work in flight; holds
        from the next run."""
        _host_array("flag_set_weights", "the weights", weights, np.float32)
        return self._lib.xengFlagSetWeights(_host_floats(weights))

    def flag_set_control(self, nsig_cross, nsig_auto, nsig_chan, wchan):
        return self._lib.xengFlagSetControl(float(nsig_cross), float(nsig_auto), float(nsig_chan), int(wchan))

    def flag_run(self, vis_arr, out_arr, stats_offset, chan_offset):
        """Enqueue only: cf32 [nfine][nstand][2][nstand][2] in; u8 [nfine][2][nstand] mask at the start of out_arr, f32
        [nfine][2][nstand][2] stats and f32 [nfine][2][4] chan `stats_offset` and `chan_offset` bytes into it; flag_mark / wait cover
        it."""
        return self._enq.xengFlagRun(vis_arr.ptr, out_arr.ptr, out_arr.ptr + int(stats_offset), out_arr.ptr + int(chan_offset))

    def flag_info(self):
        """(bytes of mask, of stats, of chan, the most LDS bytes of a work-group)"""
        m, s, c, l = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
        ffi.call("xengFlagGetInfo", ctypes.byref(m), ctypes.byref(s), ctypes.byref(c), ctypes.byref(l))
        return m.value, s.value, c.value, l.value

    def flag_control(self):
        """(nsig_cross, nsig_auto, nsig_chan, wchan) of the runs to come"""
        a, b, c, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        ffi.call("xengFlagGetControl", ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(w))
        return a.value, b.value, c.value, w.value

    # ---- component lists subtracted from the visibilities (UpchanPredict; include/xeng.h "Component lists subtracted from the
    # visibilities"): a context of its own, its kernels on the beamformer's stream
    PREDICT_SUBTRACT, PREDICT_MODEL = 0, 1

    def predict_initialize(self, gpu, nstand, nfine, nfavg, ndir, ncomp_max, cross):
        return self._lib.xengPredictInitialize(int(gpu), int(nstand), int(nfine), int(nfavg), int(ndir), int(ncomp_max), int(bool(cross)))

    def predict_set_geometry(self, tau, freq):
        """tau: host float64 [ndir][nstand] seconds, freq: host float64 [nfine] Hz, both C-contiguous.  Waits for the context's work
        in flight."""
        _host_array("predict_set_geometry", "tau", tau, np.float64)
        _host_array("predict_set_geometry", "freq", freq, np.float64)
        pd = ctypes.POINTER(ctypes.c_double)
        return self._lib.xengPredictSetGeometry(tau.ctypes.data_as(pd), freq.ctypes.data_as(pd))

    def predict_set_components(self, records):
        """records: host array of 32-byte records (blocks/imaging.py CLEAN_COMPONENT) [nfine / nfavg][ncomp_max], C-contiguous.
        Waits for the context's work in flight; holds from the next run."""
        if not (isinstance(records, np.ndarray) and records.dtype.itemsize == 32 and records.flags['C_CONTIGUOUS']):
            raise TypeError("predict_set_components: the records must be a C-contiguous array of 32-byte records")
        return self._lib.xengPredictSetComponents(records.ctypes.data_as(ctypes.c_void_p))

    def predict_set_mode(self, mode):
        return self._lib.xengPredictSetMode(int(mode))

    def predict_run(self, vis_arr, out_arr):
        """Enqueue only: cf32 [nfine][nstand][2][nstand][2] in and out (vis_arr may be None in model mode); predict_mark / wait cover
        it."""
        return self._enq.xengPredictRun(None if vis_arr is None else vis_arr.ptr, out_arr.ptr)

    def predict_info(self):
        """(tiles of 32 stands per side, work-groups per run, LDS bytes per work-group, bytes of a span, bytes of state, filled
        records, mode)"""
        t, g, l, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        b, s, n = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        ffi.call("xengPredictGetInfo", ctypes.byref(t), ctypes.byref(g), ctypes.byref(l), ctypes.byref(b), ctypes.byref(s), ctypes.byref(n), ctypes.byref(m))
        return t.value, g.value, l.value, b.value, s.value, n.value, m.value

    # ---- dedispersed transient search of the images (UpchanImageSearch; include/xeng.h "Dedispersed transient search of the
    # images"): a context of its own, its kernels on the beamformer's stream
    def imsearch_initialize(self, gpu, npix, ngroup, ndm, max_delay, nwidth, nstat):
        return self._lib.xengImsearchInitialize(int(gpu), int(npix), int(ngroup), int(ndm), int(max_delay), int(nwidth), int(nstat))

    def imsearch_set_delays(self, delays):
        """delays: host int32 [ndm][ngroup], C-contiguous, in integrations.  Waits for the context's work in flight; resets."""
        _host_array("imsearch_set_delays", "the table", delays, np.int32)
        return self._lib.xengImsearchSetDelays(delays.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    def imsearch_set_weights(self, weights):
        """weights: host float32 [ngroup], finite and >= 0, one above 0.  Waits for the context's work in flight; resets nothing,
        but no boxcar reaches back before this call."""
        _host_array("imsearch_set_weights", "the weights", weights, np.float32)
        return self._lib.xengImsearchSetWeights(_host_floats(weights))

    def imsearch_run(self, image_arr, out_arr):
        """Enqueue only: f32 [ngroup][4][npix] in, [npix] records {f32 snr, i16 idm, i16 iw} out; imsearch_mark / wait cover it."""
        return self._enq.xengImsearchRun(image_arr.ptr, out_arr.ptr)

    def imsearch_reset(self):
        """The next input counts as integration 0: no baseline, no delayed term, no boxcar reaches back (host state only)."""
        ffi.check("xengImsearchReset", self._enq.xengImsearchReset())

    def imsearch_info(self):
        """(integrations taken since the last reset, largest delay of the table in use or -1 without one)"""
        n, s = ctypes.c_longlong(), ctypes.c_int()
        ffi.call("xengImsearchGetInfo", ctypes.byref(n), ctypes.byref(s))
        return n.value, s.value

    def imsearch_baseline(self, ngroup, npix):
        """Waits for the context's work; (c, m, var) of the last complete block, float32 [ngroup][npix] each."""
        out = [np.empty((ngroup, npix), np.float32) for _ in range(3)]
        ffi.call("xengImsearchGetBaseline", *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in out])
        return tuple(out)

    # ---- completion tickets and guard bands of the engines of ffi.ENGINES, ffi.MORE_ENGINES, ffi.NEWER_ENGINES, ffi.NEWEST_ENGINES, ffi.LATEST_ENGINES, ffi.FURTHER_ENGINES, ffi.CUTOUT_ENGINES, ffi.RMSYNTH_ENGINES and ffi.TOA_ENGINES: <prefix>_mark / _wait / _ticket_done / _sync /
    # _guards_intact are made from these below the class
    def _mark(self, mark):
        t = ctypes.c_ulonglong()
        ffi.check(mark, getattr(self._enq, mark)(ctypes.byref(t)))
        return t.value

    def _ticket_done(self, ticket_done, ticket):
        d = ctypes.c_int()
        ffi.check(ticket_done, getattr(self._enq, ticket_done)(ctypes.c_ulonglong(ticket), ctypes.byref(d)))
        return bool(d.value)

    def _wait(self, ticket_done, wait, ticket):
        # ask first, without giving up the interpreter lock; only a ticket the GPU has not reached yet is worth a blocking call
        if not self._ticket_done(ticket_done, ticket):
            ffi.call(wait, ctypes.c_ulonglong(ticket))

    def _guards_intact(self, check_guards):
        ok = ctypes.c_int()
        ffi.call(check_guards, ctypes.byref(ok))
        return bool(ok.value)

    def last_error(self):
        return self._lib.xengGetLastError().decode()


def _engine_methods(cname, prefix, guards):
    """The HipBackend methods every row of ffi.ENGINES gets, by name."""
    x = "xeng" + cname

    def mark(self):
        return self._mark(x + "Mark")
    mark.__doc__ = "Ticket for everything enqueued in the %s context so far (%s_wait waits for it)." % (cname, prefix)

    def wait(self, ticket):
        self._wait(x + "TicketDone", x + "Wait", ticket)
    wait.__doc__ = "Returns when everything enqueued before %s_mark gave `ticket` has completed." % prefix

    def ticket_done(self, ticket):
        return self._ticket_done(x + "TicketDone", ticket)
    ticket_done.__doc__ = "Never blocks: whether everything enqueued before the ticket has completed."

    def sync(self):
        ffi.call(x + "Sync")
    sync.__doc__ = "Waits for everything enqueued in the %s context." % cname

    def guards_intact(self):
        return self._guards_intact(x + "CheckGuards")
    guards_intact.__doc__ = "Waits for the context's work; True while the guard bands around the %s state hold their pattern." % cname

    fs = {"mark": mark, "wait": wait, "ticket_done": ticket_done, "sync": sync}
    if guards:
        fs["guards_intact"] = guards_intact
    return {"%s_%s" % (prefix, k): f for k, f in fs.items()}


for _row in ffi.ENGINES + ffi.MORE_ENGINES + ffi.NEWER_ENGINES + ffi.NEWEST_ENGINES + ffi.LATEST_ENGINES + ffi.FURTHER_ENGINES + ffi.CUTOUT_ENGINES + ffi.RMSYNTH_ENGINES + ffi.TOA_ENGINES:
    for _name, _f in _engine_methods(*_row).items():
        _f.__name__ = _name
        _f.__qualname__ = "HipBackend." + _name
        setattr(HipBackend, _name, _f)


_default = None


def default_backend():
    global _default
    if _default is None:
        _default = HipBackend()
    return _default
