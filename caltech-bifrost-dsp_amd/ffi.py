"""ctypes binding of libxeng.so (include/xeng.h) -- the product's only route to the GPU.

This plays the role of `from bifrost.libbifrost import _bf` in the reference blocks
(corr_block.py:5, beamform_block.py:5).  There is no CPU fallback: if the HIP library is
missing or fails to load, importing `lib()` raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# XENG_LIB: load another build of the same library (the -DXENG_DIAGNOSTICS build used by profiles/: host-side diagnostic switches)
LIB_PATH = os.environ.get("XENG_LIB") or os.path.join(_HERE, "libxeng.so")

STATUS_SUCCESS = 0
SPACE_SYSTEM, SPACE_CUDA, SPACE_CUDA_HOST = 1, 2, 3

_lib = None


class XengError(RuntimeError):
    def __init__(self, fn, status, msg):
        super().__init__("%s returned %d: %s" % (fn, status, msg))
        self.status = status


class XENGarray(ctypes.Structure):
    """Mirror of include/xeng.h XENGarray (= bifrost BFarray)."""
    _fields_ = [("data", ctypes.c_void_p), ("space", ctypes.c_int), ("dtype", ctypes.c_int),
                ("ndim", ctypes.c_int), ("shape", ctypes.c_long * 8), ("strides", ctypes.c_long * 8),
                ("immutable", ctypes.c_int), ("big_endian", ctypes.c_int), ("conjugated", ctypes.c_int)]


class XengStamp(ctypes.Structure):
    """include/xeng.h xengStamp: everything the library has enqueued so far (opaque)."""
    _fields_ = [("w", ctypes.c_ulonglong * 16)]


STATUS_WOULD_BLOCK, STATUS_END_OF_DATA = 6, 7
STREAMS = {"xgpu": 1, "map": 2, "beam": 4, "copy": 8, "consumer": 16, "xgpu_out": 32}       # include/xeng.h XENG_STREAMS_*
# test hooks of the span rings (xengRingSetStampHooks)
STAMP_NOW_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong))
STAMP_DONE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong))
STAMP_WAIT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong))

# every symbol include/xeng.h declares: name -> argtypes (all return int unless noted)
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
_pi = ctypes.POINTER(ctypes.c_int)
_pa = ctypes.POINTER(XENGarray)
_ll, _pll, _psz, _pvp = ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p)
_pst = ctypes.POINTER(XengStamp)
SYMBOLS = {
    "xengStampNow": [_pst], "xengStampNowFor": [_pst, _vp, ctypes.c_uint], "xengStampDone": [_pst, _pi, _pi], "xengStampWait": [_pst],
    "xengRingCreate": [_pvp, ctypes.c_char_p, _i], "xengRingDestroy": [_vp], "xengRingResize": [_vp, _sz, _sz], "xengRingSetRecycle": [_vp, _i], "xengRingDeclareStreams": [_vp, ctypes.c_uint], "xengRingGetStampClasses": [_vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)],
    "xengRingGetInfo": [_vp, _psz, _psz, _psz, _pi, _pll, ctypes.POINTER(ctypes.c_ulonglong)],
    "xengRingBeginSequence": [_vp, _ll, ctypes.c_char_p, _sz, _i, _pll], "xengRingEndSequence": [_vp, _ll], "xengRingEndWriting": [_vp],
    "xengRingReserve": [_vp, _ll, _sz, _i, _i, _pvp, _pll], "xengRingCommit": [_vp, _ll, _ll, _sz],
    "xengRingCommitExternal": [_vp, _ll, _vp, _sz, _i],
    "xengRingOpenReader": [_vp, _i, _pi], "xengRingCloseReader": [_vp, _i],
    "xengRingNextSequence": [_vp, _i, _i, _pll, _pll, _pi, _pvp, _psz],
    "xengRingAcquire": [_vp, _i, _sz, _sz, _i, _pvp, _psz, _pll, _psz], "xengRingSpanRelease": [_ll],
    "xengRingAcquireParts": [_vp, _i, _sz, _sz, _i, _pvp, _psz, _pll, _pi, _psz],
    "xengRingSetStampHooks": [_vp, STAMP_NOW_FN, STAMP_DONE_FN, STAMP_WAIT_FN, _vp],
    "xengGetDeviceCount": [_pi], "xengSetDevice": [_i], "xengGetDevice": [_pi], "xengDeviceSynchronize": [],
    "xengGetDeviceInfo": [_i, _pi, _pi, ctypes.POINTER(_sz), ctypes.c_char_p, _i], "xengGetDevicePciBusId": [_i, ctypes.c_char_p, _i],
    "xengMalloc": [ctypes.POINTER(_vp), _sz, _i], "xengFree": [_vp, _i], "xengMemcpy": [_vp, _vp, _sz],
    "xengMemcpyAsync": [_vp, _vp, _sz], "xengMemset": [_vp, _i, _sz], "xengStreamSynchronize": [],
    "xengXgpuConfigure": [_i, _i, _i, _i, _i], "xengXgpuInitialize": [_i], "xengXgpuDestroy": [],
    "xengXgpuKernel": [_vp, _vp, _i], "xengXgpuKernelAsync": [_vp, _vp, _i], "xengXgpuKernelAsyncAcc": [_vp, _vp, _i, _vp, _i], "xengXgpuTryKernelAsyncAcc": [_vp, _vp, _i, _vp, _i], "xengXgpuWaitLaunchSlot": [],
    "xengXgpuKernelAsyncSlab": [_vp, _i, _sz, ctypes.c_uint64, _i, _vp, _i, _vp, _i], "xengXgpuTryKernelAsyncSlab": [_vp, _i, _sz, ctypes.c_uint64, _i, _vp, _i, _vp, _i], "xengXgpuGetSlabFallbacks": [_pi], "xengXgpuGetSlabStats": [_pi, _pi], "xengXgpuSync": [], "xengXgpuSyncLag": [_i], "xengXgpuDumpDone": [_i, _pi], "xengXgpuReset": [],
    "xengXgpuCorrelate": [_vp, _vp, _i], "xengXgpuGetOrder": [_vp, _vp, _vp],
    "xengXgpuSubSelect": [_vp, _vp, _vp, _vp, _i, _i], "xengXgpuReorder": [_vp, _vp, _vp, _vp],
    "xengXgpuGetInfo": [_pi, _pi, _pi, _pi, ctypes.POINTER(ctypes.c_int64), _pi],
    "xengXgpuGetPath": [_pi, _pi], "xengXgpuGetKernel": [_pi, _pi],
    "xengXgpuPacketize": [_vp, _vp, _vp, _vp, _i],
    "xengSnap2Unpack": [_vp, _i, ctypes.c_size_t, _vp, ctypes.c_uint64, _i, _i, _i, _i, _i, _pi, _pi],
    "xengSnap2UnpackAsync": [_vp, _i, ctypes.c_size_t, _vp, ctypes.c_uint64, _i, _i, _i, _i, _i],
    "xengSnap2GetAsyncDrops": [_pi], "xengSnap2StampSeq": [_vp, _i, _sz, ctypes.c_uint64, _i],
    "xengXgpuSetProfiling": [_i], "xengXgpuGetTimes": [ctypes.POINTER(ctypes.c_double), _pi],
    "xengMapAssignI32": [_vp, _vp, _sz], "xengMapAddI32": [_vp, _vp, _sz], "xengMapSync": [],
    "xengMapSumI32": [_vp, _pvp, _i, _sz, _i],
    "xengBeamformInitialize": [_i, _i, _i, _i, _i, _i], "xengBeamformDestroy": [],
    "xengBeamformRun": [_vp, _vp, _vp], "xengBeamformRunVersioned": [_vp, _vp, _vp, ctypes.c_longlong], "xengBeamformTryRunVersioned": [_vp, _vp, _vp, ctypes.c_longlong],
    "xengBeamformRunParts": [_vp, _i, _vp, _vp, _vp, ctypes.c_longlong], "xengBeamformTryRunParts": [_vp, _i, _vp, _vp, _vp, ctypes.c_longlong],
    "xengBeamformRunSlabs": [_vp, _i, _i, _vp, _i, _sz, ctypes.c_uint64, _i, _vp, _vp, ctypes.c_longlong], "xengBeamformTryRunSlabs": [_vp, _i, _i, _vp, _i, _sz, ctypes.c_uint64, _i, _vp, _vp, ctypes.c_longlong], "xengBeamformGetSlabFallbacks": [_pi], "xengBeamformGetSlabStats": [_pi, _pi],
    "xengBeamformIntegrate": [_vp, _vp, _i],
    "xengBeamformIntegrateSingleBeam": [_vp, _vp, _i, _i], "xengBeamformMark": [ctypes.POINTER(ctypes.c_ulonglong)], "xengBeamformWait": [ctypes.c_ulonglong], "xengBeamformTicketDone": [ctypes.c_ulonglong, _pi], "xengBeamformSync": [],
    "xengBeamformPacketizeVoltages": [_vp, _vp, _i, _i, _i, _i, _i, _sz, _i, _i, _i, _i, _i, ctypes.c_uint64],
    "xengBeamformSetProfiling": [_i], "xengBeamformGetTimes": [ctypes.POINTER(ctypes.c_double), _pi],
    "xengBeamformGetRouteInfo": [_pi, _pi, _pi],
    "xengUpchanInitialize": [_i, _i, _i, _i, _i, _i, _i], "xengUpchanInitializeDualPol": [_i, _i, _i, _i, _i, _i, _i], "xengUpchanRun": [_vp, _vp, _vp, _ll], "xengUpchanRunParts": [_vp, _i, _vp, _vp, _vp, _ll],
    # (the engines on the beamformer's stream: their Mark / Wait / TicketDone / Sync / Destroy / CheckGuards come from ENGINES below)
    "xengUpchanSetPfb": [_i, ctypes.POINTER(ctypes.c_float)], "xengUpchanReset": [],
    "xengUpchanCorrInitialize": [_i, _i, _i, _i, _i, _i, _i, _i], "xengUpchanCorrGetInfo": [_pi, _pi],
    "xengUpchanCorrAccumulate": [_vp], "xengUpchanCorrAccumulateParts": [_vp, _i, _vp], "xengUpchanCorrDump": [_vp], "xengUpchanCorrReset": [],
    "xengUpchanCorrSetPfb": [_i, ctypes.POINTER(ctypes.c_float)],
    "xengUpchanCorrPrime": [_vp], "xengUpchanCorrPrimeParts": [_vp, _i, _vp],
    "xengUpchanSumBeamsInitialize": [_i, _i, _i, _i, _i, _i, _i, _i], "xengUpchanSumBeamsGetInfo": [_pi, _pi, _pi],
    "xengUpchanSumBeamsRun": [_vp, _vp], "xengUpchanSumBeamsSetPfb": [_i, ctypes.POINTER(ctypes.c_float)], "xengUpchanSumBeamsPrime": [_vp],
    "xengUpchanSumBeamsReset": [],
    "xengUpchanSpectraInitialize": [_i, _i, _i, _i, _i, _i], "xengUpchanSpectraGetInfo": [_pi, _pi, _pi],
    "xengUpchanSpectraRun": [_vp, _vp], "xengUpchanSpectraRunParts": [_vp, _i, _vp, _vp], "xengUpchanSpectraSetPfb": [_i, ctypes.POINTER(ctypes.c_float)],
    "xengUpchanSpectraPrime": [_vp], "xengUpchanSpectraPrimeParts": [_vp, _i, _vp], "xengUpchanSpectraReset": [],
    "xengDedispInitialize": [_i, _i, _i, _i, _i, _i, _i], "xengDedispSetDelays": [_pi], "xengDedispSetWeights": [ctypes.POINTER(ctypes.c_float)],
    "xengDedispRun": [_vp, _i, _vp], "xengDedispReset": [], "xengDedispGetInfo": [_pi, ctypes.POINTER(ctypes.c_longlong)],
    "xengPulseInitialize": [_i, _i, _i, _i, _i, _i, _i], "xengPulseRun": [_vp, _i, _vp], "xengPulseReset": [],
    "xengPulseGetInfo": [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)],
    "xengPulseGetBaseline": [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)],
    "xengFoldInitialize": [_i, _i, _i, _i, _i, _i],
    "xengFoldSetPhase": [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong), _pll, ctypes.POINTER(ctypes.c_ubyte), _ll],
    "xengFoldSetRotations": [_pi], "xengFoldSetWeights": [ctypes.POINTER(ctypes.c_float)], "xengFoldRun": [_vp, _i],
    "xengFoldDump": [_vp, ctypes.POINTER(ctypes.c_uint), _i, _i, _i], "xengFoldReset": [], "xengFoldGetInfo": [_pll, _pll],
    "xengPeriodInitialize": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i], "xengPeriodSetMask": [ctypes.POINTER(ctypes.c_ubyte)],
    "xengPeriodRun": [_vp, _i, _vp, _pi], "xengPeriodReset": [], "xengPeriodGetInfo": [_pll, _pi, _pll],
    "xengPeriodGetSpectrum": [ctypes.POINTER(ctypes.c_float), _pi],
    "xengPlongInitialize": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _pi], "xengPlongSetMask": [ctypes.POINTER(ctypes.c_ubyte)],
    "xengPlongRun": [_vp, _i, _vp, _pi], "xengPlongReset": [], "xengPlongGetInfo": [_pll, _pi, _pll],
    "xengPlongGetSpectrum": [_i, _i, ctypes.POINTER(ctypes.c_float), _pi], "xengPlongSetBatch": [_i], "xengPlongGetBatch": [_pi, _pi],
    "xengAccelInitialize": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _pi, _i, ctypes.POINTER(ctypes.c_double)], "xengAccelSetMask": [ctypes.POINTER(ctypes.c_ubyte)],
    "xengAccelRun": [_vp, _i, _vp, _pi], "xengAccelReset": [], "xengAccelGetInfo": [_pll, _pll],
    "xengAccelGetTrialRecords": [_i, _i, _vp], "xengAccelSetBatch": [_i], "xengAccelGetBatch": [_pi, _pi],
    "xengFfaInitialize": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i], "xengFfaRun": [_vp, _i, _vp, _pi], "xengFfaReset": [],
    "xengFfaGetInfo": [_pll, _pll], "xengFfaGetStats": [ctypes.POINTER(ctypes.c_float)],
    "xengCandfoldInitialize": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _pi, _pi, ctypes.POINTER(ctypes.c_float)],
    "xengCandfoldSetCandidates": [_i, _pi, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong), _pll, ctypes.POINTER(ctypes.c_ubyte)],
    "xengCandfoldRun": [_vp, _i, _vp, _pi], "xengCandfoldReset": [], "xengCandfoldGetInfo": [_pll, _pll],
    "xengCandfoldGetCube": [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint)],
    "xengRfiInitialize": [_i, _i, _i, _i, _i], "xengRfiSetControl": [ctypes.c_float, ctypes.c_float, ctypes.c_float, _i, _i],
    "xengRfiSetMask": [ctypes.POINTER(ctypes.c_ubyte)], "xengRfiRun": [_vp, _i, _vp, _vp, _pi], "xengRfiReset": [], "xengRfiGetInfo": [_pll, _pll],
    "xengRfiGetBlock": [ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                        ctypes.POINTER(ctypes.c_float)],
    "xengDetrendInitialize": [_i, _i, _i, _i, _i, _i, _i, ctypes.c_float], "xengDetrendRun": [_vp, _i, _vp, _pi], "xengDetrendReset": [],
    "xengDetrendGetInfo": [_pll, _pll], "xengDetrendGetKnots": [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)],
    "xengCutoutInitialize": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.c_float], "xengCutoutSetDelays": [_pi],
    "xengCutoutSetWeights": [ctypes.POINTER(ctypes.c_float)], "xengCutoutRequest": [_i, _vp], "xengCutoutRun": [_vp, _i, _vp, _pi, _pi, _pi, _pi],
    "xengCutoutReset": [], "xengCutoutGetInfo": [_pll, _pi, _pll],
    "xengRmsynthInitialize": [_i, _i, _i, _i, _i, _i], "xengRmsynthSetTable": [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)],
    "xengRmsynthSetMasks": [ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_ubyte)], "xengRmsynthSetActive": [ctypes.POINTER(ctypes.c_ubyte)],
    "xengRmsynthRun": [_vp, _vp], "xengRmsynthReset": [], "xengRmsynthGetInfo": [_pll, _pi, _pll, _pll, _pll],
    "xengToaInitialize": [_i, _i, _i, _i, _i, _i, _i, _i], "xengToaSetBands": [_pi, ctypes.POINTER(ctypes.c_float)],
    "xengToaSetTables": [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)], "xengToaSetTemplate": [ctypes.POINTER(ctypes.c_float)],
    "xengToaSetMask": [ctypes.POINTER(ctypes.c_ubyte)], "xengToaSetActive": [ctypes.POINTER(ctypes.c_ubyte)],
    "xengToaRun": [_vp, _vp], "xengToaReset": [], "xengToaGetInfo": [_pll, _pi, _pll, _pll, _pll, _pll],
    "xengCdedispInitialize": [_i, _i, _i, _i, _i, _i, _i, _i], "xengCdedispSetChirp": [ctypes.POINTER(ctypes.c_float)],
    "xengCdedispRun": [_vp, _vp, _pi], "xengCdedispReset": [], "xengCdedispGetInfo": [_pi, _pi, _pll, _pll],
    "xengCdlongInitialize": [_i, _i, _i, _i, _i, _i, _i, _i], "xengCdlongSetChirp": [_i, ctypes.POINTER(ctypes.c_float)],
    "xengCdlongRun": [_vp, _vp, _pi], "xengCdlongReset": [], "xengCdlongGetInfo": [_pi, _pi, _pll, _pll],
    "xengImageInitialize": [_i, _i, _i, _i, _i], "xengImageGetInfo": [_pi, _pi, _pi, ctypes.POINTER(ctypes.c_double)],
    "xengImageSetGeometry": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)], "xengImageSetWeights": [ctypes.POINTER(ctypes.c_float), _i],
    "xengImageRun": [_vp, _vp],
    "xengGaincalInitialize": [_i, _i, _i, _i], "xengGaincalGetInfo": [_pi, _pi, ctypes.POINTER(ctypes.c_double), _pi],
    "xengGaincalSetModel": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)],
    "xengGaincalSetWeights": [ctypes.POINTER(ctypes.c_float), _i], "xengGaincalSetSolver": [_i, ctypes.c_double], "xengGaincalRun": [_vp, _vp, _vp, _i],
    "xengCalapplyInitialize": [_i, _i, _i, _i], "xengCalapplyGetInfo": [_pi, _pi, _pi, _pll],
    "xengCalapplySetModel": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)],
    "xengCalapplySetFactors": [_vp], "xengCalapplyRun": [_vp, _vp],
    "xengPeelInitialize": [_i, _i, _i, _i], "xengPeelGetInfo": [_pi, _pi, ctypes.POINTER(ctypes.c_double), _pi, _pll],
    "xengPeelSetModel": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)],
    "xengPeelSetWeights": [ctypes.POINTER(ctypes.c_float), _i], "xengPeelSetSolver": [_i, ctypes.c_double], "xengPeelRun": [_vp, _vp, _vp, _vp, _i],
    "xengCleanInitialize": [_i, _i, _i, _i, _i, _i], "xengCleanGetInfo": [_pi, _pi, _pll, _pll, _pll, ctypes.POINTER(ctypes.c_double)],
    "xengCleanSetGeometry": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)], "xengCleanSetWeights": [ctypes.POINTER(ctypes.c_float), _i],
    "xengCleanSetWindow": [ctypes.POINTER(ctypes.c_ubyte)], "xengCleanSetControl": [_i, ctypes.c_float, ctypes.c_float, ctypes.c_float],
    "xengCleanRun": [_vp, _vp],
    "xengFlagInitialize": [_i, _i, _i], "xengFlagGetInfo": [_pll, _pll, _pll, _pi], "xengFlagSetWeights": [ctypes.POINTER(ctypes.c_float)],
    "xengFlagSetControl": [ctypes.c_double, ctypes.c_double, ctypes.c_double, _i],
    "xengFlagGetControl": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), _pi],
    "xengFlagRun": [_vp, _vp, _vp, _vp],
    "xengPredictInitialize": [_i, _i, _i, _i, _i, _i, _i], "xengPredictGetInfo": [_pi, _pi, _pi, _pll, _pll, _pll, _pi],
    "xengPredictSetGeometry": [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)], "xengPredictSetComponents": [_vp], "xengPredictSetMode": [_i],
    "xengPredictRun": [_vp, _vp],
    "xengImsearchInitialize": [_i, _i, _i, _i, _i, _i, _i], "xengImsearchSetDelays": [_pi], "xengImsearchSetWeights": [ctypes.POINTER(ctypes.c_float)],
    "xengImsearchRun": [_vp, _vp], "xengImsearchReset": [], "xengImsearchGetInfo": [_pll, _pi],
    "xengImsearchGetBaseline": [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)],
    "bfXgpuInitialize": [_pa, _pa, _i], "bfXgpuKernel": [_pa, _pa, _i], "bfXgpuCorrelate": [_pa, _pa, _i],
    "bfXgpuGetOrder": [_pa, _pa, _pa], "bfXgpuSubSelect": [_pa, _pa, _pa, _pa, _i, _i],
    "bfXgpuReorder": [_pa, _pa, _pa, _pa], "bfBeamformInitialize": [_i, _i, _i, _i, _i, _i],
    "bfBeamformRun": [_pa, _pa, _pa], "bfBeamformIntegrate": [_pa, _pa, _i],
    "bfBeamformIntegrateSingleBeam": [_pa, _pa, _i, _i],
}
STRING_SYMBOLS = ["xengGetLastError", "xengVersion"]

# The engines on the beamformer's stream (csrc/xeng_common.h BeamStreamContext): (C name, HipBackend prefix, has CheckGuards).
# Every one has xeng<C name>Mark / Wait / TicketDone / Sync / Destroy with the same prototypes, and HipBackend gets
# <prefix>_mark / _wait / _ticket_done / _sync (and _guards_intact) from its row (backend.py).  The beamformer itself has a
# native binding and is not listed.
ENGINES = [("Upchan", "upchan", False), ("UpchanCorr", "upchan_corr", False), ("UpchanSumBeams", "upchan_sum_beams", False),
           ("UpchanSpectra", "upchan_spectra", False), ("Dedisp", "dedisp", True), ("Pulse", "pulse", True), ("Fold", "fold", True),
           ("Period", "period", True), ("Ffa", "ffa", True), ("Cdedisp", "cdedisp", True), ("Cdlong", "cdlong", True),
           ("Image", "image", True), ("Gaincal", "gaincal", True), ("Calapply", "calapply", True), ("Peel", "peel", True),
           ("Clean", "clean", True), ("Flag", "flag", True), ("Predict", "predict", True), ("Imsearch", "imsearch", True)]
# Engines added since tests/test_engine_table_cpu.py pinned the length of ENGINES: rows of the same kind, treated the same everywhere.
MORE_ENGINES = [("Plong", "plong", True)]
# ... and since tests/test_plong_cpu.py pinned MORE_ENGINES
NEWER_ENGINES = [("Accel", "accel", True)]
# ... and since tests/test_accel_cpu.py pinned NEWER_ENGINES
NEWEST_ENGINES = [("Candfold", "candfold", True)]
# ... and since tests/test_candfold_cpu.py pinned NEWEST_ENGINES
LATEST_ENGINES = [("Rfi", "rfi", True)]
# ... and since tests/test_rfi_cpu.py pinned LATEST_ENGINES
FURTHER_ENGINES = [("Detrend", "detrend", True)]
# ... and since tests/test_detrend_cpu.py pinned FURTHER_ENGINES
CUTOUT_ENGINES = [("Cutout", "cutout", True)]
# ... and since tests/test_cutout_cpu.py pinned CUTOUT_ENGINES
RMSYNTH_ENGINES = [("Rmsynth", "rmsynth", True)]
# ... and since tests/test_rmsynth_cpu.py pinned RMSYNTH_ENGINES
TOA_ENGINES = [("Toa", "toa", True)]
for _c, _prefix, _guards in ENGINES + MORE_ENGINES + NEWER_ENGINES + NEWEST_ENGINES + LATEST_ENGINES + FURTHER_ENGINES + CUTOUT_ENGINES + RMSYNTH_ENGINES + TOA_ENGINES:
    SYMBOLS.update({"xeng%sMark" % _c: [ctypes.POINTER(ctypes.c_ulonglong)], "xeng%sWait" % _c: [ctypes.c_ulonglong],
                    "xeng%sTicketDone" % _c: [ctypes.c_ulonglong, _pi], "xeng%sSync" % _c: [], "xeng%sDestroy" % _c: []})
    if _guards:
        SYMBOLS["xeng%sCheckGuards" % _c] = [_pi]


def lib():
    """Load libxeng.so (once).  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(or make -C caltech-bifrost-dsp_amd/csrc). There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, args in SYMBOLS.items():
            if os.environ.get("XENG_LIB") and not hasattr(L, name):
                continue            # (an older build loaded for an A/B by profiles/: calling what it lacks raises AttributeError there)
            f = getattr(L, name)
            f.argtypes = args
            f.restype = ctypes.c_int
        for name in STRING_SYMBOLS:
            getattr(L, name).restype = ctypes.c_char_p
            getattr(L, name).argtypes = []
        _lib = L
    return _lib


# Enqueue-only entry points (and the two completion queries): a few microseconds of host work, nothing to wait for.  The block threads call them through a
# second handle on the same library that does NOT release the interpreter lock around the call (ctypes.PyDLL): a thread that
# gives the lock up for a 3 us call has to win it back afterwards, and with several block threads in one interpreter that
# costs a sleep and a wake-up -- measured 50 us per call on the GPU box (profiles/r03/blocks_lock_handoff.txt), more than the
# GPU needs for the gulp.  Calls that wait (Sync, Wait, the synchronous X-engine call, copies) stay on the releasing handle.
# (Round 4: the list holds only calls that cannot wait by construction.  xengXgpuKernelAsync[Acc] wait at 256 launches in
# flight and xengBeamformRun* waits once after a weight upload in the integrated-power mode: their Try* forms return
# XENG_STATUS_WOULD_BLOCK instead, and the caller gives the lock up to wait; xengSnap2UnpackAsync shares a mutex with the
# synchronous call, which polls: it is made on the releasing handle.)
ENQUEUE_ONLY = ["xengXgpuTryKernelAsyncAcc", "xengXgpuTryKernelAsyncSlab", "xengBeamformTryRunVersioned", "xengBeamformTryRunParts", "xengBeamformTryRunSlabs",
                "xengBeamformIntegrate", "xengBeamformIntegrateSingleBeam", "xengBeamformPacketizeVoltages", "xengBeamformMark",
                "xengUpchanRun", "xengUpchanRunParts", "xengUpchanCorrAccumulate",
                "xengUpchanCorrAccumulateParts", "xengUpchanCorrDump", "xengUpchanCorrReset", "xengMapAssignI32",
                "xengUpchanReset", "xengUpchanCorrPrime", "xengUpchanCorrPrimeParts",
                "xengUpchanSumBeamsRun", "xengUpchanSumBeamsPrime", "xengUpchanSumBeamsReset",
                "xengUpchanSpectraRun", "xengUpchanSpectraRunParts", "xengUpchanSpectraPrime", "xengUpchanSpectraPrimeParts", "xengUpchanSpectraReset",
                "xengDedispRun", "xengDedispReset", "xengPulseRun", "xengPulseReset", "xengFoldRun", "xengFoldReset", "xengPeriodRun", "xengPeriodReset",
                "xengPlongRun", "xengPlongReset", "xengAccelRun", "xengAccelReset",
                "xengFfaRun", "xengFfaReset", "xengCandfoldRun", "xengCandfoldReset", "xengRfiRun", "xengRfiReset", "xengDetrendRun", "xengDetrendReset", "xengCutoutRun", "xengCutoutReset", "xengCutoutRequest", "xengRmsynthRun", "xengRmsynthReset", "xengToaRun", "xengToaReset", "xengCdedispRun", "xengCdedispReset", "xengCdlongRun", "xengCdlongReset",
                "xengImageRun", "xengGaincalRun", "xengCalapplyRun", "xengPeelRun", "xengCleanRun", "xengFlagRun", "xengPredictRun",
                "xengImsearchRun", "xengImsearchReset",
                "xengMapAddI32", "xengMapSumI32", "xengXgpuDumpDone", "xengBeamformTicketDone", "bfBeamformIntegrate", "bfBeamformIntegrateSingleBeam",
                # the span rings: bookkeeping calls, and the calls that can wait asked with may_block = 0 first
                "xengRingBeginSequence", "xengRingEndSequence", "xengRingEndWriting", "xengRingReserve", "xengRingCommit",
                "xengRingCommitExternal", "xengRingNextSequence", "xengRingAcquire", "xengRingAcquireParts", "xengRingSpanRelease", "xengRingGetInfo",
                "xengRingOpenReader", "xengRingCloseReader", "xengRingResize",
                "xengStampNow", "xengStampNowFor", "xengStampDone", "xengGetDevice", "xengSetDevice"]
for _c, _prefix, _guards in ENGINES + MORE_ENGINES + NEWER_ENGINES + NEWEST_ENGINES + LATEST_ENGINES + FURTHER_ENGINES + CUTOUT_ENGINES + RMSYNTH_ENGINES + TOA_ENGINES:     # an event record and an event query: neither can wait
    ENQUEUE_ONLY += ["xeng%sMark" % _c, "xeng%sTicketDone" % _c]
_enq = None


def enqueue_lib():
    """The same libxeng.so, bound without releasing the interpreter lock; only the ENQUEUE_ONLY symbols are typed."""
    global _enq
    if _enq is None:
        lib()                                   # (raises when the extension is missing)
        E = ctypes.PyDLL(LIB_PATH)
        for name in ENQUEUE_ONLY:
            f = getattr(E, name)
            f.argtypes = SYMBOLS[name]
            f.restype = ctypes.c_int
        _enq = E
    return _enq


def check(name, status):
    if status != STATUS_SUCCESS:
        raise XengError(name, status, lib().xengGetLastError().decode())


def call(name, *args):
    check(name, getattr(lib(), name)(*args))


class DeviceBuffer:
    """A HIP allocation (space 'cuda') or pinned host allocation ('cuda_host')."""

    def __init__(self, nbytes, space=SPACE_CUDA):
        self.nbytes = int(nbytes)
        self.space = space
        p = ctypes.c_void_p()
        call("xengMalloc", ctypes.byref(p), self.nbytes, space)
        self.ptr = p.value

    def free(self):
        if self.ptr:
            call("xengFree", self.ptr, self.space)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        call("xengMemcpy", self.ptr + offset, arr.ctypes.data, arr.nbytes)
        return self

    def download(self, dtype, count=None, offset=0):
        dtype = np.dtype(dtype)
        if count is None:
            count = (self.nbytes - offset) // dtype.itemsize
        out = np.empty(count, dtype=dtype)
        call("xengMemcpy", out.ctypes.data, self.ptr + offset, out.nbytes)
        return out

    def as_host_array(self, dtype):
        assert self.space == SPACE_CUDA_HOST
        dtype = np.dtype(dtype)
        buf = (ctypes.c_char * self.nbytes).from_address(self.ptr)
        buf._owner = self
        return np.frombuffer(buf, dtype=dtype)


def device_count():
    n = ctypes.c_int(0)
    call("xengGetDeviceCount", ctypes.byref(n))
    return n.value


def device_pci_bus_id(gpu=0):
    buf = ctypes.create_string_buffer(32)
    call("xengGetDevicePciBusId", gpu, buf, 32)
    return buf.value.decode().lower()


def device_info(gpu=0):
    cu, clk, mem = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    name = ctypes.create_string_buffer(128)
    call("xengGetDeviceInfo", gpu, ctypes.byref(cu), ctypes.byref(clk), ctypes.byref(mem), name, 128)
    return {"num_cu": cu.value, "clock_khz": clk.value, "total_mem": mem.value, "name": name.value.decode()}
