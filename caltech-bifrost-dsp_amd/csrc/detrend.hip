// Host side of the baseline removal of the dedispersed beams (BeamDetrend; detrend_kernels.h): a process-global context of its own
// on the beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "detrend_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct DetrendContext : BeamStreamContext {
    int npair = 0, ndm = 0, nwin = 0, nprod = 0, nblk = 0, normalise = 0;
    int nser = 0;                       // npair * ndm
    int D = 0;                          // 3 nblk / 2, the latency in windows
    int L = 0;                          // D + nwin, slots of the ring per series
    float k_mad = 0.f;
    float r = 0.f;                      // 1.0f / (float)(2 nblk)
    GuardedState alloc;                 // the state between its guard bands (xengDetrendCheckGuards)
    float* ring = nullptr;              // [nser][L]
    DetrendKnots kn = {};               // block k in slot k & 3
    long long nwindows = 0;             // windows taken since the last reset
    long long nblocks = 0;              // blocks decided since the last reset

    static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
    size_t ring_bytes() const { return up16((size_t)nser * L * 4); }
    size_t table_bytes() const { return up16((size_t)DT_KNOTS * nser * 4); }
    size_t state_bytes() const { return ring_bytes() + 3 * table_bytes() + up16((size_t)DT_KNOTS * nser); }
};
static std::mutex g_dtmu;
static DetrendContext g_dt;

static int detrend_destroy_locked() {
    if (!g_dt.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_dt);
    g_dt.alloc.free();
    g_dt = DetrendContext();
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengDetrendInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nblk, int normalise, float k_mad) {
    if (npair < 1 || ndm < 1 || (long long)npair * ndm > (1LL << 24))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: %d pairs x %d trials, not 1 to 2^24 series", npair, ndm);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: %d products, not 1 or 4", nprod);
    if (nblk < 4 || nblk > 8192 || (nblk & 1)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: blocks of %d windows, not an even number from 4 to 8192", nblk);
    if (nwin < 1 || nwin > nblk) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: %d windows a call, not 1 to nblk = %d", nwin, nblk);
    if (normalise != 0 && normalise != 1) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: normalise %d, not 0 or 1", normalise);
    if (!std::isfinite(k_mad) || !(k_mad > 0.f)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: k_mad %g is not finite and positive", k_mad);
    DetrendContext y;
    y.npair = npair; y.ndm = ndm; y.nwin = nwin; y.nprod = nprod; y.nblk = nblk; y.normalise = normalise;
    y.nser = npair * ndm;
    y.D = 3 * (nblk / 2);
    y.L = y.D + nwin;
    y.k_mad = k_mad;
    y.r = 1.0f / (float)(2 * nblk);
    const unsigned long long hist = (unsigned long long)y.L * y.nser * 4;
    if (hist >= (unsigned long long)XENG_DETREND_MAX_HISTORY_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: a history of %d + %d windows of %d series needs %.3g GB, the limit is %.3g GB", y.D, nwin, y.nser,
                  (double)hist * 1e-9, (double)XENG_DETREND_MAX_HISTORY_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_dtmu);
    detrend_destroy_locked();
    DetrendContext& x = g_dt;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    y.gpu = x.gpu;
    y.stream = x.stream;
    x = y;
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = DetrendContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Detrend: cannot allocate %.3g MB of state", (double)y.state_bytes() * 1e-6);
    }
    char* p = (char*)x.alloc.data();    // (every piece starts at a multiple of 16 bytes)
    x.ring = (float*)p; p += x.ring_bytes();
    x.kn.M = (float*)p; p += x.table_bytes();
    x.kn.A = (float*)p; p += x.table_bytes();
    x.kn.G = (float*)p; p += x.table_bytes();
    x.kn.valid = (unsigned char*)p;
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengDetrendRun(const void* in_dev, int nwin_call, void* out_dev, int* completed) {
    if (!in_dev || !out_dev || !completed) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: null input, output or result");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_dtmu);
    DetrendContext& x = g_dt;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Detrend: not initialized (call xengDetrendInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Detrend: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    XENG_HIP(hipSetDevice(x.gpu));
    const long long n0 = x.nwindows;
    const int e0 = (int)(n0 % x.nblk);
    const long long kcur = n0 / x.nblk;
    const bool done = e0 + nwin_call >= x.nblk;             // (nwin_call <= nblk: at most one block ends in a call)
    const dim3 tiles((unsigned)((x.nser + DT_TILE - 1) / DT_TILE), (unsigned)((nwin_call + DT_TILE - 1) / DT_TILE));
    if (x.nprod == 1)
        hipLaunchKernelGGL(detrend_ingest_kernel<1>, tiles, dim3(DT_THREADS), DT_TILE_LDS_BYTES, x.stream, (const float*)in_dev, x.ring, x.nser, x.L, (int)(n0 % x.L),
                           nwin_call);
    else
        hipLaunchKernelGGL(detrend_ingest_kernel<4>, tiles, dim3(DT_THREADS), DT_TILE_LDS_BYTES, x.stream, (const float*)in_dev, x.ring, x.nser, x.L, (int)(n0 % x.L),
                           nwin_call);
    if (done)
        hipLaunchKernelGGL(detrend_decide_kernel, dim3((unsigned)x.nser), dim3(DT_THREADS), detrend_decide_lds_bytes(x.nblk), x.stream, (const float*)x.ring, x.kn, x.nser,
                           x.nblk, x.L, (int)((kcur * x.nblk) % x.L), (int)(kcur & (DT_KNOTS - 1)), x.normalise, x.k_mad);
    const long long m0 = n0 - x.D;
    const int slotm0 = (int)(((m0 % x.L) + x.L) % x.L);
    hipLaunchKernelGGL(detrend_apply_kernel, tiles, dim3(DT_THREADS), DT_TILE_LDS_BYTES, x.stream, (const float*)x.ring, x.kn, (float*)out_dev, x.nser, x.nblk, x.L,
                       nwin_call, kcur - 2, e0, slotm0, x.normalise, x.r);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows += nwin_call;
    if (done) x.nblocks++;
    *completed = done ? 1 : 0;
    return XENG_STATUS_SUCCESS;
}

int xengDetrendReset(void) {
    std::lock_guard<std::mutex> lk(g_dtmu);
    DetrendContext& x = g_dt;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Detrend: not initialized");
    x.nwindows = 0;                     // (nothing is launched or cleared: the kernels decide by index what lies before window 0)
    x.nblocks = 0;
    return XENG_STATUS_SUCCESS;
}

int xengDetrendGetInfo(long long* nwindows_since_reset, long long* nblocks_decided) {
    if (!nwindows_since_reset || !nblocks_decided) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DetrendGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_dtmu);
    DetrendContext& x = g_dt;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Detrend: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nblocks_decided = x.nblocks;
    return XENG_STATUS_SUCCESS;
}

int xengDetrendGetKnots(float* M, float* A, unsigned char* valid) {
    if (!M || !A || !valid) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DetrendGetKnots: null result");
    std::lock_guard<std::mutex> lk(g_dtmu);
    DetrendContext& x = g_dt;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Detrend: not initialized");
    if (x.nblocks == 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "DetrendGetKnots: no block is decided since the reset");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    const size_t at = (size_t)((x.nblocks - 1) & (DT_KNOTS - 1)) * x.nser;
    XENG_HIP(hipMemcpy(M, x.kn.M + at, (size_t)x.nser * 4, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(A, x.kn.A + at, (size_t)x.nser * 4, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(valid, x.kn.valid + at, (size_t)x.nser, hipMemcpyDeviceToHost));
    return XENG_STATUS_SUCCESS;
}

int xengDetrendCheckGuards(int* intact) { return beam_context_check_guards(g_dtmu, g_dt, g_dt.alloc, "Detrend", intact); }
int xengDetrendMark(unsigned long long* ticket) { return beam_context_mark(g_dtmu, g_dt, "Detrend", ticket); }
int xengDetrendWait(unsigned long long ticket) { return beam_context_wait(g_dtmu, g_dt, "Detrend", ticket); }
int xengDetrendTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_dtmu, g_dt, "Detrend", ticket, done); }
int xengDetrendSync(void) { return beam_context_sync(g_dtmu, g_dt, "Detrend"); }

int xengDetrendDestroy(void) {
    std::lock_guard<std::mutex> lk(g_dtmu);
    return detrend_destroy_locked();
}

}  // extern "C"
