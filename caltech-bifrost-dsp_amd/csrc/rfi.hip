// Host side of the cleaning of the power beams (BeamRfiClean; rfi_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "rfi_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct RfiContext : BeamStreamContext {
    int npair = 0, nfine = 0, nwin = 0, nstat = 0;
    size_t NC = 0;                      // npair * nfine
    int L = 0;                          // nstat + nwin, slots of the ring
    float r = 0.f;                      // 1.0f / (float)nstat
    GuardedState alloc;                 // the state between its guard bands (xengRfiCheckGuards)
    float4* ring = nullptr;             // [L][NC]
    float4* run = nullptr;              // [3][NC]
    RfiTables2 tab = {};                   // block k in half k & 1
    unsigned char* mask = nullptr;      // u8[nfine]
    RfiControl2 ctl = {};                  // the controls each half's block was decided with
    RfiControl cur = {0.f, 0.f, 0, 0};  // the controls in force for the next block to be decided
    float k_chan = 0.f;
    bool have_ctl = false;
    long long nwindows = 0;             // windows taken since the last reset
    long long nblocks = 0;              // blocks decided since the last reset

    static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
    size_t half_bytes() const { return NC * (3 * 16 + 8 + 3 * 4) + up16((size_t)npair * 4) + up16(NC); }
    size_t state_bytes() const { return ((size_t)L + 3) * NC * 16 + 2 * half_bytes() + up16((size_t)nfine); }
};
static std::mutex g_rfmu;
static RfiContext g_rf;

static int rfi_destroy_locked() {
    if (!g_rf.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_rf);
    g_rf.alloc.free();
    g_rf = RfiContext();
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengRfiInitialize(int gpu, int npair, int nfine, int nwin, int nstat) {
    if (npair < 1 || npair > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: %d pairs, not 1 to 65535", npair);
    if (nfine < 4 || nfine > RF_MAX_NFINE) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: %d fine channels, not 4 to %d", nfine, RF_MAX_NFINE);
    if (nstat < 2 || nstat > (1 << 20)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: blocks of %d windows, not 2 to 2^20", nstat);
    if (nwin < 1 || nwin > nstat) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: %d windows a call, not 1 to nstat = %d", nwin, nstat);
    RfiContext y;
    y.npair = npair; y.nfine = nfine; y.nwin = nwin; y.nstat = nstat;
    y.NC = (size_t)npair * nfine;
    y.L = nstat + nwin;
    y.r = 1.0f / (float)nstat;
    const unsigned long long hist = (unsigned long long)y.L * y.NC * 16;
    if (hist >= (unsigned long long)XENG_RFI_MAX_HISTORY_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: a history of %d + %d windows of %d x %d channels needs %.3g GB, the limit is %.3g GB", nstat, nwin, npair, nfine,
                  (double)hist * 1e-9, (double)XENG_RFI_MAX_HISTORY_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_rfmu);
    rfi_destroy_locked();
    RfiContext& x = g_rf;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    y.gpu = x.gpu;
    y.stream = x.stream;
    x = y;
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = RfiContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Rfi: cannot allocate %.3g MB of state", (double)y.state_bytes() * 1e-6);
    }
    char* p = (char*)x.alloc.data();
    x.ring = (float4*)p;
    p += (size_t)x.L * x.NC * 16;
    x.run = (float4*)p;
    p += 3 * x.NC * 16;
    for (int h = 0; h < 2; h++) {       // (every piece starts at a multiple of 16 bytes)
        RfiTables& t = x.tab.h[h];
        t.c = (float4*)p; p += x.NC * 16;
        t.m = (float4*)p; p += x.NC * 16;
        t.g = (float4*)p; p += x.NC * 16;
        t.v = (float2*)p; p += x.NC * 8;
        t.mu = (float*)p; p += x.NC * 4;
        t.var = (float*)p; p += x.NC * 4;
        t.r = (float*)p; p += x.NC * 4;
        t.notkept = (int*)p; p += RfiContext::up16((size_t)npair * 4);
        t.flag = (unsigned char*)p; p += RfiContext::up16(x.NC);
    }
    x.mask = (unsigned char*)p;         // (zeros, as the whole state is after open: no channel is left out)
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengRfiSetControl(float k_chan, float t_clip, float t_broad, int min_count, int zerodm) {
    if (!std::isfinite(k_chan) || !(k_chan > 0.f) || !std::isfinite(t_clip) || !(t_clip > 0.f) || !std::isfinite(t_broad) || !(t_broad > 0.f))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RfiSetControl: k_chan %g, t_clip %g, t_broad %g are not finite and positive", k_chan, t_clip, t_broad);
    if (zerodm != 0 && zerodm != 1) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RfiSetControl: zerodm %d, not 0 or 1", zerodm);
    std::lock_guard<std::mutex> lk(g_rfmu);
    RfiContext& x = g_rf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rfi: not initialized (call xengRfiInitialize)");
    if (min_count < 0 || min_count > x.nfine) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RfiSetControl: min_count %d, not 0 to nfine = %d", min_count, x.nfine);
    x.k_chan = k_chan;
    x.cur = RfiControl{t_clip, t_broad, min_count, zerodm};
    x.have_ctl = true;
    return XENG_STATUS_SUCCESS;
}

int xengRfiSetMask(const unsigned char* mask) {
    std::lock_guard<std::mutex> lk(g_rfmu);
    RfiContext& x = g_rf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rfi: not initialized (call xengRfiInitialize)");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (no decision in flight reads the mask)
    if (mask)
        XENG_HIP(hipMemcpy(x.mask, mask, (size_t)x.nfine, hipMemcpyHostToDevice));
    else
        XENG_HIP(hip_memset_now(x.mask, 0, (size_t)x.nfine));
    return XENG_STATUS_SUCCESS;
}

int xengRfiRun(const void* in_dev, int nwin_call, void* out_dev, void* stats_dev, int* completed) {
    if (!in_dev || !out_dev || !stats_dev || !completed) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: null input, output, stats or result");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16 || (uintptr_t)stats_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: input %p, output %p or stats %p not 16-byte aligned", in_dev, out_dev, stats_dev);
    std::lock_guard<std::mutex> lk(g_rfmu);
    RfiContext& x = g_rf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rfi: not initialized (call xengRfiInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rfi: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    if (!x.have_ctl) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rfi: no controls (call xengRfiSetControl)");
    XENG_HIP(hipSetDevice(x.gpu));
    const long long n0 = x.nwindows;
    const int pos0 = (int)(n0 % x.nstat);
    const long long k0 = n0 / x.nstat;
    const bool done = pos0 + nwin_call >= x.nstat;          // (nwin_call <= nstat: at most one block ends in a call)
    const unsigned groups = (unsigned)((x.NC + RF_THREADS - 1) / RF_THREADS);
    hipLaunchKernelGGL(rfi_ingest_kernel, dim3(groups), dim3(RF_THREADS), 0, x.stream, (const float4*)in_dev, x.ring, x.run, x.tab, x.NC, nwin_call, x.nstat, x.L,
                       pos0, (int)(n0 % x.L), (int)(k0 & 1), x.r);
    if (done) {
        const int h = (int)(k0 & 1);
        x.ctl.h[h] = x.cur;             // the controls and the mask hold from the next block to be decided: this one
        hipLaunchKernelGGL(rfi_decide_kernel, dim3((unsigned)x.npair), dim3(RF_THREADS), rfi_decide_lds_bytes(x.nfine), x.stream, x.tab.h[h], (const unsigned char*)x.mask, x.nfine, x.k_chan);
    }
    hipLaunchKernelGGL(rfi_apply_kernel, dim3((unsigned)nwin_call, (unsigned)x.npair), dim3(RF_THREADS), RF_APPLY_LDS_BYTES, x.stream, (const float4*)x.ring, x.tab, x.ctl,
                       (float4*)out_dev, (int*)stats_dev, x.nfine, x.npair, x.nstat, x.L, n0 - x.nstat);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows += nwin_call;
    if (done) x.nblocks++;
    *completed = done ? 1 : 0;
    return XENG_STATUS_SUCCESS;
}

int xengRfiReset(void) {
    std::lock_guard<std::mutex> lk(g_rfmu);
    RfiContext& x = g_rf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rfi: not initialized");
    x.nwindows = 0;                     // (nothing is launched or cleared: the kernels decide by index what lies before window 0)
    x.nblocks = 0;
    return XENG_STATUS_SUCCESS;
}

int xengRfiGetInfo(long long* nwindows_since_reset, long long* nblocks_decided) {
    if (!nwindows_since_reset || !nblocks_decided) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RfiGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_rfmu);
    RfiContext& x = g_rf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rfi: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nblocks_decided = x.nblocks;
    return XENG_STATUS_SUCCESS;
}

int xengRfiGetBlock(unsigned char* flags, float* mu, float* var, float* r, float* gains) {
    if (!flags || !mu || !var || !r || !gains) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RfiGetBlock: null result");
    std::lock_guard<std::mutex> lk(g_rfmu);
    RfiContext& x = g_rf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rfi: not initialized");
    if (x.nblocks == 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "RfiGetBlock: no block is decided since the reset");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    const RfiTables& t = x.tab.h[(x.nblocks - 1) & 1];
    XENG_HIP(hipMemcpy(flags, t.flag, x.NC, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(mu, t.mu, x.NC * 4, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(var, t.var, x.NC * 4, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(r, t.r, x.NC * 4, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(gains, t.g, x.NC * 16, hipMemcpyDeviceToHost));
    return XENG_STATUS_SUCCESS;
}

int xengRfiCheckGuards(int* intact) { return beam_context_check_guards(g_rfmu, g_rf, g_rf.alloc, "Rfi", intact); }
int xengRfiMark(unsigned long long* ticket) { return beam_context_mark(g_rfmu, g_rf, "Rfi", ticket); }
int xengRfiWait(unsigned long long ticket) { return beam_context_wait(g_rfmu, g_rf, "Rfi", ticket); }
int xengRfiTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_rfmu, g_rf, "Rfi", ticket, done); }
int xengRfiSync(void) { return beam_context_sync(g_rfmu, g_rf, "Rfi"); }

int xengRfiDestroy(void) {
    std::lock_guard<std::mutex> lk(g_rfmu);
    return rfi_destroy_locked();
}

}  // extern "C"
