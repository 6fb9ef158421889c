// Host side of the incoherent dedisperser (BeamDedisperse; dedisp_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "dedisp_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct DedispContext : BeamStreamContext {
    int npair = 0, nfine = 0, nwin = 0, ndm = 0, max_delay = 0, nprod = 0;
    int L = 0;                          // windows of the history ring: max_delay + nwin
    GuardedState hist_alloc;            // the history between its guard bands (xengDedispCheckGuards)
    float* hist = nullptr;              // f32[npair][nfine][nprod][L], inside hist_alloc
    int* bt = nullptr;                  // i32[nfine][ndm]: back-delays S - s[d][q]
    float* w = nullptr;                 // f32[nfine]
    int S = -1;                         // the table's largest delay; -1: no table yet
    long long nwindows = 0;             // windows taken since the last reset
    int head = 0;                       // slot of the next window

    size_t hist_bytes() const { return (size_t)npair * nfine * nprod * (size_t)L * sizeof(float); }
};
static std::mutex g_ddmu;
static DedispContext g_dd;

static int dedisp_destroy_locked() {
    if (!g_dd.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_dd);
    g_dd.hist_alloc.free();
    if (g_dd.bt) (void)hipFree(g_dd.bt);
    if (g_dd.w) (void)hipFree(g_dd.w);
    g_dd = DedispContext();
    return XENG_STATUS_SUCCESS;
}

template <int NPROD>
static void dedisp_launch(const DedispContext& x, const float4* in, int nc, float* out) {
    const dim3 gi((unsigned)((x.nfine + DD_TILE - 1) / DD_TILE), (unsigned)x.npair, (unsigned)((nc + DD_TILE - 1) / DD_TILE));
    hipLaunchKernelGGL((dedisp_ingest_kernel<NPROD>), gi, dim3(256), 0, x.stream, in, x.hist, x.npair, x.nfine, x.L, x.head, nc);
    int tshift = 0;
    while (tshift < 6 && (1 << tshift) < nc) tshift++;
    const int TT = 1 << tshift, DD = 64 >> tshift;
    const long long tiles = (long long)((nc + TT - 1) / TT) * ((x.ndm + DD - 1) / DD);
    const int n0 = x.nwindows < (1LL << 30) ? (int)x.nwindows : (1 << 30);
    hipLaunchKernelGGL((dedisp_kernel<NPROD>), dim3((unsigned)tiles, (unsigned)x.npair), dim3(64 * DD_NSEG), 0, x.stream, x.hist, x.bt, x.w, out,
                       x.npair, x.nfine, x.ndm, x.L, x.head, n0, nc, tshift);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengDedispInitialize(int gpu, int npair, int nfine, int nwin, int ndm, int max_delay, int nprod) {
    if (npair <= 0 || nfine <= 0 || nwin <= 0 || ndm <= 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: bad sizes npair=%d nfine=%d nwin=%d ndm=%d", npair, nfine, nwin, ndm);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: nprod %d not 1 (I) or 4 (XX, YY, Re XY*, Im XY*)", nprod);
    if (max_delay < 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: max_delay %d is negative", max_delay);
    const long long L = (long long)max_delay + nwin;
    const double bytes = (double)npair * nfine * nprod * (double)L * sizeof(float);
    if (bytes > (double)XENG_DEDISP_MAX_HISTORY_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: a history of %lld windows x %d pairs x %d channels x %d is %.3g GB, above the limit of %.3g GB",
                  L, npair, nfine, nprod, bytes * 1e-9, (double)XENG_DEDISP_MAX_HISTORY_BYTES * 1e-9);
    if (npair > 65535 || (long long)ndm * nfine > (1LL << 28) || (long long)ndm * nwin > (1LL << 30))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: %d pairs, %d trials x %d channels x %d windows is more than one launch takes", npair, ndm,
                  nfine, nwin);
    std::lock_guard<std::mutex> lk(g_ddmu);
    dedisp_destroy_locked();
    DedispContext& x = g_dd;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.npair = npair; x.nfine = nfine; x.nwin = nwin; x.ndm = ndm; x.max_delay = max_delay; x.nprod = nprod;
    x.L = (int)L;
    const std::vector<float> ones((size_t)nfine, 1.f);
    if (x.hist_alloc.open(x.hist_bytes()) != hipSuccess || hipMalloc(&x.bt, (size_t)ndm * nfine * sizeof(int)) != hipSuccess ||
        hipMalloc(&x.w, (size_t)nfine * sizeof(float)) != hipSuccess ||
        hipMemcpy(x.w, ones.data(), (size_t)nfine * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.hist_alloc.free();
        if (x.bt) (void)hipFree(x.bt);
        if (x.w) (void)hipFree(x.w);
        x = DedispContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Dedisp: cannot allocate %.3g MB of history and %.3g MB of delays", bytes * 1e-6, (double)ndm * nfine * 4e-6);
    }
    x.hist = (float*)x.hist_alloc.data();
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengDedispSetDelays(const int* delays) {
    if (!delays) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DedispSetDelays: null table");
    if ((uintptr_t)delays % sizeof(int)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DedispSetDelays: table %p not aligned to int", (const void*)delays);
    std::lock_guard<std::mutex> lk(g_ddmu);
    DedispContext& x = g_dd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Dedisp: not initialized (call xengDedispInitialize)");
    int S = 0;
    for (int d = 0; d < x.ndm; d++)
        for (int q = 0; q < x.nfine; q++) {
            const int s = delays[(size_t)d * x.nfine + q];
            if (s < 0 || s > x.max_delay)
                XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DedispSetDelays: delay %d of trial %d, channel %d outside 0..max_delay = %d", s, d, q, x.max_delay);
            if (s > S) S = s;
        }
    std::vector<int> bt((size_t)x.nfine * x.ndm);
    for (int d = 0; d < x.ndm; d++)
        for (int q = 0; q < x.nfine; q++) bt[(size_t)q * x.ndm + d] = S - delays[(size_t)d * x.nfine + q];
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the table and the history)
    XENG_HIP(hipMemcpy(x.bt, bt.data(), bt.size() * sizeof(int), hipMemcpyHostToDevice));
    XENG_HIP(hipMemsetAsync(x.hist, 0, x.hist_bytes(), x.stream));
    XENG_HIP(hipStreamSynchronize(x.stream));
    x.S = S;
    x.nwindows = 0;
    x.head = 0;
    return XENG_STATUS_SUCCESS;
}

int xengDedispSetWeights(const float* weights) {
    if ((uintptr_t)weights % sizeof(float)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DedispSetWeights: weights %p not aligned to float", (const void*)weights);
    std::lock_guard<std::mutex> lk(g_ddmu);
    DedispContext& x = g_dd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Dedisp: not initialized (call xengDedispInitialize)");
    std::vector<float> w((size_t)x.nfine, 1.f);
    if (weights)
        for (int q = 0; q < x.nfine; q++) {
            if (!std::isfinite(weights[q])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DedispSetWeights: weight %d is not finite", q);
            w[q] = weights[q];
        }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the weights)
    XENG_HIP(hipMemcpy(x.w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengDedispRun(const void* in_dev, int nwin_call, void* out_dev) {
    if (!in_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: null %s", in_dev ? "output" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_ddmu);
    DedispContext& x = g_dd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Dedisp: not initialized (call xengDedispInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Dedisp: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    if (x.S < 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Dedisp: no delay table (call xengDedispSetDelays)");
    XENG_HIP(hipSetDevice(x.gpu));
    if (x.nprod == 1)
        dedisp_launch<1>(x, (const float4*)in_dev, nwin_call, (float*)out_dev);
    else
        dedisp_launch<4>(x, (const float4*)in_dev, nwin_call, (float*)out_dev);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.head = (x.head + nwin_call) % x.L;
    x.nwindows += nwin_call;
    return XENG_STATUS_SUCCESS;
}

int xengDedispReset(void) {
    std::lock_guard<std::mutex> lk(g_ddmu);
    DedispContext& x = g_dd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Dedisp: not initialized");
    x.nwindows = 0;                     // (what the ring holds lies before window 0 now: the kernel leaves it out)
    return XENG_STATUS_SUCCESS;
}

int xengDedispGetInfo(int* max_delay_in_use, long long* nwindows_since_reset) {
    if (!max_delay_in_use || !nwindows_since_reset) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "DedispGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_ddmu);
    DedispContext& x = g_dd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Dedisp: not initialized");
    *max_delay_in_use = x.S;
    *nwindows_since_reset = x.nwindows;
    return XENG_STATUS_SUCCESS;
}

int xengDedispCheckGuards(int* intact) { return beam_context_check_guards(g_ddmu, g_dd, g_dd.hist_alloc, "Dedisp", intact); }
int xengDedispMark(unsigned long long* ticket) { return beam_context_mark(g_ddmu, g_dd, "Dedisp", ticket); }
int xengDedispWait(unsigned long long ticket) { return beam_context_wait(g_ddmu, g_dd, "Dedisp", ticket); }
int xengDedispTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_ddmu, g_dd, "Dedisp", ticket, done); }
int xengDedispSync(void) { return beam_context_sync(g_ddmu, g_dd, "Dedisp"); }

int xengDedispDestroy(void) {
    std::lock_guard<std::mutex> lk(g_ddmu);
    return dedisp_destroy_locked();
}

}  // extern "C"
