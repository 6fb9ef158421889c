// Host side of the boxcar single-pulse search (BeamPulseSearch; pulse_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "pulse_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct PulseContext : BeamStreamContext {
    int npair = 0, ndm = 0, nwin = 0, nprod = 0, nwidth = 0, nstat = 0;
    int nser = 0;                       // npair * ndm
    int T = 0, L = 0;                   // windows a boxcar reaches back before a call: 2^(nwidth-1) - 1; slots of the y ring: T + nwin
    GuardedState alloc;                 // the state and the y ring between their guard bands (xengPulseCheckGuards)
    float* state = nullptr;             // f32[PS_NSTATE][nser], inside alloc
    float* tail = nullptr;              // f32[L][nser], behind the state
    float* rho = nullptr;               // f32[nwidth]
    float r_nstat = 0.f;
    long long nwindows = 0;             // windows taken since the last reset

    size_t state_bytes() const { return (size_t)(PS_NSTATE + L) * nser * sizeof(float); }
};
constexpr int PS_LDS_ROWS = 256;        // rows of 64 floats in the 64 KiB a work-group may take
static std::mutex g_psmu;
static PulseContext g_ps;

static int pulse_destroy_locked() {
    if (!g_ps.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_ps);
    g_ps.alloc.free();
    if (g_ps.rho) (void)hipFree(g_ps.rho);
    g_ps = PulseContext();
    return XENG_STATUS_SUCCESS;
}

template <int NPROD>
static void pulse_launch(const PulseContext& x, const float* in, int nc, float4* out) {
    const int rows = x.T + 2 * nc < 16 ? 16 : x.T + 2 * nc;             // (the last reduction takes 12 rows)
    const int n0 = x.nwindows < (1LL << 30) ? (int)x.nwindows : (1 << 30);
    hipLaunchKernelGGL((pulse_search_kernel<NPROD>), dim3((unsigned)((x.nser + PS_SERIES - 1) / PS_SERIES)), dim3(64 * PS_WAVES),
                       (size_t)rows * PS_SERIES * sizeof(float), x.stream, in, x.state, x.tail, x.rho, out, x.nser, nc, x.nwidth, x.nstat, x.r_nstat,
                       x.L, (int)(x.nwindows % x.L), n0, (int)(x.nwindows % x.nstat));
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengPulseInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nwidth, int nstat) {
    if (npair <= 0 || ndm <= 0 || nwin <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: bad sizes npair=%d ndm=%d nwin=%d", npair, ndm, nwin);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: nprod %d not 1 (I) or 4 (XX, YY, Re XY*, Im XY*)", nprod);
    if (nwidth < 1 || nwidth > 8) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: %d boxcar widths, not 1 to 8", nwidth);
    if (nstat < 2 || nstat > (1 << 20)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: a baseline block of %d windows, not 2 to 2^20", nstat);
    if ((1 << (nwidth - 1)) > nstat)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: the widest boxcar, %d windows, is longer than a baseline block of %d", 1 << (nwidth - 1), nstat);
    const int T = (1 << (nwidth - 1)) - 1;
    if ((long long)npair * ndm > (1LL << 24) || (long long)T + 2LL * nwin > PS_LDS_ROWS)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: %d pairs x %d trials, or %d windows a call behind boxcars of up to %d, is more than one launch takes",
                  npair, ndm, nwin, T + 1);
    std::lock_guard<std::mutex> lk(g_psmu);
    pulse_destroy_locked();
    PulseContext& x = g_ps;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.npair = npair; x.ndm = ndm; x.nwin = nwin; x.nprod = nprod; x.nwidth = nwidth; x.nstat = nstat;
    x.nser = npair * ndm;
    x.T = T;
    x.L = T + nwin;
    x.r_nstat = 1.0f / (float)nstat;
    float rho[8];
    for (int iw = 0; iw < nwidth; iw++) rho[iw] = (float)std::ldexp(iw & 1 ? 0.70710678118654752440 : 1.0, -(iw >> 1));    // 2^(-iw/2)
    if (x.alloc.open(x.state_bytes()) != hipSuccess || hipMalloc(&x.rho, sizeof(rho)) != hipSuccess ||
        hipMemcpy(x.rho, rho, sizeof(rho), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        if (x.rho) (void)hipFree(x.rho);
        x = PulseContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Pulse: cannot allocate %.3g MB of state", (double)(PS_NSTATE + T + nwin) * npair * ndm * 4e-6);
    }
    x.state = (float*)x.alloc.data();
    x.tail = x.state + (size_t)PS_NSTATE * x.nser;
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengPulseRun(const void* in_dev, int nwin_call, void* out_dev) {
    if (!in_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: null %s", in_dev ? "output" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_psmu);
    PulseContext& x = g_ps;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Pulse: not initialized (call xengPulseInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Pulse: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    XENG_HIP(hipSetDevice(x.gpu));
    if (x.nprod == 1)
        pulse_launch<1>(x, (const float*)in_dev, nwin_call, (float4*)out_dev);
    else
        pulse_launch<4>(x, (const float*)in_dev, nwin_call, (float4*)out_dev);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows += nwin_call;
    return XENG_STATUS_SUCCESS;
}

int xengPulseReset(void) {
    std::lock_guard<std::mutex> lk(g_psmu);
    PulseContext& x = g_ps;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Pulse: not initialized");
    x.nwindows = 0;                     // (what the state and the ring hold lies before window 0 now: the kernel leaves it out)
    return XENG_STATUS_SUCCESS;
}

int xengPulseGetInfo(long long* nwindows_since_reset, long long* nblocks_complete) {
    if (!nwindows_since_reset || !nblocks_complete) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PulseGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_psmu);
    PulseContext& x = g_ps;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Pulse: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nblocks_complete = x.nwindows / x.nstat;
    return XENG_STATUS_SUCCESS;
}

int xengPulseGetBaseline(float* c, float* m, float* var) {
    if (!c || !m || !var) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PulseGetBaseline: null result");
    std::lock_guard<std::mutex> lk(g_psmu);
    PulseContext& x = g_ps;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Pulse: not initialized");
    if (x.nwindows < x.nstat) XENG_FAIL(XENG_STATUS_INVALID_STATE, "PulseGetBaseline: %lld windows since the reset, no block of %d is complete", x.nwindows, x.nstat);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    const size_t n = (size_t)x.nser * sizeof(float);
    XENG_HIP(hipMemcpy(c, x.state + (size_t)PS_DC * x.nser, n, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(m, x.state + (size_t)PS_DM * x.nser, n, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(var, x.state + (size_t)PS_DV * x.nser, n, hipMemcpyDeviceToHost));
    return XENG_STATUS_SUCCESS;
}

int xengPulseCheckGuards(int* intact) { return beam_context_check_guards(g_psmu, g_ps, g_ps.alloc, "Pulse", intact); }
int xengPulseMark(unsigned long long* ticket) { return beam_context_mark(g_psmu, g_ps, "Pulse", ticket); }
int xengPulseWait(unsigned long long ticket) { return beam_context_wait(g_psmu, g_ps, "Pulse", ticket); }
int xengPulseTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_psmu, g_ps, "Pulse", ticket, done); }
int xengPulseSync(void) { return beam_context_sync(g_psmu, g_ps, "Pulse"); }

int xengPulseDestroy(void) {
    std::lock_guard<std::mutex> lk(g_psmu);
    return pulse_destroy_locked();
}

}  // extern "C"
