// Host side of the calibration stage (UpchanCalApply; calapply_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "calapply_kernels.h"
#include "xeng_common.h"

namespace xeng {

static_assert(XENG_CALAPPLY_MAX_NSRC == CA_K && XENG_CALAPPLY_MAX_NSTAND == CA_MAX_NSTAND, "the limits of include/xeng.h are the kernel's");

struct CalapplyContext : BeamStreamContext {
    int nstand = 0, nfine = 0, nsrc = 0;
    GuardedState alloc;                 // the state between its guard bands (xengCalapplyCheckGuards)
    double* freq = nullptr;             // f64[nfine], inside alloc
    double* tau = nullptr;              // f64[nsrc][nstand], behind it
    float2* a = nullptr;                // cf32[nfine][nsrc][nstand]: the steering factors (calapply_steer_kernel)
    float2* h = nullptr;                // cf32[nfine][2][nstand]: the apply factors
    float* flux = nullptr;              // f32[nfine][nsrc]
    bool model = false;

    size_t state_bytes() const {
        const size_t n = ((size_t)nfine + (size_t)nsrc * nstand) * sizeof(double) + ((size_t)nfine * nsrc * nstand + (size_t)nfine * 2 * nstand) * sizeof(float2) +
                         (size_t)nfine * nsrc * sizeof(float);
        return (n + 15) & ~(size_t)15;
    }
    int ntile() const { return (nstand + CA_T - 1) / CA_T; }
};
static std::mutex g_camu;
static CalapplyContext g_ca;

static int calapply_destroy_locked() {
    if (!g_ca.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_ca);
    g_ca.alloc.free();
    g_ca = CalapplyContext();
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengCalapplyInitialize(int gpu, int nstand, int nfine, int nsrc) {
    if (nstand <= 0 || nfine <= 0 || nsrc < 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Calapply: bad sizes nstand=%d nfine=%d nsrc=%d", nstand, nfine, nsrc);
    if (nsrc > XENG_CALAPPLY_MAX_NSRC)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Calapply: %d sources, %d at the most", nsrc, XENG_CALAPPLY_MAX_NSRC);
    if (nstand > XENG_CALAPPLY_MAX_NSTAND)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Calapply: %d stands, %d at the most", nstand, XENG_CALAPPLY_MAX_NSTAND);
    if (nfine > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Calapply: %d fine channels is more than one launch takes", nfine);
    std::lock_guard<std::mutex> lk(g_camu);
    calapply_destroy_locked();
    CalapplyContext& x = g_ca;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nstand = nstand; x.nfine = nfine; x.nsrc = nsrc;
    const std::vector<float2> ones((size_t)nfine * 2 * nstand, make_float2(1.f, 0.f));
    float2* h = nullptr;
    if (x.alloc.open(x.state_bytes()) == hipSuccess) {
        x.freq = (double*)x.alloc.data();
        x.tau = x.freq + nfine;
        x.a = (float2*)(x.tau + (size_t)nsrc * nstand);
        x.h = x.a + (size_t)nfine * nsrc * nstand;
        x.flux = (float*)(x.h + (size_t)nfine * 2 * nstand);
        if (hipMemcpy(x.h, ones.data(), ones.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess) h = x.h;
    }
    if (!h) {
        (void)hipGetLastError();
        x.alloc.free();
        x = CalapplyContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Calapply: cannot allocate %.3g MB of state", (double)nfine * nstand * (nsrc + 2) * 8e-6);
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengCalapplyGetInfo(int* ntile, int* ngroup, int* lds_bytes, long long* span_bytes) {
    if (!ntile || !ngroup || !lds_bytes || !span_bytes) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplyGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_camu);
    CalapplyContext& x = g_ca;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Calapply: not initialized");
    *ntile = x.ntile();
    *ngroup = x.ntile() * (x.ntile() + 1) / 2 * x.nfine;
    *lds_bytes = (int)calapply_lds_bytes();
    *span_bytes = (long long)x.nfine * (2LL * x.nstand) * (2LL * x.nstand) * (long long)sizeof(float2);
    return XENG_STATUS_SUCCESS;
}

int xengCalapplySetModel(const double* tau, const double* freq, const float* flux) {
    if (!freq) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplySetModel: null frequencies");
    std::lock_guard<std::mutex> lk(g_camu);
    CalapplyContext& x = g_ca;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Calapply: not initialized (call xengCalapplyInitialize)");
    if (x.nsrc > 0 && (!tau || !flux)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplySetModel: null %s", !tau ? "delays" : "fluxes");
    for (int c = 0; c < x.nfine; c++)
        if (!std::isfinite(freq[c])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplySetModel: frequency %d is not finite", c);
    for (size_t i = 0; i < (size_t)x.nsrc * x.nstand; i++)
        if (!std::isfinite(tau[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplySetModel: delay %zu is not finite", i);
    for (size_t i = 0; i < (size_t)x.nfine * x.nsrc; i++)
        if (!std::isfinite(flux[i]) || flux[i] < 0.f)
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplySetModel: flux %zu is %g: not a finite number >= 0", i, (double)flux[i]);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(x.freq, freq, (size_t)x.nfine * sizeof(double), hipMemcpyHostToDevice));
    if (x.nsrc > 0) {
        XENG_HIP(hipMemcpy(x.tau, tau, (size_t)x.nsrc * x.nstand * sizeof(double), hipMemcpyHostToDevice));
        XENG_HIP(hipMemcpy(x.flux, flux, (size_t)x.nfine * x.nsrc * sizeof(float), hipMemcpyHostToDevice));
        const unsigned nb = (unsigned)(((size_t)x.nsrc * x.nstand + CA_STEER_THREADS - 1) / CA_STEER_THREADS);
        hipLaunchKernelGGL(calapply_steer_kernel, dim3(nb, (unsigned)x.nfine), dim3(CA_STEER_THREADS), 0, x.stream, x.freq, x.tau, x.a, x.nstand, x.nsrc);
        stream_tick(STREAM_BEAM);
        XENG_HIP(hipGetLastError());
        XENG_HIP(hipStreamSynchronize(x.stream));
    }
    x.model = true;
    return XENG_STATUS_SUCCESS;
}

int xengCalapplySetFactors(const void* h) {
    if (!h) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplySetFactors: null factors");
    std::lock_guard<std::mutex> lk(g_camu);
    CalapplyContext& x = g_ca;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Calapply: not initialized (call xengCalapplyInitialize)");
    const float* w = (const float*)h;
    for (size_t i = 0; i < (size_t)x.nfine * 2 * x.nstand * 2; i++)
        if (!std::isfinite(w[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CalapplySetFactors: word %zu is not finite", i);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the factors: they apply to the next Run only)
    XENG_HIP(hipMemcpy(x.h, h, (size_t)x.nfine * 2 * x.nstand * sizeof(float2), hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengCalapplyRun(const void* vis_dev, void* out_dev) {
    if (!vis_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Calapply: null %s", !vis_dev ? "input" : "output");
    if ((uintptr_t)vis_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Calapply: input %p or output %p not 16-byte aligned", vis_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_camu);
    CalapplyContext& x = g_ca;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Calapply: not initialized (call xengCalapplyInitialize)");
    if (x.nsrc > 0 && !x.model) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Calapply: no sky model (call xengCalapplySetModel)");
    XENG_HIP(hipSetDevice(x.gpu));
    const int nt = x.ntile();
    hipLaunchKernelGGL(calapply_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)x.nfine), dim3(CA_THREADS), 0, x.stream, (const float2*)vis_dev, x.a, x.flux,
                       x.h, (float2*)out_dev, x.nstand, x.nsrc);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

int xengCalapplyCheckGuards(int* intact) { return beam_context_check_guards(g_camu, g_ca, g_ca.alloc, "Calapply", intact); }
int xengCalapplyMark(unsigned long long* ticket) { return beam_context_mark(g_camu, g_ca, "Calapply", ticket); }
int xengCalapplyWait(unsigned long long ticket) { return beam_context_wait(g_camu, g_ca, "Calapply", ticket); }
int xengCalapplyTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_camu, g_ca, "Calapply", ticket, done); }
int xengCalapplySync(void) { return beam_context_sync(g_camu, g_ca, "Calapply"); }

int xengCalapplyDestroy(void) {
    std::lock_guard<std::mutex> lk(g_camu);
    return calapply_destroy_locked();
}

}  // extern "C"
