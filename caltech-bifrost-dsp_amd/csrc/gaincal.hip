// Host side of the gain solver (UpchanGainCal; gaincal_kernels.h): a process-global context of its own on the beamformer's
// stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "gaincal_kernels.h"
#include "xeng_common.h"

namespace xeng {

static_assert(XENG_GAINCAL_MAX_NSRC == GC_K && XENG_GAINCAL_MAX_NSTAND == GC_MAX_NSTAND, "the limits of include/xeng.h are the kernel's");

struct GaincalContext : BeamStreamContext {
    int nstand = 0, nfine = 0, nsrc = 0;
    GuardedState alloc;                 // the state between its guard bands (xengGaincalCheckGuards)
    double* freq = nullptr;             // f64[nfine], inside alloc
    double* tau = nullptr;              // f64[nsrc][nstand], behind it
    float2* keep_g = nullptr;           // cf32[nfine][2][nstand]: the last unreferenced solution
    float* flux = nullptr;              // f32[nfine][nsrc]
    float* w = nullptr;                 // f32[nstand]
    int* keep_ok = nullptr;             // i32[nfine][2]: that solution was converged and finite
    bool model = false, weights = false;
    int refant = 0, niter = XENG_GAINCAL_DEFAULT_NITER;
    double tol = XENG_GAINCAL_DEFAULT_TOL;

    size_t state_bytes() const {
        const size_t n = ((size_t)nfine + (size_t)nsrc * nstand) * sizeof(double) + (size_t)nfine * 2 * nstand * sizeof(float2) +
                         ((size_t)nfine * nsrc + nstand) * sizeof(float) + (size_t)nfine * 2 * sizeof(int);
        return (n + 15) & ~(size_t)15;
    }
};
static std::mutex g_gcmu;
static GaincalContext g_gc;

static int gaincal_destroy_locked() {
    if (!g_gc.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_gc);
    g_gc.alloc.free();
    g_gc = GaincalContext();
    return XENG_STATUS_SUCCESS;
}

// after the stream has drained: no (channel, pol) has a solution to start from
static hipError_t gaincal_forget(GaincalContext& x) { return hip_memset_now(x.keep_ok, 0, (size_t)x.nfine * 2 * sizeof(int)); }

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengGaincalInitialize(int gpu, int nstand, int nfine, int nsrc) {
    if (nstand <= 0 || nfine <= 0 || nsrc <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Gaincal: bad sizes nstand=%d nfine=%d nsrc=%d", nstand, nfine, nsrc);
    if (nsrc > XENG_GAINCAL_MAX_NSRC)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Gaincal: %d sources, the rows of one MFMA tile take %d at the most", nsrc, XENG_GAINCAL_MAX_NSRC);
    if (nstand > XENG_GAINCAL_MAX_NSTAND)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Gaincal: %d stands, the steering tile in LDS takes %d at the most", nstand, XENG_GAINCAL_MAX_NSTAND);
    if (nfine > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Gaincal: %d fine channels is more than one launch takes", nfine);
    std::lock_guard<std::mutex> lk(g_gcmu);
    gaincal_destroy_locked();
    GaincalContext& x = g_gc;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nstand = nstand; x.nfine = nfine; x.nsrc = nsrc;
    const size_t lds = gaincal_lds_bytes(nstand);
    if (lds > (64 << 10) && hipFuncSetAttribute((const void*)gaincal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        x = GaincalContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Gaincal: %d stands need %zu bytes of LDS, which the device refuses", nstand, lds);
    }
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = GaincalContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Gaincal: cannot allocate %.3g MB of state", (double)nfine * nstand * 16e-6);
    }
    x.freq = (double*)x.alloc.data();
    x.tau = x.freq + nfine;
    x.keep_g = (float2*)(x.tau + (size_t)nsrc * nstand);
    x.flux = (float*)(x.keep_g + (size_t)nfine * 2 * nstand);
    x.w = x.flux + (size_t)nfine * nsrc;
    x.keep_ok = (int*)(x.w + nstand);
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengGaincalGetInfo(int* lds_bytes, int* niter, double* tol, int* refant) {
    if (!lds_bytes || !niter || !tol || !refant) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_gcmu);
    GaincalContext& x = g_gc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Gaincal: not initialized");
    *lds_bytes = (int)gaincal_lds_bytes(x.nstand);
    *niter = x.niter;
    *tol = x.tol;
    *refant = x.refant;
    return XENG_STATUS_SUCCESS;
}

int xengGaincalSetModel(const double* tau, const double* freq, const float* flux) {
    if (!tau || !freq || !flux) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetModel: null %s", !tau ? "delays" : !freq ? "frequencies" : "fluxes");
    std::lock_guard<std::mutex> lk(g_gcmu);
    GaincalContext& x = g_gc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Gaincal: not initialized (call xengGaincalInitialize)");
    for (int c = 0; c < x.nfine; c++)
        if (!std::isfinite(freq[c])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetModel: frequency %d is not finite", c);
    for (size_t i = 0; i < (size_t)x.nsrc * x.nstand; i++)
        if (!std::isfinite(tau[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetModel: delay %zu is not finite", i);
    for (size_t i = 0; i < (size_t)x.nfine * x.nsrc; i++)
        if (!std::isfinite(flux[i]) || flux[i] < 0.f)
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetModel: flux %zu is %g: not a finite number >= 0", i, (double)flux[i]);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(x.freq, freq, (size_t)x.nfine * sizeof(double), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.tau, tau, (size_t)x.nsrc * x.nstand * sizeof(double), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.flux, flux, (size_t)x.nfine * x.nsrc * sizeof(float), hipMemcpyHostToDevice));
    XENG_HIP(gaincal_forget(x));
    x.model = true;
    return XENG_STATUS_SUCCESS;
}

int xengGaincalSetWeights(const float* w, int refant) {
    if (!w) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetWeights: null weights");
    std::lock_guard<std::mutex> lk(g_gcmu);
    GaincalContext& x = g_gc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Gaincal: not initialized (call xengGaincalInitialize)");
    for (int s = 0; s < x.nstand; s++)
        if (!std::isfinite(w[s]) || w[s] < 0.f) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetWeights: weight %d is %g: not a finite number >= 0", s, (double)w[s]);
    if (refant < 0 || refant >= x.nstand) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetWeights: reference stand %d of %d", refant, x.nstand);
    if (!(w[refant] > 0.f)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetWeights: the reference stand %d has weight 0", refant);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the weights: they apply to the next Run only)
    XENG_HIP(hipMemcpy(x.w, w, (size_t)x.nstand * sizeof(float), hipMemcpyHostToDevice));
    XENG_HIP(gaincal_forget(x));
    x.refant = refant;
    x.weights = true;
    return XENG_STATUS_SUCCESS;
}

int xengGaincalSetSolver(int niter, double tol) {
    if (niter < 0 || niter > XENG_GAINCAL_MAX_NITER) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetSolver: %d iterations, not in [0, %d]", niter, XENG_GAINCAL_MAX_NITER);
    if (!std::isfinite(tol) || tol < 0.0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "GaincalSetSolver: tolerance %g: not a finite number >= 0", tol);
    std::lock_guard<std::mutex> lk(g_gcmu);
    GaincalContext& x = g_gc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Gaincal: not initialized (call xengGaincalInitialize)");
    x.niter = niter;                            // (kernel arguments: launches in flight keep theirs)
    x.tol = tol;
    return XENG_STATUS_SUCCESS;
}

int xengGaincalRun(const void* vis_dev, void* gains_dev, void* stats_dev, int warm) {
    if (!vis_dev || !gains_dev || !stats_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Gaincal: null %s", !vis_dev ? "input" : !gains_dev ? "gains" : "stats");
    if ((uintptr_t)vis_dev % 16 || (uintptr_t)gains_dev % 8 || (uintptr_t)stats_dev % 4)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Gaincal: input %p not 16-byte, gains %p not 8-byte or stats %p not 4-byte aligned", vis_dev, gains_dev, stats_dev);
    std::lock_guard<std::mutex> lk(g_gcmu);
    GaincalContext& x = g_gc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Gaincal: not initialized (call xengGaincalInitialize)");
    if (!x.model) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Gaincal: no sky model (call xengGaincalSetModel)");
    if (!x.weights) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Gaincal: no weights and reference stand (call xengGaincalSetWeights)");
    XENG_HIP(hipSetDevice(x.gpu));
    hipLaunchKernelGGL(gaincal_kernel, dim3((unsigned)x.nfine, 2), dim3(GC_THREADS), gaincal_lds_bytes(x.nstand), x.stream, (const float2*)vis_dev, x.freq, x.tau,
                       x.flux, x.w, (float2*)gains_dev, (float*)stats_dev, x.keep_g, x.keep_ok, x.nstand, x.nsrc, x.niter, (float)x.tol, x.refant, warm != 0);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

int xengGaincalCheckGuards(int* intact) { return beam_context_check_guards(g_gcmu, g_gc, g_gc.alloc, "Gaincal", intact); }
int xengGaincalMark(unsigned long long* ticket) { return beam_context_mark(g_gcmu, g_gc, "Gaincal", ticket); }
int xengGaincalWait(unsigned long long ticket) { return beam_context_wait(g_gcmu, g_gc, "Gaincal", ticket); }
int xengGaincalTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_gcmu, g_gc, "Gaincal", ticket, done); }
int xengGaincalSync(void) { return beam_context_sync(g_gcmu, g_gc, "Gaincal"); }

int xengGaincalDestroy(void) {
    std::lock_guard<std::mutex> lk(g_gcmu);
    return gaincal_destroy_locked();
}

}  // extern "C"
