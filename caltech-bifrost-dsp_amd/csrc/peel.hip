// Host side of the peeling stage (UpchanPeel; peel_kernels.h): a process-global context of its own on the beamformer's stream
// (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "peel_kernels.h"
#include "xeng_common.h"

namespace xeng {

static_assert(XENG_PEEL_MAX_NDIR == PL_D && XENG_PEEL_MAX_NSTAND == PL_MAX_NSTAND, "the limits of include/xeng.h are the kernels'");

struct PeelContext : BeamStreamContext {
    int nstand = 0, nfine = 0, ndir = 0;
    GuardedState alloc;                 // the state between its guard bands (xengPeelCheckGuards)
    double* freq = nullptr;             // f64[nfine], inside alloc
    double* tau = nullptr;              // f64[ndir][nstand], behind it
    float2* a = nullptr;                // cf32[nfine][ndir][nstand]: the steering factors (peel_steer_kernel)
    float2* keep_g = nullptr;           // cf32[nfine][2][ndir][nstand]: the last unreferenced solution
    float* flux = nullptr;              // f32[nfine][ndir]
    float* w = nullptr;                 // f32[nstand]
    int* keep_ok = nullptr;             // i32[nfine][2]: that solution was converged and finite
    bool model = false, weights = false;
    int refant = 0, niter = XENG_PEEL_DEFAULT_NITER;
    double tol = XENG_PEEL_DEFAULT_TOL;

    size_t state_bytes() const {
        const size_t n = ((size_t)nfine + (size_t)ndir * nstand) * sizeof(double) + (size_t)3 * nfine * ndir * nstand * sizeof(float2) +
                         ((size_t)nfine * ndir + nstand) * sizeof(float) + (size_t)nfine * 2 * sizeof(int);
        return (n + 15) & ~(size_t)15;
    }
    int ntile() const { return (nstand + PS_T - 1) / PS_T; }
};
static std::mutex g_plmu;
static PeelContext g_pl;

static int peel_destroy_locked() {
    if (!g_pl.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_pl);
    g_pl.alloc.free();
    g_pl = PeelContext();
    return XENG_STATUS_SUCCESS;
}

// after the stream has drained: no (channel, pol) has a solution to start from
static hipError_t peel_forget(PeelContext& x) { return hip_memset_now(x.keep_ok, 0, (size_t)x.nfine * 2 * sizeof(int)); }

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengPeelInitialize(int gpu, int nstand, int nfine, int ndir) {
    if (nstand <= 0 || nfine <= 0 || ndir <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Peel: bad sizes nstand=%d nfine=%d ndir=%d", nstand, nfine, ndir);
    if (ndir > XENG_PEEL_MAX_NDIR) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Peel: %d directions, %d at the most", ndir, XENG_PEEL_MAX_NDIR);
    if (nstand > XENG_PEEL_MAX_NSTAND)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Peel: %d stands, the tables in LDS take %d at the most", nstand, XENG_PEEL_MAX_NSTAND);
    if (nfine > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Peel: %d fine channels is more than one launch takes", nfine);
    std::lock_guard<std::mutex> lk(g_plmu);
    peel_destroy_locked();
    PeelContext& x = g_pl;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nstand = nstand; x.nfine = nfine; x.ndir = ndir;
    const size_t lds = peel_lds_bytes(nstand);
    if (lds > (64 << 10) && hipFuncSetAttribute((const void*)peel_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        x = PeelContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Peel: %d stands need %zu bytes of LDS, which the device refuses", nstand, lds);
    }
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = PeelContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Peel: cannot allocate %.3g MB of state", (double)nfine * ndir * nstand * 24e-6);
    }
    x.freq = (double*)x.alloc.data();
    x.tau = x.freq + nfine;
    x.a = (float2*)(x.tau + (size_t)ndir * nstand);
    x.keep_g = x.a + (size_t)nfine * ndir * nstand;
    x.flux = (float*)(x.keep_g + (size_t)nfine * 2 * ndir * nstand);
    x.w = x.flux + (size_t)nfine * ndir;
    x.keep_ok = (int*)(x.w + nstand);
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengPeelGetInfo(int* lds_bytes, int* niter, double* tol, int* refant, long long* span_bytes) {
    if (!lds_bytes || !niter || !tol || !refant || !span_bytes) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_plmu);
    PeelContext& x = g_pl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Peel: not initialized");
    *lds_bytes = (int)peel_lds_bytes(x.nstand);
    *niter = x.niter;
    *tol = x.tol;
    *refant = x.refant;
    *span_bytes = (long long)x.nfine * (2LL * x.nstand) * (2LL * x.nstand) * (long long)sizeof(float2);
    return XENG_STATUS_SUCCESS;
}

int xengPeelSetModel(const double* tau, const double* freq, const float* flux) {
    if (!tau || !freq || !flux) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetModel: null %s", !tau ? "delays" : !freq ? "frequencies" : "fluxes");
    std::lock_guard<std::mutex> lk(g_plmu);
    PeelContext& x = g_pl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Peel: not initialized (call xengPeelInitialize)");
    for (int c = 0; c < x.nfine; c++)
        if (!std::isfinite(freq[c])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetModel: frequency %d is not finite", c);
    for (size_t i = 0; i < (size_t)x.ndir * x.nstand; i++)
        if (!std::isfinite(tau[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetModel: delay %zu is not finite", i);
    for (size_t i = 0; i < (size_t)x.nfine * x.ndir; i++)
        if (!std::isfinite(flux[i]) || flux[i] < 0.f)
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetModel: flux %zu is %g: not a finite number >= 0", i, (double)flux[i]);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(x.freq, freq, (size_t)x.nfine * sizeof(double), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.tau, tau, (size_t)x.ndir * x.nstand * sizeof(double), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.flux, flux, (size_t)x.nfine * x.ndir * sizeof(float), hipMemcpyHostToDevice));
    const unsigned nb = (unsigned)(((size_t)x.ndir * x.nstand + PL_STEER_THREADS - 1) / PL_STEER_THREADS);
    hipLaunchKernelGGL(peel_steer_kernel, dim3(nb, (unsigned)x.nfine), dim3(PL_STEER_THREADS), 0, x.stream, x.freq, x.tau, x.a, x.nstand, x.ndir);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    XENG_HIP(hipStreamSynchronize(x.stream));
    XENG_HIP(peel_forget(x));
    x.model = true;
    return XENG_STATUS_SUCCESS;
}

int xengPeelSetWeights(const float* w, int refant) {
    if (!w) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetWeights: null weights");
    std::lock_guard<std::mutex> lk(g_plmu);
    PeelContext& x = g_pl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Peel: not initialized (call xengPeelInitialize)");
    for (int s = 0; s < x.nstand; s++)
        if (!std::isfinite(w[s]) || w[s] < 0.f) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetWeights: weight %d is %g: not a finite number >= 0", s, (double)w[s]);
    if (refant < 0 || refant >= x.nstand) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetWeights: reference stand %d of %d", refant, x.nstand);
    if (!(w[refant] > 0.f)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetWeights: the reference stand %d has weight 0", refant);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the weights: they apply to the next Run only)
    XENG_HIP(hipMemcpy(x.w, w, (size_t)x.nstand * sizeof(float), hipMemcpyHostToDevice));
    XENG_HIP(peel_forget(x));
    x.refant = refant;
    x.weights = true;
    return XENG_STATUS_SUCCESS;
}

int xengPeelSetSolver(int niter, double tol) {
    if (niter < 0 || niter > XENG_PEEL_MAX_NITER) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetSolver: %d sweeps, not in [0, %d]", niter, XENG_PEEL_MAX_NITER);
    if (!std::isfinite(tol) || tol < 0.0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeelSetSolver: tolerance %g: not a finite number >= 0", tol);
    std::lock_guard<std::mutex> lk(g_plmu);
    PeelContext& x = g_pl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Peel: not initialized (call xengPeelInitialize)");
    x.niter = niter;                            // (kernel arguments: launches in flight keep theirs)
    x.tol = tol;
    return XENG_STATUS_SUCCESS;
}

int xengPeelRun(const void* vis_dev, void* out_dev, void* gains_dev, void* stats_dev, int warm) {
    if (!vis_dev || !out_dev || !gains_dev || !stats_dev)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Peel: null %s", !vis_dev ? "input" : !out_dev ? "output" : !gains_dev ? "gains" : "stats");
    if ((uintptr_t)vis_dev % 16 || (uintptr_t)out_dev % 16 || (uintptr_t)gains_dev % 8 || (uintptr_t)stats_dev % 4)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Peel: input %p or output %p not 16-byte, gains %p not 8-byte or stats %p not 4-byte aligned", vis_dev, out_dev,
                  gains_dev, stats_dev);
    if (vis_dev == out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Peel: the output is the input (the mirrored tiles would be read after they were written)");
    std::lock_guard<std::mutex> lk(g_plmu);
    PeelContext& x = g_pl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Peel: not initialized (call xengPeelInitialize)");
    if (!x.model) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Peel: no sky model (call xengPeelSetModel)");
    if (!x.weights) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Peel: no weights and reference stand (call xengPeelSetWeights)");
    XENG_HIP(hipSetDevice(x.gpu));
    hipLaunchKernelGGL(peel_solve_kernel, dim3((unsigned)x.nfine, 2), dim3(PL_THREADS), peel_lds_bytes(x.nstand), x.stream, (const float2*)vis_dev, x.a, x.flux, x.w,
                       (float2*)gains_dev, (float*)stats_dev, x.keep_g, x.keep_ok, x.nstand, x.ndir, x.niter, (float)x.tol, x.refant, warm != 0);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    const int nt = x.ntile();
    hipLaunchKernelGGL(peel_subtract_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)x.nfine), dim3(PS_THREADS), 0, x.stream, (const float2*)vis_dev, x.a, x.flux,
                       (const float2*)gains_dev, (float2*)out_dev, x.nstand, x.ndir);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

int xengPeelCheckGuards(int* intact) { return beam_context_check_guards(g_plmu, g_pl, g_pl.alloc, "Peel", intact); }
int xengPeelMark(unsigned long long* ticket) { return beam_context_mark(g_plmu, g_pl, "Peel", ticket); }
int xengPeelWait(unsigned long long ticket) { return beam_context_wait(g_plmu, g_pl, "Peel", ticket); }
int xengPeelTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_plmu, g_pl, "Peel", ticket, done); }
int xengPeelSync(void) { return beam_context_sync(g_plmu, g_pl, "Peel"); }

int xengPeelDestroy(void) {
    std::lock_guard<std::mutex> lk(g_plmu);
    return peel_destroy_locked();
}

}  // extern "C"
