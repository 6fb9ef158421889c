// Host side of the deconvolver (UpchanClean; clean_kernels.h): a process-global context of its own on the beamformer's stream
// (BeamStreamContext, xeng_common.h).  A Run enqueues niter + 2 launches of the one kernel and reads nothing back.
#include <cmath>
#include <mutex>
#include <vector>

#include "clean_kernels.h"
#include "xeng_common.h"

namespace xeng {

static size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

struct CleanContext : BeamStreamContext {
    int nstand = 0, nfine = 0, nfavg = 0, npix = 0, niter_max = 0;
    GuardedState alloc;                 // the state between its guard bands (xengCleanCheckGuards)
    double* freq = nullptr;             // f64[nfine], inside alloc
    double* tauT = nullptr;             // f64[nstand][npix], behind it
    float* w = nullptr;                 // f32[nstand]
    uint8_t* mask = nullptr;            // u8[npix]
    int* rec = nullptr;                 // i32[2][ngroup][ntile][CLN_REC]
    int* gstate = nullptr;              // i32[2][ngroup][4]
    bool geometry = false;              // SetGeometry has been called
    int autos = 0;
    double norm = 0.0, dsum = 0.0;      // 1 / (nfavg sum w_s w_t) and sum w_s^2 (0 with autos), float64; the kernel takes them rounded once
    int niter = 0;
    float gain = 0.1f, threshold = 0.f, fraction = 0.f;

    int ngroup() const { return nfine / nfavg; }
    int ntile() const { return (npix + CLN_PX - 1) / CLN_PX; }
    size_t rec_bytes() const { return (size_t)2 * ngroup() * ntile() * CLN_REC * sizeof(int); }
    size_t state_bytes() const {
        return ((size_t)nfine + (size_t)npix * nstand) * sizeof(double) + pad16((size_t)nstand * sizeof(float)) + pad16((size_t)npix) + rec_bytes() +
               (size_t)2 * ngroup() * 4 * sizeof(int);
    }
    long long comp_offset() const { return (long long)ngroup() * 4 * npix * 4; }
    long long stats_offset() const { return comp_offset() + (long long)ngroup() * niter * CLN_REC * 4; }
    long long span_bytes() const { return stats_offset() + (long long)ngroup() * 16; }
};
static std::mutex g_clmu;
static CleanContext g_cl;

static int clean_destroy_locked() {
    if (!g_cl.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_cl);
    g_cl.alloc.free();
    g_cl = CleanContext();
    return XENG_STATUS_SUCCESS;
}

// sum of w_s w_t over the pairs that count and sum of w_s^2, in float64
static double clean_weight_sum(const float* w, int nstand, int autos, double* squares) {
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < nstand; s++) {
        s1 += (double)w[s];
        s2 += (double)w[s] * (double)w[s];
    }
    *squares = s2;
    return autos ? s1 * s1 : s1 * s1 - s2;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengCleanInitialize(int gpu, int nstand, int nfine, int nfavg, int npix, int niter_max) {
    if (nstand <= 0 || nfine <= 0 || nfavg <= 0 || npix <= 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Clean: bad sizes nstand=%d nfine=%d nfavg=%d npix=%d", nstand, nfine, nfavg, npix);
    if (nfine % nfavg) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Clean: nfavg %d does not divide nfine %d", nfavg, nfine);
    if (niter_max < 1 || niter_max > XENG_CLEAN_MAX_NITER)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Clean: niter_max %d is not in [1, %d]", niter_max, XENG_CLEAN_MAX_NITER);
    if (nstand > XENG_CLEAN_MAX_NSTAND)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Clean: %d stands, the fractions of a component in LDS take %d at the most", nstand, XENG_CLEAN_MAX_NSTAND);
    if (nfine / nfavg > 65535 || npix > (1 << 24) || (double)npix * nstand * 8.0 > (double)XENG_CLEAN_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Clean: %d channel groups x %d pixels x %d stands is more than one launch or a state of %.3g GB takes",
                  nfine / nfavg, npix, nstand, (double)XENG_CLEAN_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_clmu);
    clean_destroy_locked();
    CleanContext& x = g_cl;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nstand = nstand; x.nfine = nfine; x.nfavg = nfavg; x.npix = npix; x.niter_max = niter_max;
    std::vector<float> ones((size_t)nstand, 1.0f);
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = CleanContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Clean: cannot allocate %.3g MB of state", (double)npix * nstand * 8e-6);
    }
    x.freq = (double*)x.alloc.data();
    x.tauT = x.freq + nfine;
    x.w = (float*)(x.tauT + (size_t)npix * nstand);
    x.mask = (uint8_t*)x.w + pad16((size_t)nstand * sizeof(float));
    x.rec = (int*)(x.mask + pad16((size_t)npix));
    x.gstate = (int*)((uint8_t*)x.rec + x.rec_bytes());
    if (hipMemcpy(x.w, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hip_memset_now(x.mask, 1, (size_t)npix) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = CleanContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Clean: cannot upload the weights and the window");
    }
    x.autos = 0;
    x.norm = 1.0 / ((double)nfavg * clean_weight_sum(ones.data(), nstand, 0, &x.dsum));     // (one stand without autos: no pair, infinite until SetWeights)
    x.niter = niter_max;
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengCleanGetInfo(int* ngroup, int* pixel_tile, long long* comp_offset, long long* stats_offset, long long* span_bytes, double* norm) {
    if (!ngroup || !pixel_tile || !comp_offset || !stats_offset || !span_bytes || !norm) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_clmu);
    CleanContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: not initialized");
    *ngroup = x.ngroup();
    *pixel_tile = CLN_PX;
    *comp_offset = x.comp_offset();
    *stats_offset = x.stats_offset();
    *span_bytes = x.span_bytes();
    *norm = x.norm;
    return XENG_STATUS_SUCCESS;
}

int xengCleanSetGeometry(const double* tau, const double* freq) {
    if (!tau || !freq) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetGeometry: null %s", tau ? "frequencies" : "delays");
    std::lock_guard<std::mutex> lk(g_clmu);
    CleanContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: not initialized (call xengCleanInitialize)");
    for (int c = 0; c < x.nfine; c++)
        if (!std::isfinite(freq[c])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetGeometry: frequency %d is not finite", c);
    for (size_t i = 0; i < (size_t)x.npix * x.nstand; i++)
        if (!std::isfinite(tau[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetGeometry: delay %zu is not finite", i);
    std::vector<double> t((size_t)x.npix * x.nstand);       // [nstand][npix]: a wave's reads run along the pixels
    for (int p = 0; p < x.npix; p++)
        for (int s = 0; s < x.nstand; s++) t[(size_t)s * x.npix + p] = tau[(size_t)p * x.nstand + s];
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(x.freq, freq, (size_t)x.nfine * sizeof(double), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.tauT, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    x.geometry = true;
    return XENG_STATUS_SUCCESS;
}

int xengCleanSetWeights(const float* w, int autos) {
    if (!w) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetWeights: null weights");
    std::lock_guard<std::mutex> lk(g_clmu);
    CleanContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: not initialized (call xengCleanInitialize)");
    for (int s = 0; s < x.nstand; s++)
        if (!std::isfinite(w[s]) || w[s] < 0.f) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetWeights: weight %d is %g: not a finite number >= 0", s, (double)w[s]);
    double squares = 0.0;
    const double sum = clean_weight_sum(w, x.nstand, autos != 0, &squares);
    if (!(sum > 0.0))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetWeights: the weights leave no pair of stands%s", autos ? "" : " (autos are off: two stands at least)");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the weights: they apply to the next Run only)
    XENG_HIP(hipMemcpy(x.w, w, (size_t)x.nstand * sizeof(float), hipMemcpyHostToDevice));
    x.autos = autos != 0;
    x.norm = 1.0 / ((double)x.nfavg * sum);
    x.dsum = autos ? 0.0 : squares;
    return XENG_STATUS_SUCCESS;
}

int xengCleanSetWindow(const unsigned char* mask) {
    std::lock_guard<std::mutex> lk(g_clmu);
    CleanContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: not initialized (call xengCleanInitialize)");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the window)
    if (mask) XENG_HIP(hipMemcpy(x.mask, mask, (size_t)x.npix, hipMemcpyHostToDevice));
    else XENG_HIP(hip_memset_now(x.mask, 1, (size_t)x.npix));
    return XENG_STATUS_SUCCESS;
}

int xengCleanSetControl(int niter, float gain, float threshold, float fraction) {
    if (!(gain > 0.f && gain <= 1.f)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetControl: gain %g is not in (0, 1]", (double)gain);
    if (!std::isfinite(threshold) || threshold < 0.f || !std::isfinite(fraction) || fraction < 0.f)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetControl: threshold %g or fraction %g is not a finite number >= 0", (double)threshold, (double)fraction);
    std::lock_guard<std::mutex> lk(g_clmu);
    CleanContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: not initialized (call xengCleanInitialize)");
    if (niter < 0 || niter > x.niter_max) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CleanSetControl: niter %d is not in [0, %d]", niter, x.niter_max);
    x.niter = niter; x.gain = gain; x.threshold = threshold; x.fraction = fraction;     // (arguments of the launches: nothing in flight reads them)
    return XENG_STATUS_SUCCESS;
}

int xengCleanRun(const void* image_dev, void* out_dev) {
    if (!image_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Clean: null %s", image_dev ? "output" : "input");
    if ((uintptr_t)image_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Clean: input %p or output %p not 16-byte aligned", image_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_clmu);
    CleanContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: not initialized (call xengCleanInitialize)");
    if (!x.geometry) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: no geometry (call xengCleanSetGeometry)");
    if (!std::isfinite(x.norm)) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Clean: the weights leave no pair of stands (call xengCleanSetWeights)");
    XENG_HIP(hipSetDevice(x.gpu));
    uint8_t* out = (uint8_t*)out_dev;
    for (int step = 0; step <= x.niter + 1; step++) {
        const dim3 grid((unsigned)(step <= x.niter ? x.ntile() : 1), (unsigned)x.ngroup());
        hipLaunchKernelGGL(clean_step_kernel, grid, dim3(CLN_PX), clean_lds_bytes(x.nstand), x.stream, (const float*)image_dev, (float*)out,
                           (int*)(out + x.comp_offset()), (int*)(out + x.stats_offset()), x.freq, x.tauT, x.w, x.mask, x.rec, x.gstate, x.nstand, x.npix,
                           x.ntile(), x.nfavg, x.niter, step, x.gain, x.threshold, x.fraction, (float)x.norm, (float)x.dsum);
        stream_tick(STREAM_BEAM);
    }
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

int xengCleanCheckGuards(int* intact) { return beam_context_check_guards(g_clmu, g_cl, g_cl.alloc, "Clean", intact); }
int xengCleanMark(unsigned long long* ticket) { return beam_context_mark(g_clmu, g_cl, "Clean", ticket); }
int xengCleanWait(unsigned long long ticket) { return beam_context_wait(g_clmu, g_cl, "Clean", ticket); }
int xengCleanTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_clmu, g_cl, "Clean", ticket, done); }
int xengCleanSync(void) { return beam_context_sync(g_clmu, g_cl, "Clean"); }

int xengCleanDestroy(void) {
    std::lock_guard<std::mutex> lk(g_clmu);
    return clean_destroy_locked();
}

}  // extern "C"
