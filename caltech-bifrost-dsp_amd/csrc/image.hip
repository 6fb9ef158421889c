// Host side of the imager (UpchanImage; image_kernels.h): a process-global context of its own on the beamformer's stream
// (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "image_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct ImageContext : BeamStreamContext {
    int nstand = 0, nfine = 0, nfavg = 0, npix = 0;
    GuardedState alloc;                 // the state between its guard bands (xengImageCheckGuards)
    double* freq = nullptr;             // f64[nfine], inside alloc
    double* tau = nullptr;              // f64[npix][nstand], behind it
    float* w = nullptr;                 // f32[nstand], behind that
    bool geometry = false;              // SetGeometry has been called
    int autos = 0;
    double norm = 0.0;                  // 1 / (nfavg sum w_s w_t), float64; the kernel takes it rounded once

    size_t state_bytes() const { return ((size_t)nfine + (size_t)npix * nstand) * sizeof(double) + (((size_t)nstand * sizeof(float) + 15) & ~(size_t)15); }
};
static std::mutex g_immu;
static ImageContext g_im;

static int image_destroy_locked() {
    if (!g_im.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_im);
    g_im.alloc.free();
    g_im = ImageContext();
    return XENG_STATUS_SUCCESS;
}

// sum of w_s w_t over the pairs that count, in float64; <= 0: nothing to image
static double image_weight_sum(const float* w, int nstand, int autos) {
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < nstand; s++) {
        s1 += (double)w[s];
        s2 += (double)w[s] * (double)w[s];
    }
    return autos ? s1 * s1 : s1 * s1 - s2;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengImageInitialize(int gpu, int nstand, int nfine, int nfavg, int npix) {
    if (nstand <= 0 || nfine <= 0 || nfavg <= 0 || npix <= 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Image: bad sizes nstand=%d nfine=%d nfavg=%d npix=%d", nstand, nfine, nfavg, npix);
    if (nfine % nfavg) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Image: nfavg %d does not divide nfine %d", nfavg, nfine);
    if (nstand > XENG_IMAGE_MAX_NSTAND)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Image: %d stands, the steering tile in LDS takes %d at the most", nstand, XENG_IMAGE_MAX_NSTAND);
    if (nfine / nfavg > 65535 || npix > (1 << 24) || (double)npix * nstand * 8.0 > (double)XENG_IMAGE_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Image: %d channel groups x %d pixels x %d stands is more than one launch or a state of %.3g GB takes",
                  nfine / nfavg, npix, nstand, (double)XENG_IMAGE_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_immu);
    image_destroy_locked();
    ImageContext& x = g_im;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nstand = nstand; x.nfine = nfine; x.nfavg = nfavg; x.npix = npix;
    const size_t lds = image_lds_bytes(nstand);
    if (lds > (64 << 10) && hipFuncSetAttribute((const void*)image_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        x = ImageContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Image: %d stands need %zu bytes of LDS, which the device refuses", nstand, lds);
    }
    std::vector<float> ones((size_t)nstand, 1.0f);
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = ImageContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Image: cannot allocate %.3g MB of state", (double)npix * nstand * 8e-6);
    }
    x.freq = (double*)x.alloc.data();
    x.tau = x.freq + nfine;
    x.w = (float*)(x.tau + (size_t)npix * nstand);
    if (hipMemcpy(x.w, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = ImageContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Image: cannot upload the weights");
    }
    x.autos = 0;
    x.norm = 1.0 / ((double)nfavg * image_weight_sum(ones.data(), nstand, 0));      // (one stand without autos: no pair, infinite until SetWeights)
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengImageGetInfo(int* ngroup, int* pixel_tile, int* lds_bytes, double* norm) {
    if (!ngroup || !pixel_tile || !lds_bytes || !norm) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImageGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_immu);
    ImageContext& x = g_im;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Image: not initialized");
    *ngroup = x.nfine / x.nfavg;
    *pixel_tile = IMG_PX;
    *lds_bytes = (int)image_lds_bytes(x.nstand);
    *norm = x.norm;
    return XENG_STATUS_SUCCESS;
}

int xengImageSetGeometry(const double* tau, const double* freq) {
    if (!tau || !freq) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImageSetGeometry: null %s", tau ? "frequencies" : "delays");
    std::lock_guard<std::mutex> lk(g_immu);
    ImageContext& x = g_im;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Image: not initialized (call xengImageInitialize)");
    for (int c = 0; c < x.nfine; c++)
        if (!std::isfinite(freq[c])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImageSetGeometry: frequency %d is not finite", c);
    for (size_t i = 0; i < (size_t)x.npix * x.nstand; i++)
        if (!std::isfinite(tau[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImageSetGeometry: delay %zu is not finite", i);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(x.freq, freq, (size_t)x.nfine * sizeof(double), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.tau, tau, (size_t)x.npix * x.nstand * sizeof(double), hipMemcpyHostToDevice));
    x.geometry = true;
    return XENG_STATUS_SUCCESS;
}

int xengImageSetWeights(const float* w, int autos) {
    if (!w) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImageSetWeights: null weights");
    std::lock_guard<std::mutex> lk(g_immu);
    ImageContext& x = g_im;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Image: not initialized (call xengImageInitialize)");
    for (int s = 0; s < x.nstand; s++)
        if (!std::isfinite(w[s]) || w[s] < 0.f) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImageSetWeights: weight %d is %g: not a finite number >= 0", s, (double)w[s]);
    const double sum = image_weight_sum(w, x.nstand, autos != 0);
    if (!(sum > 0.0))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImageSetWeights: the weights leave no pair of stands%s", autos ? "" : " (autos are off: two stands at least)");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the weights: they apply to the next Run only)
    XENG_HIP(hipMemcpy(x.w, w, (size_t)x.nstand * sizeof(float), hipMemcpyHostToDevice));
    x.autos = autos != 0;
    x.norm = 1.0 / ((double)x.nfavg * sum);
    return XENG_STATUS_SUCCESS;
}

int xengImageRun(const void* vis_dev, void* out_dev) {
    if (!vis_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Image: null %s", vis_dev ? "output" : "input");
    if ((uintptr_t)vis_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Image: input %p or output %p not 16-byte aligned", vis_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_immu);
    ImageContext& x = g_im;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Image: not initialized (call xengImageInitialize)");
    if (!x.geometry) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Image: no geometry (call xengImageSetGeometry)");
    if (!std::isfinite(x.norm)) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Image: the weights leave no pair of stands (call xengImageSetWeights)");
    XENG_HIP(hipSetDevice(x.gpu));
    const dim3 grid((unsigned)((x.npix + IMG_PX - 1) / IMG_PX), (unsigned)(x.nfine / x.nfavg));
    hipLaunchKernelGGL(image_kernel, grid, dim3(IMG_THREADS), image_lds_bytes(x.nstand), x.stream, (const float2*)vis_dev, x.freq, x.tau, x.w, (float*)out_dev,
                       x.nstand, x.npix, x.nfavg, x.autos, (float)x.norm);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

int xengImageCheckGuards(int* intact) { return beam_context_check_guards(g_immu, g_im, g_im.alloc, "Image", intact); }
int xengImageMark(unsigned long long* ticket) { return beam_context_mark(g_immu, g_im, "Image", ticket); }
int xengImageWait(unsigned long long ticket) { return beam_context_wait(g_immu, g_im, "Image", ticket); }
int xengImageTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_immu, g_im, "Image", ticket, done); }
int xengImageSync(void) { return beam_context_sync(g_immu, g_im, "Image"); }

int xengImageDestroy(void) {
    std::lock_guard<std::mutex> lk(g_immu);
    return image_destroy_locked();
}

}  // extern "C"
