// Host side of the flagging stage (UpchanFlag; flag_kernels.h): a process-global context of its own on the beamformer's stream
// (BeamStreamContext, xeng_common.h).
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "flag_kernels.h"
#include "xeng_common.h"

namespace xeng {

static_assert(XENG_FLAG_MAX_NSTAND == FL_MAX_NSTAND && XENG_FLAG_MAX_NFINE == FL_MAX_NFINE && XENG_FLAG_MAX_WCHAN == FL_MAX_WCHAN,
              "the limits of include/xeng.h are the kernels'");

struct FlagContext : BeamStreamContext {
    int nstand = 0, nfine = 0;
    GuardedState alloc;                 // the state between its guard bands (xengFlagCheckGuards)
    float* part = nullptr;              // f32[nfine][2][nstand][ntile], inside alloc
    float* autos = nullptr;             // f32[nfine][2][nstand], behind it
    float* w = nullptr;                 // f32[nstand]
    float2* zero = nullptr;             // 16 bytes of zeros, 16-byte aligned, at the end of the state
    float k_cross = 0.f, k_auto = 0.f, k_chan = 0.f;
    double nsig_cross = 0, nsig_auto = 0, nsig_chan = 0;
    int wchan = 0;

    int ntile() const { return (nstand + FL_T - 1) / FL_T; }
    size_t state_bytes() const {
        return zero_offset() + 16;
    }
    size_t zero_offset() const {
        const size_t n = ((size_t)nfine * 2 * nstand * (ntile() + 1) + (size_t)nstand) * sizeof(float);
        return (n + 15) & ~(size_t)15;
    }
};
static std::mutex g_flmu;
static FlagContext g_fl;

static int flag_destroy_locked() {
    if (!g_fl.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_fl);
    g_fl.alloc.free();
    g_fl = FlagContext();
    return XENG_STATUS_SUCCESS;
}

// k = float32(nsig * 1.4826): float64 on the host, rounded once
static float flag_threshold(double nsig) { return (float)(nsig * 1.4826); }

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengFlagInitialize(int gpu, int nstand, int nfine) {
    if (nstand <= 0 || nfine <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Flag: bad sizes nstand=%d nfine=%d", nstand, nfine);
    if (nstand < 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Flag: %d stands, the tests need 4 at the least", nstand);
    if (nstand > XENG_FLAG_MAX_NSTAND) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Flag: %d stands, %d at the most", nstand, XENG_FLAG_MAX_NSTAND);
    if (nfine > XENG_FLAG_MAX_NFINE) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Flag: %d fine channels, %d at the most", nfine, XENG_FLAG_MAX_NFINE);
    std::lock_guard<std::mutex> lk(g_flmu);
    flag_destroy_locked();
    FlagContext& x = g_fl;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nstand = nstand; x.nfine = nfine;
    const std::vector<float> ones((size_t)nstand, 1.f);
    bool ok = false;
    if (x.alloc.open(x.state_bytes()) == hipSuccess) {
        x.part = (float*)x.alloc.data();
        x.autos = x.part + (size_t)nfine * 2 * nstand * x.ntile();
        x.w = x.autos + (size_t)nfine * 2 * nstand;
        x.zero = (float2*)(x.alloc.data() + x.zero_offset());
        ok = hipMemcpy(x.w, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        x.alloc.free();
        x = FlagContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Flag: cannot allocate %.3g MB of state", (double)nfine * nstand * 8e-6 * ((nstand + FL_T - 1) / FL_T + 1));
    }
    x.nsig_cross = XENG_FLAG_DEFAULT_NSIG_CROSS; x.nsig_auto = XENG_FLAG_DEFAULT_NSIG_AUTO; x.nsig_chan = XENG_FLAG_DEFAULT_NSIG_CHAN;
    x.k_cross = flag_threshold(x.nsig_cross); x.k_auto = flag_threshold(x.nsig_auto); x.k_chan = flag_threshold(x.nsig_chan);
    x.wchan = XENG_FLAG_DEFAULT_WCHAN;
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengFlagGetInfo(long long* mask_bytes, long long* stats_bytes, long long* chan_bytes, int* lds_bytes) {
    if (!mask_bytes || !stats_bytes || !chan_bytes || !lds_bytes) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FlagGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_flmu);
    FlagContext& x = g_fl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Flag: not initialized");
    *mask_bytes = (long long)x.nfine * 2 * x.nstand;
    *stats_bytes = (long long)x.nfine * 2 * x.nstand * 2 * (long long)sizeof(float);
    *chan_bytes = (long long)x.nfine * 2 * 4 * (long long)sizeof(float);
    *lds_bytes = (int)std::max(flag_stats_lds_bytes(), std::max(flag_test_lds_bytes(), flag_chan_lds_bytes()));
    return XENG_STATUS_SUCCESS;
}

int xengFlagSetWeights(const float* w) {
    if (!w) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FlagSetWeights: null weights");
    std::lock_guard<std::mutex> lk(g_flmu);
    FlagContext& x = g_fl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Flag: not initialized (call xengFlagInitialize)");
    int non = 0;
    for (int s = 0; s < x.nstand; s++) {
        if (!std::isfinite(w[s]) || w[s] < 0.f) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FlagSetWeights: weight %d is %g: not a finite number >= 0", s, (double)w[s]);
        non += w[s] > 0.f;
    }
    if (non < 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FlagSetWeights: the weights leave %d stands, the tests need 4 at the least", non);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the weights: they apply to the next Run only)
    XENG_HIP(hipMemcpy(x.w, w, (size_t)x.nstand * sizeof(float), hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengFlagSetControl(double nsig_cross, double nsig_auto, double nsig_chan, int wchan) {
    for (double v : {nsig_cross, nsig_auto, nsig_chan})
        if (!std::isfinite(v) || v < 0 || !std::isfinite(flag_threshold(v)))
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FlagSetControl: nsig %g is not a finite number >= 0", v);
    if (wchan < 0 || wchan > XENG_FLAG_MAX_WCHAN) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FlagSetControl: wchan %d outside [0, %d]", wchan, XENG_FLAG_MAX_WCHAN);
    std::lock_guard<std::mutex> lk(g_flmu);
    FlagContext& x = g_fl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Flag: not initialized (call xengFlagInitialize)");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (the controls are launch arguments: the wait only keeps the setters alike)
    x.nsig_cross = nsig_cross; x.nsig_auto = nsig_auto; x.nsig_chan = nsig_chan;
    x.k_cross = flag_threshold(nsig_cross); x.k_auto = flag_threshold(nsig_auto); x.k_chan = flag_threshold(nsig_chan);
    x.wchan = wchan;
    return XENG_STATUS_SUCCESS;
}

int xengFlagGetControl(double* nsig_cross, double* nsig_auto, double* nsig_chan, int* wchan) {
    if (!nsig_cross || !nsig_auto || !nsig_chan || !wchan) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FlagGetControl: null result");
    std::lock_guard<std::mutex> lk(g_flmu);
    FlagContext& x = g_fl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Flag: not initialized");
    *nsig_cross = x.nsig_cross; *nsig_auto = x.nsig_auto; *nsig_chan = x.nsig_chan; *wchan = x.wchan;
    return XENG_STATUS_SUCCESS;
}

int xengFlagRun(const void* vis_dev, void* mask_dev, void* stats_dev, void* chan_dev) {
    if (!vis_dev || !mask_dev || !stats_dev || !chan_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Flag: null %s", !vis_dev ? "input" : "output");
    if ((uintptr_t)vis_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Flag: input %p not 16-byte aligned", vis_dev);
    if ((uintptr_t)stats_dev % 4 || (uintptr_t)chan_dev % 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Flag: stats %p or chan %p not 4-byte aligned", stats_dev, chan_dev);
    std::lock_guard<std::mutex> lk(g_flmu);
    FlagContext& x = g_fl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Flag: not initialized (call xengFlagInitialize)");
    XENG_HIP(hipSetDevice(x.gpu));
    const int nt = x.ntile();
    hipLaunchKernelGGL(flag_stats_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)x.nfine), dim3(FL_THREADS), 0, x.stream, (const float2*)vis_dev, x.w, x.zero,
                       x.part, x.autos, x.nstand);
    hipLaunchKernelGGL(flag_test_kernel, dim3(2, (unsigned)x.nfine), dim3(FL_TEST_THREADS), 0, x.stream, x.part, x.autos, x.w, (unsigned char*)mask_dev,
                       (float*)stats_dev, (float*)chan_dev, x.nstand, x.k_cross, x.k_auto);
    hipLaunchKernelGGL(flag_chan_kernel, dim3(2), dim3(FL_CHAN_THREADS), 0, x.stream, (unsigned char*)mask_dev, (float*)chan_dev, x.nstand, x.nfine, x.k_chan, x.wchan);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

int xengFlagCheckGuards(int* intact) { return beam_context_check_guards(g_flmu, g_fl, g_fl.alloc, "Flag", intact); }
int xengFlagMark(unsigned long long* ticket) { return beam_context_mark(g_flmu, g_fl, "Flag", ticket); }
int xengFlagWait(unsigned long long ticket) { return beam_context_wait(g_flmu, g_fl, "Flag", ticket); }
int xengFlagTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_flmu, g_fl, "Flag", ticket, done); }
int xengFlagSync(void) { return beam_context_sync(g_flmu, g_fl, "Flag"); }

int xengFlagDestroy(void) {
    std::lock_guard<std::mutex> lk(g_flmu);
    return flag_destroy_locked();
}

}  // extern "C"
