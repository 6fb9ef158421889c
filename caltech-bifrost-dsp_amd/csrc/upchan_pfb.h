// Host side of the PFB front end of every context that upchannelises (xeng<Name>SetPfb of Upchan, UpchanCorr, UpchanSpectra and
// UpchanSumBeams; the kernels' half is uc_pfb_frame in upchan_kernels.h), and of the u8 gulp that the first three read, in one
// part or two.  A context owns its coefficients and a history of the last (ntap - 1) * N samples u8 [(ntap - 1) * N][nchan][ninput],
// refreshed from each gulp's tail by D2D copies on the context's stream right after the launch that read the previous history:
// the next launch on that stream is the only reader, so one buffer suffices.  (UpchanSumBeams keeps float2 rows in two halves,
// and its kernel writes the history itself.)
//
// What holds for every context, stated here once:
//  - Every argument that can be is checked before the context is looked at: a bad call is told apart from a missing context
//    (INVALID_ARGUMENT against INVALID_STATE), and nothing is launched.  What depends on the context's sizes is checked right after.
//  - SetPfb waits for the stream before it replaces coefficients and history (launches in flight read both); the new history is
//    marked empty; when it fails the previous state is intact.
//  - In a run the order on the stream is: launch, history copies, stream_tick(STREAM_BEAM), so that the stamp of the input span
//    covers the copies; hipGetLastError comes after the tick.  A prime ticks once after its copies.
#pragma once
#include <cmath>

#include "upchan_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct PfbState {
    int ntap = 1;
    float* h = nullptr;                 // [ntap][N] on the device; null: the plain FFT (the kernels without a UcPfb)
    uint8_t* hist = nullptr;            // u8 [(ntap - 1) * N][nchan][ninput]; null when ntap = 1
    bool valid = false;                 // hist holds the samples right before the next gulp

    void release() {
        if (h) (void)hipFree(h);
        if (hist) (void)hipFree(hist);
        *this = PfbState();
    }
    UcPfb args() const { return UcPfb{h, hist, ntap, valid ? 1 : 0}; }
};

// a context with a PFB front end: what the functions below need of it
struct PfbContext : BeamStreamContext {
    int ntime = 0, nupchan = 0;         // samples per gulp, fine channels per channel (N)
    size_t pfb_row = 0;                 // bytes of history per sample: nchan * ninput of u8
    PfbState pfb;                       // xeng<Name>SetPfb (ntap 1 without coefficients: the plain FFT)
};

// Replaces s (the caller has waited for the context's stream): coefficients uploaded, a history of row bytes per sample
// allocated and marked empty.  On failure s is left as it was.
inline int pfb_set(const char* who, PfbState& s, int ntap, const float* coeffs, int nupchan, size_t row) {
    PfbState n;
    n.ntap = ntap;
    const size_t hbytes = (size_t)(ntap - 1) * nupchan * row;
    if ((coeffs && hipMalloc(&n.h, (size_t)ntap * nupchan * sizeof(float)) != hipSuccess) ||
        (hbytes && hipMalloc(&n.hist, hbytes) != hipSuccess) ||
        (coeffs && hipMemcpy(n.h, coeffs, (size_t)ntap * nupchan * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipGetLastError();
        n.release();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "%sSetPfb: cannot set up %d PFB taps (%.3g MB of history)", who, ntap, hbytes * 1e-6);
    }
    s.release();
    s = n;
    return XENG_STATUS_SUCCESS;
}

// xeng<who>SetPfb.  lk is the context's mutex, not locked yet: taken here once the arguments have passed, and still held on
// return for what the caller has to add.
inline int pfb_configure(std::unique_lock<std::mutex>& lk, PfbContext& x, const char* who, int ntap, const float* coeffs) {
    if (ntap < 1 || ntap > UC_MAXTAP) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%sSetPfb: %d PFB taps, not 1 to %d", who, ntap, UC_MAXTAP);
    if (!coeffs && ntap > 1) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%sSetPfb: %d PFB taps without coefficients", who, ntap);
    lk.lock();
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "%s: not initialized (call xeng%sInitialize)", who, who);
    // what needs the context's sizes: finite coefficients, a gulp at least as long as the history
    if (coeffs)
        for (int m = 0; m < ntap * x.nupchan; m++)
            if (!std::isfinite(coeffs[m])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%sSetPfb: PFB coefficient %d is not finite", who, m);
    if ((long long)(ntap - 1) * x.nupchan > x.ntime)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%sSetPfb: gulps of %d samples are shorter than the PFB history of %d x %d", who, x.ntime,
                  ntap - 1, x.nupchan);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    return pfb_set(who, x.pfb, ntap, coeffs, x.nupchan, x.pfb_row);
}

// The u8 gulp of xeng<who><op>[Parts], in one part (*in1 null: *in1 = in0, *ntime0 = ntime) or two (samples [*ntime0, ntime) at
// *in1), each part whole frames of nupchan samples.  lk as in pfb_configure: locked here, between the checks that need no
// context and the one that does, and held on return.
inline int gulp_begin(std::unique_lock<std::mutex>& lk, const PfbContext& x, const char* who, const char* op, const void* in0,
                      const void** in1, int* ntime0) {
    if (!in0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s%s: null input", who, op);
    if (*in1 && *ntime0 <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s%s: first part of %d samples", who, op, *ntime0);
    lk.lock();
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "%s: not initialized (call xeng%sInitialize)", who, who);
    if (!*in1) { *in1 = in0; *ntime0 = x.ntime; }
    else if (*ntime0 >= x.ntime || *ntime0 % x.nupchan)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s%s: parts of %d + %d samples: both must be positive multiples of nupchan %d", who, op,
                  *ntime0, x.ntime - *ntime0, x.nupchan);
    return XENG_STATUS_SUCCESS;
}

// The history becomes the last (ntap - 1) * N samples of this gulp, the parts as gulp_begin left them.  One copy, or two when
// the tail straddles ntime0.
inline int pfb_refresh(PfbContext& x, const void* in0_dev, int ntime0, const void* in1_dev) {
    PfbState& s = x.pfb;
    const uint8_t* in0 = (const uint8_t*)in0_dev;
    const uint8_t* in1 = (const uint8_t*)in1_dev;
    const size_t row = x.pfb_row;
    const int nh = (s.ntap - 1) * x.nupchan;
    if (!nh) return XENG_STATUS_SUCCESS;
    const int t = x.ntime - nh;                                 // first sample of the tail
    if (t >= ntime0) {
        XENG_HIP(hipMemcpyAsync(s.hist, in1 + (size_t)(t - ntime0) * row, (size_t)nh * row, hipMemcpyDeviceToDevice, x.stream));
    } else {
        XENG_HIP(hipMemcpyAsync(s.hist, in0 + (size_t)t * row, (size_t)(ntime0 - t) * row, hipMemcpyDeviceToDevice, x.stream));
        if (x.ntime > ntime0)
            XENG_HIP(hipMemcpyAsync(s.hist + (size_t)(ntime0 - t) * row, in1, (size_t)(x.ntime - ntime0) * row, hipMemcpyDeviceToDevice, x.stream));
    }
    s.valid = true;
    return XENG_STATUS_SUCCESS;
}

// After the launch that read the history, on the same stream and before the caller's stream_tick: the launch's error looked at,
// the history for the next gulp enqueued.
inline int pfb_after_launch(PfbContext& x, const void* in0, int ntime0, const void* in1) {
    if (!x.pfb.hist) return XENG_STATUS_SUCCESS;
    XENG_HIP(hipGetLastError());
    return pfb_refresh(x, in0, ntime0, in1);
}

// xeng<who>Prime[Parts]: the history from this gulp's tail, nothing launched
inline int pfb_prime(std::mutex& mu, PfbContext& x, const char* who, const void* in0, int ntime0, const void* in1) {
    std::unique_lock<std::mutex> lk(mu, std::defer_lock);
    int rc = gulp_begin(lk, x, who, "Prime", in0, &in1, &ntime0);
    if (rc || !x.pfb.hist) return rc;   // (no history without taps before the frame's own)
    XENG_HIP(hipSetDevice(x.gpu));
    if ((rc = pfb_refresh(x, in0, ntime0, in1))) return rc;
    stream_tick(STREAM_BEAM);
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng
