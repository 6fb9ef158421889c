// Host side of the PFB front end shared by the Upchan and UpchanCorr contexts (xengUpchanSetPfb, xengUpchanCorrSetPfb; the
// kernels' half is uc_pfb_frame in upchan_kernels.h).  A context owns its coefficients and a history of the last (ntap - 1) * N
// samples u8 [(ntap - 1) * N][nchan][ninput], refreshed from each gulp's tail by D2D copies on the context's stream right after
// the launch that read the previous history: the next launch on that stream is the only reader, so one buffer suffices.
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

// what can be refused without a context
inline int pfb_check_args(const char* who, int ntap, const float* coeffs) {
    if (ntap < 1 || ntap > UC_MAXTAP) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s: %d PFB taps, not 1 to %d", who, ntap, UC_MAXTAP);
    if (!coeffs && ntap > 1) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s: %d PFB taps without coefficients", who, ntap);
    return XENG_STATUS_SUCCESS;
}

// what needs the context's sizes: finite coefficients, a gulp at least as long as the history
inline int pfb_check_sizes(const char* who, int ntap, const float* coeffs, int nupchan, int ntime) {
    if (coeffs)
        for (int m = 0; m < ntap * nupchan; m++)
            if (!std::isfinite(coeffs[m])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s: PFB coefficient %d is not finite", who, m);
    if ((long long)(ntap - 1) * nupchan > ntime)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s: gulps of %d samples are shorter than the PFB history of %d x %d", who, ntime, ntap - 1,
                  nupchan);
    return XENG_STATUS_SUCCESS;
}

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
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "%s: cannot set up %d PFB taps (%.3g MB of history)", who, ntap, hbytes * 1e-6);
    }
    s.release();
    s = n;
    return XENG_STATUS_SUCCESS;
}

// After a launch that read s.hist, on the same stream and before that stream's clock ticks (so that the stamp of the input span
// covers the copies): the history becomes the last (ntap - 1) * N samples of this gulp, samples [0, ntime0) at in0 and
// [ntime0, ntime) at in1 (one part: in1 = in0, ntime0 = ntime).  One copy, or two when the tail straddles ntime0.
inline int pfb_refresh(PfbState& s, hipStream_t stream, const uint8_t* in0, int ntime0, const uint8_t* in1, int ntime, int nupchan, size_t row) {
    const int nh = (s.ntap - 1) * nupchan;
    if (!nh) return XENG_STATUS_SUCCESS;
    const int t = ntime - nh;                                   // first sample of the tail
    if (t >= ntime0) {
        XENG_HIP(hipMemcpyAsync(s.hist, in1 + (size_t)(t - ntime0) * row, (size_t)nh * row, hipMemcpyDeviceToDevice, stream));
    } else {
        XENG_HIP(hipMemcpyAsync(s.hist, in0 + (size_t)t * row, (size_t)(ntime0 - t) * row, hipMemcpyDeviceToDevice, stream));
        if (ntime > ntime0)
            XENG_HIP(hipMemcpyAsync(s.hist + (size_t)(ntime0 - t) * row, in1, (size_t)(ntime - ntime0) * row, hipMemcpyDeviceToDevice, stream));
    }
    s.valid = true;
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng
