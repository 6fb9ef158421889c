// Host side of the FFT periodicity search (BeamPeriodSearch; period_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "period_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct PeriodContext : BeamStreamContext {
    int npair = 0, ndm = 0, nwin = 0, nprod = 0, nt = 0, nstack = 0, nlevel = 0, nwhite = 0, kmin = 0;
    int nser = 0;                       // npair * ndm
    int L = 0, lb = 0;                  // log2 (nt / 2), log2 nwhite
    GuardedState alloc;                 // the state between its guard bands (xengPeriodCheckGuards)
    float* tbuf = nullptr;              // f32[nser][nt], inside alloc
    float* A = nullptr;                 // f32[nser][nt/2], behind it
    float2* tw = nullptr;               // float2[nt/2]
    float2* twu = nullptr;              // float2[nt/4]
    float* cnt = nullptr;               // f32[nt/2 / nwhite]
    uint8_t* keep = nullptr;            // u8[nt/2]
    long long nwindows = 0;             // windows taken since the last reset
    int nseg = 0;                       // segments of the stack in progress that are complete
    int nseg_A = 0;                     // segments A holds (nstack after the call that completed a stack; 0: nothing current)
    long long nstacks = 0;              // stacks completed since the last reset

    size_t state_bytes() const {
        const size_t n = (size_t)nt / 2;
        return ((size_t)nser * nt + (size_t)nser * n) * sizeof(float) + n * sizeof(float2) + n / 2 * sizeof(float2) + n / nwhite * sizeof(float) + n;
    }
};
static std::mutex g_prmu;
static PeriodContext g_pr;

static int period_destroy_locked() {
    if (!g_pr.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_pr);
    g_pr.alloc.free();
    g_pr = PeriodContext();
    return XENG_STATUS_SUCCESS;
}

static int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}

// the mask and, per whitening block, the number of its bins that count (k >= 1, kept), uploaded; the caller has made the stream idle
static hipError_t period_upload_mask(const PeriodContext& x, const unsigned char* keep) {
    const int n = x.nt / 2;
    std::vector<uint8_t> m((size_t)n, 1);
    if (keep)
        for (int k = 0; k < n; k++) m[k] = keep[k] ? 1 : 0;
    std::vector<float> cnt((size_t)(n / x.nwhite), 0.f);
    for (int k = 1; k < n; k++) cnt[k / x.nwhite] += (float)m[k];
    hipError_t e = hipMemcpy(x.keep, m.data(), m.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    return hipMemcpy(x.cnt, cnt.data(), cnt.size() * sizeof(float), hipMemcpyHostToDevice);
}

template <int NPROD>
static void period_ingest(const PeriodContext& x, const float* in, int nc, int slot0) {
    const dim3 g((unsigned)((x.nser + PR_TILE - 1) / PR_TILE), (unsigned)((nc + PR_TILE - 1) / PR_TILE));
    hipLaunchKernelGGL((period_ingest_kernel<NPROD>), g, dim3(256), 0, x.stream, in, x.tbuf, x.nser, x.nt, slot0, nc);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengPeriodInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nt, int nstack, int nlevel, int nwhite, int kmin) {
    if (npair <= 0 || ndm <= 0 || nwin <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: bad sizes npair=%d ndm=%d nwin=%d", npair, ndm, nwin);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: nprod %d not 1 (I) or 4 (XX, YY, Re XY*, Im XY*)", nprod);
    if (nt < (1 << 8) || nt > (1 << 14) || (nt & (nt - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: a segment of %d windows, not a power of two from 2^8 to 2^14", nt);
    if (nstack < 1) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: %d segments in a stack", nstack);
    if (nlevel < 1 || nlevel > PR_MAX_LEVEL) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: %d harmonic levels, not 1 to %d", nlevel, PR_MAX_LEVEL);
    if (nwhite < 8 || nwhite > nt / 2 || (nwhite & (nwhite - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: a whitening block of %d bins, not a power of two from 8 to nt/2 = %d", nwhite, nt / 2);
    if (kmin < 1 || kmin >= nt / 32) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: kmin %d not in 1 .. nt/32 - 1 = %d", kmin, nt / 32 - 1);
    if (nwin > nt) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: %d windows a call are more than a segment of %d", nwin, nt);
    if ((long long)npair * ndm > (1LL << 24))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: %d pairs x %d trials is more than one launch takes", npair, ndm);
    if ((double)npair * ndm * nt * 6.0 > (double)XENG_PERIOD_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: %d series of %d windows need %.3g GB of state, above the limit of %.3g GB", npair * ndm, nt,
                  (double)npair * ndm * nt * 6e-9, (double)XENG_PERIOD_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_prmu);
    period_destroy_locked();
    PeriodContext& x = g_pr;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.npair = npair; x.ndm = ndm; x.nwin = nwin; x.nprod = nprod; x.nt = nt; x.nstack = nstack; x.nlevel = nlevel; x.nwhite = nwhite; x.kmin = kmin;
    x.nser = npair * ndm;
    const int n = nt / 2;
    x.L = ilog2(n);
    x.lb = ilog2(nwhite);
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, x.gpu) != hipSuccess || (size_t)lds < (size_t)n * sizeof(float2)) {
        (void)hipGetLastError();
        x = PeriodContext();
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: the FFT of a segment of %d windows needs %zu bytes of LDS, a work-group may take %d", nt,
                  (size_t)n * sizeof(float2), lds);
    }
    // twiddles: float64, rounded once
    std::vector<float2> tw((size_t)n + n / 2);
    const double step = -2.0 * 3.14159265358979323846 / (double)nt;
    for (int k = 0; k < n; k++) tw[k] = make_float2((float)std::cos(step * k), (float)std::sin(step * k));
    for (int t = 0; t < n / 2; t++) {
        int k = 0;
        for (int b = 0; b < x.L; b++) k |= ((2 * t >> b) & 1) << (x.L - 1 - b);
        tw[(size_t)n + t] = tw[k];
    }
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = PeriodContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Period: cannot allocate %.3g MB of state", (double)npair * ndm * nt * 6e-6);
    }
    x.tbuf = (float*)x.alloc.data();
    x.A = x.tbuf + (size_t)x.nser * nt;
    x.tw = (float2*)(x.A + (size_t)x.nser * n);
    x.twu = x.tw + n;
    x.cnt = (float*)(x.twu + n / 2);
    x.keep = (uint8_t*)(x.cnt + n / nwhite);
    if (hipMemcpy(x.tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess || period_upload_mask(x, nullptr) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = PeriodContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Period: cannot upload the twiddles and the mask");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengPeriodSetMask(const unsigned char* keep) {
    std::lock_guard<std::mutex> lk(g_prmu);
    PeriodContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Period: not initialized (call xengPeriodInitialize)");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the mask)
    XENG_HIP(period_upload_mask(x, keep));
    return XENG_STATUS_SUCCESS;
}

int xengPeriodRun(const void* in_dev, int nwin_call, void* out_dev, int* completed) {
    if (!in_dev || !completed) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: null %s", in_dev ? "result" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_prmu);
    PeriodContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Period: not initialized (call xengPeriodInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    const int pos = (int)(x.nwindows % x.nt);
    const int head = nwin_call < x.nt - pos ? nwin_call : x.nt - pos;   // windows of the call that go into the segment in progress
    const bool seg_done = pos + head == x.nt, stack_done = seg_done && x.nseg + 1 == x.nstack;
    if (stack_done && !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Period: the call completes a stack and has a null output");
    XENG_HIP(hipSetDevice(x.gpu));
    const float* in = (const float*)in_dev;
    if (x.nprod == 1)
        period_ingest<1>(x, in, head, pos);
    else
        period_ingest<4>(x, in, head, pos);
    if (seg_done) {
        hipLaunchKernelGGL(period_spectrum_kernel, dim3((unsigned)x.nser), dim3(PR_THREADS), (size_t)(x.nt / 2) * sizeof(float2), x.stream, x.tbuf, x.A,
                           x.keep, x.cnt, x.tw, x.twu, (PeriodRecord*)out_dev, x.L, x.lb, x.nlevel, x.kmin, (int)(x.nseg == 0), (int)stack_done);
        if (nwin_call > head) {
            in += (size_t)head * x.nser * x.nprod;
            if (x.nprod == 1)
                period_ingest<1>(x, in, nwin_call - head, 0);
            else
                period_ingest<4>(x, in, nwin_call - head, 0);
        }
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows += nwin_call;
    if (seg_done) {
        x.nseg_A = x.nseg + 1;
        x.nseg = stack_done ? 0 : x.nseg + 1;
        if (stack_done) x.nstacks++;
    }
    *completed = stack_done ? 1 : 0;
    return XENG_STATUS_SUCCESS;
}

int xengPeriodReset(void) {
    std::lock_guard<std::mutex> lk(g_prmu);
    PeriodContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Period: not initialized");
    x.nwindows = 0;                     // (the partial segment and the partial stack are dropped by index: the next segment
    x.nseg = 0;                         //  fills the time buffer from slot 0 and, as a stack's first, stores A)
    x.nseg_A = 0;
    x.nstacks = 0;
    return XENG_STATUS_SUCCESS;
}

int xengPeriodGetInfo(long long* nwindows_since_reset, int* nseg_in_stack, long long* nstacks_complete) {
    if (!nwindows_since_reset || !nseg_in_stack || !nstacks_complete) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeriodGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_prmu);
    PeriodContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Period: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nseg_in_stack = x.nseg;
    *nstacks_complete = x.nstacks;
    return XENG_STATUS_SUCCESS;
}

int xengPeriodGetSpectrum(float* A_host, int* nseg) {
    if (!A_host || !nseg) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PeriodGetSpectrum: null result");
    std::lock_guard<std::mutex> lk(g_prmu);
    PeriodContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Period: not initialized");
    if (x.nseg_A == 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "PeriodGetSpectrum: no segment is complete since the reset");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    XENG_HIP(hipMemcpy(A_host, x.A, (size_t)x.nser * (x.nt / 2) * sizeof(float), hipMemcpyDeviceToHost));
    *nseg = x.nseg_A;
    return XENG_STATUS_SUCCESS;
}

int xengPeriodCheckGuards(int* intact) { return beam_context_check_guards(g_prmu, g_pr, g_pr.alloc, "Period", intact); }
int xengPeriodMark(unsigned long long* ticket) { return beam_context_mark(g_prmu, g_pr, "Period", ticket); }
int xengPeriodWait(unsigned long long ticket) { return beam_context_wait(g_prmu, g_pr, "Period", ticket); }
int xengPeriodTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_prmu, g_pr, "Period", ticket, done); }
int xengPeriodSync(void) { return beam_context_sync(g_prmu, g_pr, "Period"); }

int xengPeriodDestroy(void) {
    std::lock_guard<std::mutex> lk(g_prmu);
    return period_destroy_locked();
}

}  // extern "C"
