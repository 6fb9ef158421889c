// Host side of the dedispersed transient search of the images (UpchanImageSearch; imsearch_kernels.h): a process-global context of
// its own on the beamformer's stream (BeamStreamContext, xeng_common.h).
#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

#include "imsearch_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct ImsearchContext : BeamStreamContext {
    int npix = 0, ngroup = 0, ndm = 0, max_delay = 0, nwidth = 0, nstat = 0;
    int npitch = 0;                     // npix rounded up to 4: the rows of the rings
    int T = 0;                          // integrations a boxcar reaches back: 2^(nwidth-1) - 1
    int S = -1;                         // largest delay of the table in use, -1 before SetDelays
    int nused = 0;                      // groups of weight != 0
    GuardedState alloc;                 // state, U, Z between their guard bands (xengImsearchCheckGuards)
    float *state = nullptr, *U = nullptr, *Z = nullptr;
    int *bk = nullptr, *gk = nullptr;   // i32[ndm][nusedp], i32[nusedp]: nused rounded up to IS_CHUNK
    float* wk = nullptr;                // f32[nusedp]
    std::vector<int> delays;            // s[d][g] as set
    std::vector<float> weights;         // all ones until set
    float kappa = 0.f, r_nstat = 0.f;
    long long nint = 0, n_w = 0;        // integrations since the last reset; that count when the weights were last set

    size_t state_words() const { return (size_t)IS_NSTATE * ngroup * npix; }
    size_t u_words() const { return (size_t)(max_delay + 1) * ngroup * npitch; }
    size_t z_words() const { return (size_t)(T + 1) * ndm * npitch; }
    size_t bytes() const { return (state_words() + u_words() + z_words()) * sizeof(float); }
};
static std::mutex g_ismu;
static ImsearchContext g_is;

static void imsearch_free(ImsearchContext& x) {
    x.alloc.free();
    if (x.bk) (void)hipFree(x.bk);
    if (x.gk) (void)hipFree(x.gk);
    if (x.wk) (void)hipFree(x.wk);
}

static int imsearch_destroy_locked() {
    if (!g_is.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_is);
    imsearch_free(g_is);
    g_is = ImsearchContext();
    return XENG_STATUS_SUCCESS;
}

// The compact tables of the groups in use, from the delays and the weights as set; the caller has synchronised the stream.
static int imsearch_upload_tables(ImsearchContext& x) {
    std::vector<int> gk;
    std::vector<float> wk;
    double sum2 = 0.0;
    for (int g = 0; g < x.ngroup; g++)
        if (x.weights[g] != 0.f) {
            gk.push_back(g);
            wk.push_back(x.weights[g]);
            sum2 += (double)x.weights[g] * (double)x.weights[g];
        }
    x.nused = (int)gk.size();
    x.kappa = (float)(1.0 / std::sqrt(sum2));
    const size_t nusedp = (size_t)(x.nused + IS_CHUNK - 1) / IS_CHUNK * IS_CHUNK;   // (whole chunks: the padding names a row that exists, with weight 0)
    gk.resize(nusedp, gk[0]);
    wk.resize(nusedp, 0.f);
    XENG_HIP(hipMemcpy(x.gk, gk.data(), gk.size() * sizeof(int), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.wk, wk.data(), wk.size() * sizeof(float), hipMemcpyHostToDevice));
    if (x.S >= 0) {
        std::vector<int> bk((size_t)x.ndm * nusedp, 0);
        for (int d = 0; d < x.ndm; d++)
            for (int k = 0; k < x.nused; k++) bk[(size_t)d * nusedp + k] = x.S - x.delays[(size_t)d * x.ngroup + gk[k]];
        XENG_HIP(hipMemcpy(x.bk, bk.data(), bk.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    return XENG_STATUS_SUCCESS;
}

template <int NW>
static void imsearch_search_launch(const ImsearchContext& x, float2* out, unsigned ntile, long long n, long long since) {
    hipLaunchKernelGGL((imsearch_search_kernel<NW>), dim3(ntile), dim3(64 * IS_WAVES), 0, x.stream, (const float*)x.U, x.Z, (const int*)x.bk,
                       (const int*)x.gk, (const float*)x.wk, out, x.npix, x.npitch, x.ngroup, x.ndm, x.nused, x.nstat, x.S, n < INT_MAX ? (int)n : INT_MAX,
                       (int)(n % (x.S + 1)), (int)(n % (x.T + 1)), since < x.T ? (int)since : x.T, x.kappa);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengImsearchInitialize(int gpu, int npix, int ngroup, int ndm, int max_delay, int nwidth, int nstat) {
    if (npix <= 0 || ngroup <= 0 || ndm <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: bad sizes npix=%d ngroup=%d ndm=%d", npix, ngroup, ndm);
    if (max_delay < 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: max_delay %d is negative", max_delay);
    if (npix > (1 << 24) || ndm > 1024) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: %d pixels (at most 2^24) or %d trials (at most 1024)", npix, ndm);
    if (nwidth < 1 || nwidth > IS_MAX_NWIDTH) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: %d boxcar widths, not 1 to %d", nwidth, IS_MAX_NWIDTH);
    if (nstat < 2 || nstat > (1 << 20)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: a baseline block of %d integrations, not 2 to 2^20", nstat);
    if ((1 << (nwidth - 1)) > nstat)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: the widest boxcar, %d integrations, is longer than a baseline block of %d", 1 << (nwidth - 1), nstat);
    const int npitch = (npix + 3) & ~3, T = (1 << (nwidth - 1)) - 1;
    const double bytes = 4.0 * ((double)IS_NSTATE * ngroup * npix + ((double)max_delay + 1) * ngroup * npitch + (double)(T + 1) * ndm * npitch);
    if (bytes > (double)XENG_IMSEARCH_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: %.3g MB of state is above XENG_IMSEARCH_MAX_STATE_BYTES", bytes * 1e-6);
    std::lock_guard<std::mutex> lk(g_ismu);
    imsearch_destroy_locked();
    ImsearchContext& x = g_is;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.npix = npix; x.ngroup = ngroup; x.ndm = ndm; x.max_delay = max_delay; x.nwidth = nwidth; x.nstat = nstat;
    x.npitch = npitch;
    x.T = T;
    x.r_nstat = 1.0f / (float)nstat;
    x.weights.assign((size_t)ngroup, 1.f);
    const size_t ngroupp = (size_t)(ngroup + IS_CHUNK - 1) / IS_CHUNK * IS_CHUNK;
    if (x.alloc.open(x.bytes()) != hipSuccess || hipMalloc(&x.bk, (size_t)ndm * ngroupp * sizeof(int)) != hipSuccess ||
        hipMalloc(&x.gk, ngroupp * sizeof(int)) != hipSuccess || hipMalloc(&x.wk, ngroupp * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        imsearch_free(x);
        x = ImsearchContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Imsearch: cannot allocate %.3g MB of state", bytes * 1e-6);
    }
    x.state = (float*)x.alloc.data();
    x.U = x.state + x.state_words();
    x.Z = x.U + x.u_words();
    x.live = true;
    rc = imsearch_upload_tables(x);
    if (rc) {
        imsearch_destroy_locked();
        return rc;
    }
    return XENG_STATUS_SUCCESS;
}

int xengImsearchSetDelays(const int* delays) {
    if (!delays) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchSetDelays: null table");
    if ((uintptr_t)delays % sizeof(int)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchSetDelays: table %p not aligned to int", (const void*)delays);
    std::lock_guard<std::mutex> lk(g_ismu);
    ImsearchContext& x = g_is;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Imsearch: not initialized (call xengImsearchInitialize)");
    int S = 0;
    for (int d = 0; d < x.ndm; d++)
        for (int g = 0; g < x.ngroup; g++) {
            const int s = delays[(size_t)d * x.ngroup + g];
            if (s < 0 || s > x.max_delay)
                XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchSetDelays: delay %d of trial %d, group %d outside 0..max_delay = %d", s, d, g, x.max_delay);
            if (s > S) S = s;
        }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    x.delays.assign(delays, delays + (size_t)x.ndm * x.ngroup);
    x.S = S;
    x.nint = 0;                                 // (S moves the time axis)
    x.n_w = 0;
    return imsearch_upload_tables(x);
}

int xengImsearchSetWeights(const float* weights) {
    if (!weights) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchSetWeights: null weights");
    if ((uintptr_t)weights % sizeof(float)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchSetWeights: weights %p not aligned to float", (const void*)weights);
    std::lock_guard<std::mutex> lk(g_ismu);
    ImsearchContext& x = g_is;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Imsearch: not initialized (call xengImsearchInitialize)");
    bool any = false;
    for (int g = 0; g < x.ngroup; g++) {
        if (!std::isfinite(weights[g]) || weights[g] < 0.f) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchSetWeights: weight %d is not finite and >= 0", g);
        any = any || weights[g] > 0.f;
    }
    if (!any) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchSetWeights: no weight above 0");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    x.weights.assign(weights, weights + x.ngroup);
    x.n_w = x.nint;                             // (every z before this one was summed with other weights)
    return imsearch_upload_tables(x);
}

int xengImsearchRun(const void* image_dev, void* out_dev) {
    if (!image_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: null %s", image_dev ? "output" : "input");
    if ((uintptr_t)image_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Imsearch: input %p or output %p not 16-byte aligned", image_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_ismu);
    ImsearchContext& x = g_is;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Imsearch: not initialized (call xengImsearchInitialize)");
    if (x.S < 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Imsearch: no delay table (call xengImsearchSetDelays)");
    XENG_HIP(hipSetDevice(x.gpu));
    const long long n = x.nint;
    const unsigned ntile = (unsigned)((x.npitch + IS_TILE - 1) / IS_TILE);
    const long long since = n - x.n_w;
    hipLaunchKernelGGL(imsearch_ingest_kernel, dim3(ntile, (unsigned)x.ngroup), dim3(64), 0, x.stream, (const float*)image_dev, x.state, x.U, x.npix,
                       x.npitch, x.ngroup, x.nstat, x.r_nstat, (int)(n % x.nstat), (int)(n >= x.nstat), (int)(n % (x.S + 1)));
    switch (x.nwidth) {
        case 1: imsearch_search_launch<1>(x, (float2*)out_dev, ntile, n, since); break;
        case 2: imsearch_search_launch<2>(x, (float2*)out_dev, ntile, n, since); break;
        case 3: imsearch_search_launch<3>(x, (float2*)out_dev, ntile, n, since); break;
        case 4: imsearch_search_launch<4>(x, (float2*)out_dev, ntile, n, since); break;
        case 5: imsearch_search_launch<5>(x, (float2*)out_dev, ntile, n, since); break;
        default: imsearch_search_launch<6>(x, (float2*)out_dev, ntile, n, since); break;
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nint = n + 1;
    return XENG_STATUS_SUCCESS;
}

int xengImsearchReset(void) {
    std::lock_guard<std::mutex> lk(g_ismu);
    ImsearchContext& x = g_is;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Imsearch: not initialized");
    x.nint = 0;                         // (what the state and the rings hold lies before integration 0 now: the kernels leave it out)
    x.n_w = 0;
    return XENG_STATUS_SUCCESS;
}

int xengImsearchGetInfo(long long* nintegrations, int* max_delay_in_use) {
    if (!nintegrations || !max_delay_in_use) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_ismu);
    ImsearchContext& x = g_is;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Imsearch: not initialized");
    *nintegrations = x.nint;
    *max_delay_in_use = x.S;
    return XENG_STATUS_SUCCESS;
}

int xengImsearchGetBaseline(float* c, float* m, float* var) {
    if (!c || !m || !var) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ImsearchGetBaseline: null result");
    std::lock_guard<std::mutex> lk(g_ismu);
    ImsearchContext& x = g_is;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Imsearch: not initialized");
    if (x.nint < x.nstat)
        XENG_FAIL(XENG_STATUS_INVALID_STATE, "ImsearchGetBaseline: %lld integrations since the reset, no block of %d is complete", x.nint, x.nstat);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    const size_t plane = (size_t)x.ngroup * x.npix, n = plane * sizeof(float);
    XENG_HIP(hipMemcpy(c, x.state + IS_DC * plane, n, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(m, x.state + IS_DM * plane, n, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(var, x.state + IS_DV * plane, n, hipMemcpyDeviceToHost));
    return XENG_STATUS_SUCCESS;
}

int xengImsearchCheckGuards(int* intact) { return beam_context_check_guards(g_ismu, g_is, g_is.alloc, "Imsearch", intact); }
int xengImsearchMark(unsigned long long* ticket) { return beam_context_mark(g_ismu, g_is, "Imsearch", ticket); }
int xengImsearchWait(unsigned long long ticket) { return beam_context_wait(g_ismu, g_is, "Imsearch", ticket); }
int xengImsearchTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_ismu, g_is, "Imsearch", ticket, done); }
int xengImsearchSync(void) { return beam_context_sync(g_ismu, g_is, "Imsearch"); }

int xengImsearchDestroy(void) {
    std::lock_guard<std::mutex> lk(g_ismu);
    return imsearch_destroy_locked();
}

}  // extern "C"
