// Host side of the Faraday rotation-measure synthesis (BeamRmSynth; rmsynth_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).  The host keeps the list of used channels and the masks' counts, which
// it forms when the tables are set; a call is four launches and carries nothing over to the next.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "rmsynth_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct RmsynthContext : BeamStreamContext {
    int npair = 0, nchg = 0, nbin = 0, nphi = 0, feeds = 0;
    int nrun = 0;                       // ceil(nbin / 64)
    int nused = -1;                     // channels with use != 0; -1: no table yet
    long long ncalls = 0;               // calls since the last reset
    GuardedState alloc;                 // the state between its guard bands (xengRmsynthCheckGuards)
    float* T = nullptr;                 // [nchg][nphi][2]
    float* w = nullptr;                 // [nchg]
    unsigned char* use = nullptr;       // [nchg]
    int* gl = nullptr;                  // [nchg]: the used channels, ascending, in the first nused words
    unsigned char* off = nullptr;       // [npair][nbin]
    unsigned char* on = nullptr;        // [npair][nbin]
    unsigned char* active = nullptr;    // [npair]
    int* cnt = nullptr;                 // [npair][2] = (n_on, n_off)
    float* base = nullptr;              // [npair][4][nchg]
    float* part = nullptr;              // [npair][nrun][nphi]
    float* spec = nullptr;              // [npair][nphi]
    int* kbest = nullptr;               // [npair]

    static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
    size_t T_bytes() const { return up16((size_t)nchg * nphi * 8); }
    size_t chan_bytes(size_t word) const { return up16((size_t)nchg * word); }
    size_t mask_bytes() const { return up16((size_t)npair * nbin); }
    size_t pair_bytes(size_t word) const { return up16((size_t)npair * word); }
    size_t base_bytes() const { return up16((size_t)npair * 4 * nchg * 4); }
    size_t part_bytes() const { return up16((size_t)npair * nrun * nphi * 4); }
    size_t spec_bytes() const { return up16((size_t)npair * nphi * 4); }
    size_t state_bytes() const {
        return T_bytes() + chan_bytes(4) + chan_bytes(1) + chan_bytes(4) + 2 * mask_bytes() + pair_bytes(1) + pair_bytes(8) + base_bytes() + part_bytes() +
               spec_bytes() + pair_bytes(4);
    }
    size_t spec_offset() const { return (size_t)npair * sizeof(RmRecord); }
    size_t prof_offset() const { return spec_offset() + (size_t)npair * nphi * 4; }
    size_t out_bytes() const { return prof_offset() + (size_t)npair * 4 * nbin * 4; }
};
static_assert(sizeof(RmRecord) == 16, "the record of include/xeng.h");
static std::mutex g_rmmu;
static RmsynthContext g_rm;

static int rmsynth_destroy_locked() {
    if (!g_rm.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_rm);
    g_rm.alloc.free();
    g_rm = RmsynthContext();
    return XENG_STATUS_SUCCESS;
}

// (n_on, n_off) per pair of masks given as [npair][nbin]
static std::vector<int> rmsynth_counts(const RmsynthContext& x, const std::vector<unsigned char>& off, const std::vector<unsigned char>& on) {
    std::vector<int> cnt((size_t)x.npair * 2, 0);
    for (int p = 0; p < x.npair; p++)
        for (int b = 0; b < x.nbin; b++) {
            cnt[2 * p] += on[(size_t)p * x.nbin + b] != 0;
            cnt[2 * p + 1] += off[(size_t)p * x.nbin + b] != 0;
        }
    return cnt;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengRmsynthInitialize(int gpu, int npair, int nchg, int nbin, int nphi, int feeds) {
    if (npair < 1 || npair > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: npair %d outside 1..65535", npair);
    if (nchg < 1 || nchg > XENG_RMSYNTH_MAX_NCHG) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: nchg %d outside 1..%d", nchg, XENG_RMSYNTH_MAX_NCHG);
    if (nbin < 1 || nbin > XENG_RMSYNTH_MAX_NBIN) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: nbin %d outside 1..%d", nbin, XENG_RMSYNTH_MAX_NBIN);
    if (nphi < 1 || nphi > XENG_RMSYNTH_MAX_NPHI) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: nphi %d outside 1..%d", nphi, XENG_RMSYNTH_MAX_NPHI);
    if (feeds != 0 && feeds != 1) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: feeds %d is neither 0 (linear) nor 1 (circular)", feeds);
    if ((long long)nchg * nphi * 8 > XENG_RMSYNTH_MAX_TABLE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: a table of %d channels x %d depths needs %.3g GB, the limit is %.3g GB", nchg, nphi,
                  (double)nchg * nphi * 8e-9, (double)XENG_RMSYNTH_MAX_TABLE_BYTES * 1e-9);
    RmsynthContext y;
    y.npair = npair; y.nchg = nchg; y.nbin = nbin; y.nphi = nphi; y.feeds = feeds;
    y.nrun = (nbin + RM_TILE - 1) / RM_TILE;
    if ((unsigned long long)y.out_bytes() >= (1ULL << 32) || (unsigned long long)y.part_bytes() >= (1ULL << 32))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: %d pairs x (%d depths, %d bins): an output or the run partials of 4 GiB or more", npair, nphi, nbin);
    std::lock_guard<std::mutex> lk(g_rmmu);
    rmsynth_destroy_locked();
    RmsynthContext& x = g_rm;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    y.gpu = x.gpu;
    y.stream = x.stream;
    x = y;
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = RmsynthContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Rmsynth: cannot allocate %.3g MB of state", (double)y.state_bytes() * 1e-6);
    }
    char* p = (char*)x.alloc.data();    // (every piece starts at a multiple of 16 bytes)
    x.T = (float*)p; p += x.T_bytes();
    x.w = (float*)p; p += x.chan_bytes(4);
    x.use = (unsigned char*)p; p += x.chan_bytes(1);
    x.gl = (int*)p; p += x.chan_bytes(4);
    x.off = (unsigned char*)p; p += x.mask_bytes();
    x.on = (unsigned char*)p; p += x.mask_bytes();
    x.active = (unsigned char*)p; p += x.pair_bytes(1);
    x.cnt = (int*)p; p += x.pair_bytes(8);
    x.base = (float*)p; p += x.base_bytes();
    x.part = (float*)p; p += x.part_bytes();
    x.spec = (float*)p; p += x.spec_bytes();
    x.kbest = (int*)p;
    // the defaults: every bin off-pulse and on-pulse, every pair active
    const std::vector<unsigned char> ones((size_t)npair * nbin, 1);
    const std::vector<int> cnt = rmsynth_counts(x, ones, ones);
    if (hipMemcpy(x.off, ones.data(), ones.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x.on, ones.data(), ones.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x.active, ones.data(), (size_t)npair, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x.cnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = RmsynthContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Rmsynth: cannot set the default masks");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengRmsynthSetTable(const float* T, const float* w, const unsigned char* use) {
    if (!T) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RmsynthSetTable: null table");
    if ((uintptr_t)T % sizeof(float) || (uintptr_t)w % sizeof(float))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RmsynthSetTable: table %p or weights %p not aligned to float", (const void*)T, (const void*)w);
    std::lock_guard<std::mutex> lk(g_rmmu);
    RmsynthContext& x = g_rm;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rmsynth: not initialized (call xengRmsynthInitialize)");
    std::vector<float> wv((size_t)x.nchg, 1.f);
    std::vector<unsigned char> uv((size_t)x.nchg, 1);
    std::vector<int> gl((size_t)x.nchg, 0);
    int nused = 0;
    for (int g = 0; g < x.nchg; g++) {
        if (w) {
            if (!std::isfinite(w[g])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RmsynthSetTable: weight %d is not finite", g);
            wv[g] = w[g];
        }
        if (use) uv[g] = use[g] != 0;
        if (!uv[g]) continue;
        const float* row = T + (size_t)g * x.nphi * 2;
        for (int k = 0; k < 2 * x.nphi; k++)
            if (!std::isfinite(row[k])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RmsynthSetTable: the table of used channel %d, depth %d is not finite", g, k / 2);
        gl[nused++] = g;
    }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(x.T, T, (size_t)x.nchg * x.nphi * 8, hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.w, wv.data(), wv.size() * 4, hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.use, uv.data(), uv.size(), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.gl, gl.data(), gl.size() * 4, hipMemcpyHostToDevice));
    x.nused = nused;
    return XENG_STATUS_SUCCESS;
}

int xengRmsynthSetMasks(const unsigned char* off, const unsigned char* on) {
    std::lock_guard<std::mutex> lk(g_rmmu);
    RmsynthContext& x = g_rm;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rmsynth: not initialized (call xengRmsynthInitialize)");
    const size_t n = (size_t)x.npair * x.nbin;
    std::vector<unsigned char> a(n, 1), b(n, 1);
    for (size_t i = 0; i < n; i++) {
        if (off) a[i] = off[i] != 0;
        if (on) b[i] = on[i] != 0;
    }
    const std::vector<int> cnt = rmsynth_counts(x, a, b);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the masks)
    XENG_HIP(hipMemcpy(x.off, a.data(), n, hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.on, b.data(), n, hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.cnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengRmsynthSetActive(const unsigned char* active) {
    std::lock_guard<std::mutex> lk(g_rmmu);
    RmsynthContext& x = g_rm;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rmsynth: not initialized (call xengRmsynthInitialize)");
    std::vector<unsigned char> a((size_t)x.npair, 1);
    if (active)
        for (int p = 0; p < x.npair; p++) a[p] = active[p] != 0;
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the list)
    XENG_HIP(hipMemcpy(x.active, a.data(), a.size(), hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengRmsynthRun(const void* in_dev, void* out_dev) {
    if (!in_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: null input or output");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Rmsynth: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_rmmu);
    RmsynthContext& x = g_rm;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rmsynth: not initialized (call xengRmsynthInitialize)");
    if (x.nused < 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rmsynth: no table (call xengRmsynthSetTable)");
    XENG_HIP(hipSetDevice(x.gpu));
    const float* X = (const float*)in_dev;
    char* o = (char*)out_dev;
    const unsigned ntile_k = (unsigned)((x.nphi + RM_TILE - 1) / RM_TILE);
    hipLaunchKernelGGL(rmsynth_base_kernel, dim3((unsigned)(((long long)x.npair * x.nchg + 3) / 4)), dim3(RM_THREADS), RM_BASE_LDS_BYTES, x.stream, X,
                       (const unsigned char*)x.off, (const unsigned char*)x.use, (const unsigned char*)x.active, (const int*)x.cnt, x.base, x.npair, x.nchg, x.nbin,
                       x.feeds);
    hipLaunchKernelGGL(rmsynth_contract_kernel, dim3(ntile_k, (unsigned)x.nrun, (unsigned)x.npair), dim3(RM_THREADS), RM_CONTRACT_LDS_BYTES, x.stream, X,
                       (const float*)x.T, (const int*)x.gl, (const float*)x.base, (const unsigned char*)x.on, (const unsigned char*)x.active, x.part, x.nused, x.nchg,
                       x.nbin, x.nphi, x.feeds);
    hipLaunchKernelGGL(rmsynth_pick_kernel, dim3((unsigned)x.npair), dim3(RM_THREADS), RM_PICK_LDS_BYTES, x.stream, (const float*)x.part,
                       (const unsigned char*)x.active, (const int*)x.cnt, x.spec, x.kbest, (RmRecord*)o, (float*)(o + x.spec_offset()), x.nrun, x.nphi);
    hipLaunchKernelGGL(rmsynth_profile_kernel, dim3((unsigned)((x.nbin + RM_THREADS - 1) / RM_THREADS), (unsigned)x.npair), dim3(RM_THREADS), 0, x.stream, X,
                       (const float*)x.T, (const float*)x.w, (const int*)x.gl, (const float*)x.base, (const unsigned char*)x.active, (const int*)x.kbest,
                       (float*)(o + x.prof_offset()), x.nused, x.nchg, x.nbin, x.nphi, x.feeds);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.ncalls++;
    return XENG_STATUS_SUCCESS;
}

int xengRmsynthReset(void) {
    std::lock_guard<std::mutex> lk(g_rmmu);
    RmsynthContext& x = g_rm;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rmsynth: not initialized");
    x.ncalls = 0;                       // (nothing is launched or cleared: a call carries nothing over to the next)
    return XENG_STATUS_SUCCESS;
}

int xengRmsynthGetInfo(long long* ncalls_since_reset, int* nused, long long* spec_offset, long long* prof_offset, long long* out_bytes) {
    if (!ncalls_since_reset || !nused || !spec_offset || !prof_offset || !out_bytes) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "RmsynthGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_rmmu);
    RmsynthContext& x = g_rm;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Rmsynth: not initialized");
    *ncalls_since_reset = x.ncalls;
    *nused = x.nused;
    *spec_offset = (long long)x.spec_offset();
    *prof_offset = (long long)x.prof_offset();
    *out_bytes = (long long)x.out_bytes();
    return XENG_STATUS_SUCCESS;
}

int xengRmsynthCheckGuards(int* intact) { return beam_context_check_guards(g_rmmu, g_rm, g_rm.alloc, "Rmsynth", intact); }
int xengRmsynthMark(unsigned long long* ticket) { return beam_context_mark(g_rmmu, g_rm, "Rmsynth", ticket); }
int xengRmsynthWait(unsigned long long ticket) { return beam_context_wait(g_rmmu, g_rm, "Rmsynth", ticket); }
int xengRmsynthTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_rmmu, g_rm, "Rmsynth", ticket, done); }
int xengRmsynthSync(void) { return beam_context_sync(g_rmmu, g_rm, "Rmsynth"); }

int xengRmsynthDestroy(void) {
    std::lock_guard<std::mutex> lk(g_rmmu);
    return rmsynth_destroy_locked();
}

}  // extern "C"
