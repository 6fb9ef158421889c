// Host side of the template-matched arrival phases (BeamToa; toa_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).  The host keeps the lists of used groups per sub-band and the mask's
// counts, which it forms when the bands and the mask are set; a call is six launches and carries nothing over to the next.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "toa_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct ToaContext : BeamStreamContext {
    int npair = 0, nprod = 0, nchg = 0, nbin = 0, nsub = 0, nharm = 0, nlag = 0;
    bool bands = false, tables = false, templ = false;
    std::vector<int> used;              // [nsub]: used groups per sub-band
    long long ncalls = 0;               // calls since the last reset
    GuardedState alloc;                 // the state between its guard bands (xengToaCheckGuards)
    float* D = nullptr;                 // [nbin][nharm][2]
    float* L = nullptr;                 // [nharm][nlag][2]
    float* S = nullptr;                 // [npair][nsub + 1][nharm][2]
    float* w = nullptr;                 // [nchg]
    int* gl = nullptr;                  // [nchg]: the used groups of the sub-bands, ascending, in the first gs[nsub] words
    int* gs = nullptr;                  // [nsub + 1]: where each sub-band's groups begin in gl
    unsigned char* off = nullptr;       // [npair][nbin]
    unsigned char* active = nullptr;    // [npair]
    int* cnt = nullptr;                 // [npair] = n_off
    float* bv = nullptr;                // [npair][nsub + 1][2] = (base, var)

    static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
    size_t nrow() const { return (size_t)npair * (nsub + 1); }
    size_t D_bytes() const { return up16((size_t)nbin * nharm * 8); }
    size_t L_bytes() const { return up16((size_t)nharm * nlag * 8); }
    size_t S_bytes() const { return up16(nrow() * nharm * 8); }
    size_t chan_bytes() const { return up16((size_t)nchg * 4); }
    size_t gs_bytes() const { return up16((size_t)(nsub + 1) * 4); }
    size_t mask_bytes() const { return up16((size_t)npair * nbin); }
    size_t pair_bytes(size_t word) const { return up16((size_t)npair * word); }
    size_t bv_bytes() const { return up16(nrow() * 8); }
    size_t state_bytes() const {
        return D_bytes() + L_bytes() + S_bytes() + 2 * chan_bytes() + gs_bytes() + mask_bytes() + pair_bytes(1) + pair_bytes(4) + bv_bytes();
    }
    size_t prof_offset() const { return nrow() * sizeof(ToaRecord); }
    size_t harm_offset() const { return prof_offset() + nrow() * nbin * 4; }
    size_t ccf_offset() const { return harm_offset() + nrow() * nharm * 8; }
    size_t out_bytes() const { return ccf_offset() + nrow() * nlag * 4; }
};
static_assert(sizeof(ToaRecord) == 16, "the record of include/xeng.h");
static std::mutex g_toamu;
static ToaContext g_toa;

static int toa_destroy_locked() {
    if (!g_toa.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_toa);
    g_toa.alloc.free();
    g_toa = ToaContext();
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengToaInitialize(int gpu, int npair, int nprod, int nchg, int nbin, int nsub, int nharm, int nlag) {
    if (npair < 1 || npair > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: npair %d outside 1..65535", npair);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: nprod %d is neither 1 nor 4", nprod);
    if (nchg < 1 || nchg > XENG_TOA_MAX_NCHG) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: nchg %d outside 1..%d", nchg, XENG_TOA_MAX_NCHG);
    if (nbin < 1 || nbin > XENG_TOA_MAX_NBIN) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: nbin %d outside 1..%d", nbin, XENG_TOA_MAX_NBIN);
    if (nsub < 1 || nsub > XENG_TOA_MAX_NSUB) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: nsub %d outside 1..%d", nsub, XENG_TOA_MAX_NSUB);
    const int hmax = (nbin - 1) / 2 < XENG_TOA_MAX_NHARM ? (nbin - 1) / 2 : XENG_TOA_MAX_NHARM;
    if (nharm < 1 || nharm > hmax)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: nharm %d outside 1..%d (min(%d, (nbin - 1) / 2) at %d bins)", nharm, hmax, XENG_TOA_MAX_NHARM, nbin);
    if (nlag < 1 || nlag > XENG_TOA_MAX_NLAG) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: nlag %d outside 1..%d", nlag, XENG_TOA_MAX_NLAG);
    const long long tb[3] = {(long long)nbin * nharm * 8, (long long)nharm * nlag * 8, (long long)npair * (nsub + 1) * nharm * 8};
    for (int i = 0; i < 3; i++)
        if (tb[i] > XENG_TOA_MAX_TABLE_BYTES)
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: the %s table needs %.3g GB, the limit is %.3g GB", i == 0 ? "bin" : i == 1 ? "lag" : "template",
                      (double)tb[i] * 1e-9, (double)XENG_TOA_MAX_TABLE_BYTES * 1e-9);
    ToaContext y;
    y.npair = npair; y.nprod = nprod; y.nchg = nchg; y.nbin = nbin; y.nsub = nsub; y.nharm = nharm; y.nlag = nlag;
    if ((unsigned long long)y.out_bytes() >= (1ULL << 32))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: %d pairs x %d rows x (%d bins, %d harmonics, %d lags): an output of 4 GiB or more", npair, nsub + 1, nbin,
                  nharm, nlag);
    y.used.assign((size_t)nsub, -1);
    std::lock_guard<std::mutex> lk(g_toamu);
    toa_destroy_locked();
    ToaContext& x = g_toa;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    y.gpu = x.gpu;
    y.stream = x.stream;
    x = y;
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = ToaContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Toa: cannot allocate %.3g MB of state", (double)y.state_bytes() * 1e-6);
    }
    char* p = (char*)x.alloc.data();    // (every piece starts at a multiple of 16 bytes)
    x.D = (float*)p; p += x.D_bytes();
    x.L = (float*)p; p += x.L_bytes();
    x.S = (float*)p; p += x.S_bytes();
    x.w = (float*)p; p += x.chan_bytes();
    x.gl = (int*)p; p += x.chan_bytes();
    x.gs = (int*)p; p += x.gs_bytes();
    x.off = (unsigned char*)p; p += x.mask_bytes();
    x.active = (unsigned char*)p; p += x.pair_bytes(1);
    x.cnt = (int*)p; p += x.pair_bytes(4);
    x.bv = (float*)p;
    // the defaults: every bin off-pulse, every pair active
    const std::vector<unsigned char> ones((size_t)npair * nbin, 1);
    const std::vector<int> cnt((size_t)npair, nbin);
    if (hipMemcpy(x.off, ones.data(), ones.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x.active, ones.data(), (size_t)npair, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x.cnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = ToaContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Toa: cannot set the default mask");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengToaSetBands(const int* edges, const float* w) {
    if (!edges) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetBands: null edges");
    if ((uintptr_t)edges % sizeof(int) || (uintptr_t)w % sizeof(float))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetBands: edges %p or weights %p not aligned to a word", (const void*)edges, (const void*)w);
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized (call xengToaInitialize)");
    if (edges[0] < 0 || edges[x.nsub] > x.nchg)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetBands: the edges %d..%d leave the %d groups", edges[0], edges[x.nsub], x.nchg);
    for (int r = 0; r < x.nsub; r++)
        if (edges[r] > edges[r + 1]) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetBands: edge %d (%d) is above edge %d (%d)", r, edges[r], r + 1, edges[r + 1]);
    std::vector<float> wv((size_t)x.nchg, 1.f);
    std::vector<int> gl((size_t)x.nchg, 0), gs((size_t)x.nsub + 1, 0), used((size_t)x.nsub, 0);
    if (w)
        for (int g = 0; g < x.nchg; g++) {
            if (!std::isfinite(w[g])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetBands: weight %d is not finite", g);
            wv[g] = w[g];
        }
    int n = 0;
    for (int r = 0; r < x.nsub; r++) {
        gs[r] = n;
        for (int g = edges[r]; g < edges[r + 1]; g++)
            if (wv[g] != 0.f) gl[n++] = g;
        used[r] = n - gs[r];
    }
    gs[x.nsub] = n;
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the lists)
    XENG_HIP(hipMemcpy(x.w, wv.data(), wv.size() * 4, hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.gl, gl.data(), gl.size() * 4, hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.gs, gs.data(), gs.size() * 4, hipMemcpyHostToDevice));
    x.used = used;
    x.bands = true;
    return XENG_STATUS_SUCCESS;
}

// copies n finite floats of a host table into the state
static int toa_set_floats(ToaContext& x, const char* what, float* dst, const float* src, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(src[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: word %zu of the %s table is not finite", i, what);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(dst, src, n * 4, hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengToaSetTables(const float* D, const float* L) {
    if (!D || !L) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetTables: null table");
    if ((uintptr_t)D % sizeof(float) || (uintptr_t)L % sizeof(float))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetTables: table %p or %p not aligned to float", (const void*)D, (const void*)L);
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized (call xengToaInitialize)");
    int rc = toa_set_floats(x, "bin", x.D, D, (size_t)x.nbin * x.nharm * 2);
    if (rc) return rc;
    rc = toa_set_floats(x, "lag", x.L, L, (size_t)x.nharm * x.nlag * 2);
    if (rc) return rc;
    x.tables = true;
    return XENG_STATUS_SUCCESS;
}

int xengToaSetTemplate(const float* S) {
    if (!S) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetTemplate: null template");
    if ((uintptr_t)S % sizeof(float)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaSetTemplate: template %p not aligned to float", (const void*)S);
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized (call xengToaInitialize)");
    const int rc = toa_set_floats(x, "template", x.S, S, x.nrow() * x.nharm * 2);
    if (rc) return rc;
    x.templ = true;
    return XENG_STATUS_SUCCESS;
}

int xengToaSetMask(const unsigned char* off) {
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized (call xengToaInitialize)");
    const size_t n = (size_t)x.npair * x.nbin;
    std::vector<unsigned char> a(n, 1);
    std::vector<int> cnt((size_t)x.npair, 0);
    for (size_t i = 0; i < n; i++) {
        if (off) a[i] = off[i] != 0;
        cnt[i / x.nbin] += a[i];
    }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the mask)
    XENG_HIP(hipMemcpy(x.off, a.data(), n, hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.cnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengToaSetActive(const unsigned char* active) {
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized (call xengToaInitialize)");
    std::vector<unsigned char> a((size_t)x.npair, 1);
    if (active)
        for (int p = 0; p < x.npair; p++) a[p] = active[p] != 0;
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the list)
    XENG_HIP(hipMemcpy(x.active, a.data(), a.size(), hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengToaRun(const void* in_dev, void* out_dev) {
    if (!in_dev || !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: null input or output");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Toa: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized (call xengToaInitialize)");
    if (!x.bands) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: no sub-bands (call xengToaSetBands)");
    if (!x.tables) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: no tables (call xengToaSetTables)");
    if (!x.templ) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: no template (call xengToaSetTemplate)");
    XENG_HIP(hipSetDevice(x.gpu));
    const float* X = (const float*)in_dev;
    char* o = (char*)out_dev;
    ToaRecord* rec = (ToaRecord*)o;
    float* P = (float*)(o + x.prof_offset());
    float* PH = (float*)(o + x.harm_offset());
    float* ccf = (float*)(o + x.ccf_offset());
    const int nrow = (int)x.nrow();
    const unsigned ntile = (unsigned)((nrow + TOA_ROWS - 1) / TOA_ROWS);
    const dim3 gsc((unsigned)((x.nbin + 4 * TOA_THREADS - 1) / (4 * TOA_THREADS)), (unsigned)x.nsub, (unsigned)x.npair);
    if (x.nprod == 4)
        hipLaunchKernelGGL(toa_scrunch_kernel<4>, gsc, dim3(TOA_THREADS), 0, x.stream, X, (const float*)x.w, (const int*)x.gl, (const int*)x.gs,
                           (const unsigned char*)x.active, P, x.nchg, x.nbin, x.nsub);
    else
        hipLaunchKernelGGL(toa_scrunch_kernel<1>, gsc, dim3(TOA_THREADS), 0, x.stream, X, (const float*)x.w, (const int*)x.gl, (const int*)x.gs,
                           (const unsigned char*)x.active, P, x.nchg, x.nbin, x.nsub);
    hipLaunchKernelGGL(toa_band_kernel, dim3((unsigned)((x.nbin + TOA_THREADS - 1) / TOA_THREADS), (unsigned)x.npair), dim3(TOA_THREADS), 0, x.stream,
                       (const unsigned char*)x.active, P, x.nbin, x.nsub);
    hipLaunchKernelGGL(toa_base_kernel, dim3((unsigned)((nrow + 3) / 4)), dim3(TOA_THREADS), TOA_BASE_LDS_BYTES, x.stream, (const float*)P,
                       (const unsigned char*)x.off, (const unsigned char*)x.active, (const int*)x.cnt, x.bv, nrow, x.nbin, x.nsub);
    hipLaunchKernelGGL(toa_dft_kernel, dim3(ntile, (unsigned)((x.nharm + TOA_THREADS - 1) / TOA_THREADS)), dim3(TOA_THREADS), TOA_DFT_LDS_BYTES, x.stream,
                       (const float*)P, (const float*)x.bv, (const float*)x.D, (const unsigned char*)x.active, PH, nrow, x.nbin, x.nsub, x.nharm);
    hipLaunchKernelGGL(toa_corr_kernel, dim3(ntile, (unsigned)((x.nlag + TOA_THREADS - 1) / TOA_THREADS)), dim3(TOA_THREADS), TOA_CORR_LDS_BYTES, x.stream,
                       (const float*)PH, (const float*)x.S, (const float*)x.L, (const unsigned char*)x.active, ccf, nrow, x.nsub, x.nharm, x.nlag);
    hipLaunchKernelGGL(toa_pick_kernel, dim3((unsigned)nrow), dim3(TOA_THREADS), TOA_PICK_LDS_BYTES, x.stream, (const float*)ccf, (const float*)x.bv,
                       (const int*)x.gs, (const unsigned char*)x.active, rec, x.nsub, x.nlag);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.ncalls++;
    return XENG_STATUS_SUCCESS;
}

int xengToaReset(void) {
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized");
    x.ncalls = 0;                       // (nothing is launched or cleared: a call carries nothing over to the next)
    return XENG_STATUS_SUCCESS;
}

int xengToaGetInfo(long long* ncalls_since_reset, int* nused, long long* prof_offset, long long* harm_offset, long long* ccf_offset, long long* out_bytes) {
    if (!ncalls_since_reset || !nused || !prof_offset || !harm_offset || !ccf_offset || !out_bytes) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "ToaGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_toamu);
    ToaContext& x = g_toa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Toa: not initialized");
    *ncalls_since_reset = x.ncalls;
    for (int r = 0; r < x.nsub; r++) nused[r] = x.used[(size_t)r];
    *prof_offset = (long long)x.prof_offset();
    *harm_offset = (long long)x.harm_offset();
    *ccf_offset = (long long)x.ccf_offset();
    *out_bytes = (long long)x.out_bytes();
    return XENG_STATUS_SUCCESS;
}

int xengToaCheckGuards(int* intact) { return beam_context_check_guards(g_toamu, g_toa, g_toa.alloc, "Toa", intact); }
int xengToaMark(unsigned long long* ticket) { return beam_context_mark(g_toamu, g_toa, "Toa", ticket); }
int xengToaWait(unsigned long long ticket) { return beam_context_wait(g_toamu, g_toa, "Toa", ticket); }
int xengToaTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_toamu, g_toa, "Toa", ticket, done); }
int xengToaSync(void) { return beam_context_sync(g_toamu, g_toa, "Toa"); }

int xengToaDestroy(void) {
    std::lock_guard<std::mutex> lk(g_toamu);
    return toa_destroy_locked();
}

}  // extern "C"
