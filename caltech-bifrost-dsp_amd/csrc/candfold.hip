// Host side of the candidate folder (BeamCandFold; candfold_kernels.h): a process-global context of its own on the beamformer's
// stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "candfold_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct CandfoldContext : BeamStreamContext {
    int npair = 0, ndm = 0, nwin = 0, nprod = 0, ncand_max = 0, nbin = 0, nsub = 0, nsubwin = 0, nwidth = 0, ntrial = 0;
    int nser = 0;                       // npair * ndm
    int W = 0;                          // nsub * nbin, words of a candidate's cube
    long long nt = 0;                   // nsub * nsubwin, windows of a segment
    int izero = -1;                     // the first trial with d1 = d2 = 0
    size_t lds = 0;                     // bytes of dynamic LDS of the refine kernel
    GuardedState alloc;                 // the state between its guard bands (xengCandfoldCheckGuards)
    float* cube[2] = {nullptr, nullptr};        // f32[ncand_max][W], each followed by its hits: one half folds, the other keeps the last segment
    uint32_t* hits[2] = {nullptr, nullptr};     // u32[ncand_max][W]
    CfCand* cand[2] = {nullptr, nullptr};       // [ncand_max]: the set in force and the one that waits for the segment boundary
    int* rot = nullptr;                 // i32[ntrial][nsub]
    int* zrot = nullptr;                // i32[nsub], zeros
    float* gain = nullptr;              // f32[nwidth]
    int cur = 0;                        // the half that folds
    int act = 0;                        // the candidate table in force
    bool have_cands = false, pending = false;
    long long n_ref = 0;                // the window at which the set in force took effect
    long long nwindows = 0;             // windows taken since the last reset
    long long nsegs = 0;                // segments completed since the last reset

    size_t half_words() const { return 2 * (size_t)ncand_max * W; }
    size_t state_bytes() const {
        return 2 * half_words() * 4 + 2 * (size_t)ncand_max * sizeof(CfCand) + ((size_t)ntrial * nsub + nsub + CF_MAX_WIDTH) * 4;
    }
};
static std::mutex g_cfmu;
static CandfoldContext g_cf;

static int candfold_destroy_locked() {
    if (!g_cf.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_cf);
    g_cf.alloc.free();
    g_cf = CandfoldContext();
    return XENG_STATUS_SUCCESS;
}

// the windows [pos, pos + nc) of the segment in progress, the first of them m0 windows after the set's reference
static void candfold_fold(CandfoldContext& x, const float* in, int pos, long long m0, int nc) {
    const size_t lds = 2 * CF_TILE * sizeof(float);
    if (x.nprod == 1)
        hipLaunchKernelGGL((candfold_fold_kernel<1>), dim3((unsigned)x.ncand_max), dim3(CF_THREADS), lds, x.stream, in, x.cube[x.cur], x.hits[x.cur],
                           x.cand[x.act], x.nser, x.nbin, x.W, x.nsubwin, pos, (unsigned)m0, nc);
    else
        hipLaunchKernelGGL((candfold_fold_kernel<4>), dim3((unsigned)x.ncand_max), dim3(CF_THREADS), lds, x.stream, in, x.cube[x.cur], x.hits[x.cur],
                           x.cand[x.act], x.nser, x.nbin, x.W, x.nsubwin, pos, (unsigned)m0, nc);
}

// +0 over the half that folds, one launch
static void candfold_clear(CandfoldContext& x) {
    const size_t n = x.half_words();
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(candfold_clear_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, x.stream, (uint32_t*)x.cube[x.cur], n);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengCandfoldInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int ncand_max, int nbin, int nsub, int nsubwin, int nwidth, int ntrial,
                           const int* d1, const int* d2, const float* g) {
    if (npair <= 0 || ndm <= 0 || nwin <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: bad sizes npair=%d ndm=%d nwin=%d", npair, ndm, nwin);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: nprod %d not 1 (I) or 4 (XX, YY, Re XY*, Im XY*)", nprod);
    if ((long long)npair * ndm > (1LL << 24)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d pairs x %d trials are more than 2^24 series", npair, ndm);
    if (ncand_max < 1 || ncand_max > XENG_CANDFOLD_MAX_CAND)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d candidates, not 1 to %d", ncand_max, XENG_CANDFOLD_MAX_CAND);
    if (nbin < 16 || nbin > 256 || (nbin & (nbin - 1))) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d bins, not a power of two from 16 to 256", nbin);
    if (nsub < 2 || nsub > 64 || nsub * nbin > 8192)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d sub-integrations of %d bins, not 2 to 64 with nsub*nbin <= 8192", nsub, nbin);
    if (nsubwin < 1 || (long long)nsub * nsubwin >= (1LL << 31))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d windows a sub-integration, not 1 or more with nsub*nsubwin < 2^31", nsubwin);
    if ((long long)nwin > (long long)nsub * nsubwin)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d windows a call are more than a segment of %d x %d", nwin, nsub, nsubwin);
    if (nwidth < 1 || nwidth > CF_MAX_WIDTH || (1 << (nwidth - 1)) > nbin / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d boxcar widths, not 1 or more with 2^(nwidth-1) <= nbin/2 = %d", nwidth, nbin / 2);
    if (ntrial < 1 || ntrial > XENG_CANDFOLD_MAX_TRIAL) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d trials, not 1 to %d", ntrial, XENG_CANDFOLD_MAX_TRIAL);
    if (!d1 || !d2 || !g) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: null trial table or gains");
    if ((uintptr_t)d1 % 4 || (uintptr_t)d2 % 4 || (uintptr_t)g % 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: a table is not aligned to 4 bytes");
    for (int t = 0; t < ntrial; t++)
        if (d1[t] < -(1 << 20) || d1[t] > (1 << 20) || d2[t] < -(1 << 20) || d2[t] > (1 << 20))
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: trial %d (%d, %d) outside +-2^20 sixteenths of a bin", t, d1[t], d2[t]);
    for (int iw = 0; iw < nwidth; iw++)
        if (!std::isfinite(g[iw]) || !(g[iw] > 0.f)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: gain %d is not finite and positive", iw);
    CandfoldContext y;
    y.npair = npair; y.ndm = ndm; y.nwin = nwin; y.nprod = nprod; y.ncand_max = ncand_max; y.nbin = nbin; y.nsub = nsub; y.nsubwin = nsubwin;
    y.nwidth = nwidth; y.ntrial = ntrial;
    y.nser = npair * ndm;
    y.W = nsub * nbin;
    y.nt = (long long)nsub * nsubwin;
    y.lds = (2 * (size_t)y.W + CF_REFINE_EXTRA) * sizeof(float);
    if (y.state_bytes() > (size_t)XENG_CANDFOLD_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d candidates of %d x %d words and %d trials need %.3g GB of state, above the limit of %.3g GB", ncand_max,
                  nsub, nbin, ntrial, (double)y.state_bytes() * 1e-9, (double)XENG_CANDFOLD_MAX_STATE_BYTES * 1e-9);
    std::vector<int> rot((size_t)ntrial * nsub);
    for (int t = 0; t < ntrial; t++) {
        if (y.izero < 0 && d1[t] == 0 && d2[t] == 0) y.izero = t;
        for (int s = 0; s < nsub; s++) {
            const long long r = cf_shift(d1[t], d2[t], s, nsub) % nbin;
            rot[(size_t)t * nsub + s] = (int)(r < 0 ? r + nbin : r);
        }
    }
    std::lock_guard<std::mutex> lk(g_cfmu);
    candfold_destroy_locked();
    CandfoldContext& x = g_cf;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    y.gpu = x.gpu;
    y.stream = x.stream;
    x = y;
    int lds = 0;
    bool fits = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, x.gpu) == hipSuccess;
    if (fits && x.lds > (64 << 10))     // (above 64 KiB a kernel has to ask: the device's answer is the check)
        fits = hipFuncSetAttribute((const void*)candfold_refine_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)x.lds) == hipSuccess;
    else if (fits)
        fits = x.lds <= (size_t)lds;
    if (!fits) {
        (void)hipGetLastError();
        x = CandfoldContext();
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: the refinement of %d x %d words needs %zu bytes of LDS, a work-group may take %d", nsub, nbin, y.lds, lds);
    }
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = CandfoldContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Candfold: cannot allocate %.3g MB of state", (double)y.state_bytes() * 1e-6);
    }
    const size_t cw = (size_t)ncand_max * x.W;
    x.cube[0] = (float*)x.alloc.data();
    x.hits[0] = (uint32_t*)(x.cube[0] + cw);
    x.cube[1] = (float*)(x.hits[0] + cw);
    x.hits[1] = (uint32_t*)(x.cube[1] + cw);
    x.cand[0] = (CfCand*)(x.hits[1] + cw);
    x.cand[1] = x.cand[0] + ncand_max;
    x.rot = (int*)(x.cand[1] + ncand_max);
    x.zrot = x.rot + (size_t)ntrial * nsub;     // (zeros, as the whole state is after open)
    x.gain = (float*)(x.zrot + nsub);
    if (hipMemcpy(x.rot, rot.data(), rot.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x.gain, g, (size_t)nwidth * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = CandfoldContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Candfold: cannot upload the trial table");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengCandfoldSetCandidates(int ncand, const int* series, const unsigned long long* phi0, const unsigned long long* dphi, const long long* ddphi,
                              const unsigned char* active) {
    if (!series || !phi0 || !dphi || !ddphi || !active) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CandfoldSetCandidates: null array");
    if ((uintptr_t)series % 4 || (uintptr_t)phi0 % 8 || (uintptr_t)dphi % 8 || (uintptr_t)ddphi % 8)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CandfoldSetCandidates: an array is not aligned to its words");
    std::lock_guard<std::mutex> lk(g_cfmu);
    CandfoldContext& x = g_cf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Candfold: not initialized (call xengCandfoldInitialize)");
    if (ncand < 1 || ncand > x.ncand_max) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CandfoldSetCandidates: %d candidates, not 1 to %d", ncand, x.ncand_max);
    std::vector<CfCand> tab((size_t)x.ncand_max, CfCand{0, 0, 0, 0, 0});
    for (int c = 0; c < ncand; c++) {
        if (series[c] < 0 || series[c] >= x.nser)
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CandfoldSetCandidates: candidate %d names series %d of %d", c, series[c], x.nser);
        tab[c] = CfCand{phi0[c], dphi[c], ddphi[c], (uint32_t)series[c], active[c] ? 1u : 0u};
    }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (nothing in flight reads the table that waits; after this, nothing reads either)
    XENG_HIP(hipMemcpy(x.cand[x.act ^ 1], tab.data(), tab.size() * sizeof(CfCand), hipMemcpyHostToDevice));
    if (x.nwindows % x.nt == 0) {               // the count stands on a boundary: in force at once
        x.act ^= 1;
        x.n_ref = x.nwindows;
        x.pending = false;
    } else {
        x.pending = true;
    }
    x.have_cands = true;
    return XENG_STATUS_SUCCESS;
}

int xengCandfoldRun(const void* in_dev, int nwin_call, void* out_dev, int* completed) {
    if (!in_dev || !completed) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: null %s", in_dev ? "result" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_cfmu);
    CandfoldContext& x = g_cf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Candfold: not initialized (call xengCandfoldInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    if (!x.have_cands) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Candfold: no candidates (call xengCandfoldSetCandidates)");
    const int pos = (int)(x.nwindows % x.nt);
    const int head = (long long)nwin_call < x.nt - pos ? nwin_call : (int)(x.nt - pos);     // windows of the call that go into the segment in progress
    const bool seg_done = pos + (long long)head == x.nt;
    const long long m0 = x.nwindows - x.n_ref;
    const long long mlast = seg_done && x.pending ? m0 + head - 1 : m0 + nwin_call - 1;      // (a set that waits starts again from m = 0)
    if (mlast >= (1LL << 31))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: window %lld after the candidates' reference is beyond 2^31 - 1 (call xengCandfoldSetCandidates)", mlast);
    if (seg_done && !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Candfold: the call completes a segment and has a null output");
    XENG_HIP(hipSetDevice(x.gpu));
    const float* in = (const float*)in_dev;
    candfold_fold(x, in, pos, m0, head);
    if (seg_done) {
        CfRecord* rec = (CfRecord*)out_dev;
        hipLaunchKernelGGL(candfold_refine_kernel, dim3((unsigned)x.ncand_max), dim3(CF_THREADS), x.lds, x.stream, x.cube[x.cur], x.hits[x.cur], x.cand[x.act],
                           x.rot, x.zrot, x.gain, rec, (float*)(rec + x.ncand_max), x.nsub, x.nbin, x.nwidth, x.ntrial, x.izero);
        x.cur ^= 1;                     // (this segment stays for xengCandfoldGetCube; the one before it goes)
        candfold_clear(x);
        if (x.pending) {
            x.act ^= 1;
            x.n_ref = x.nwindows + head;
            x.pending = false;
        }
        if (nwin_call > head) candfold_fold(x, in + (size_t)head * x.nser * x.nprod, 0, x.nwindows + head - x.n_ref, nwin_call - head);
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows += nwin_call;
    if (seg_done) x.nsegs++;
    *completed = seg_done ? 1 : 0;
    return XENG_STATUS_SUCCESS;
}

int xengCandfoldReset(void) {
    std::lock_guard<std::mutex> lk(g_cfmu);
    CandfoldContext& x = g_cf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Candfold: not initialized");
    XENG_HIP(hipSetDevice(x.gpu));
    candfold_clear(x);                  // (the partial segment is dropped)
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    if (x.pending) {                    // (the reset is a segment boundary)
        x.act ^= 1;
        x.pending = false;
    }
    x.n_ref = 0;                        // the next window has m = 0
    x.nwindows = 0;
    x.nsegs = 0;
    return XENG_STATUS_SUCCESS;
}

int xengCandfoldGetInfo(long long* nwindows_since_reset, long long* nsegments_complete) {
    if (!nwindows_since_reset || !nsegments_complete) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CandfoldGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_cfmu);
    CandfoldContext& x = g_cf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Candfold: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nsegments_complete = x.nsegs;
    return XENG_STATUS_SUCCESS;
}

int xengCandfoldGetCube(float* cube_host, unsigned int* hits_host) {
    if (!cube_host || !hits_host) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CandfoldGetCube: null result");
    std::lock_guard<std::mutex> lk(g_cfmu);
    CandfoldContext& x = g_cf;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Candfold: not initialized");
    if (x.nsegs == 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "CandfoldGetCube: no segment is complete since the reset");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    const size_t n = (size_t)x.ncand_max * x.W * 4;
    XENG_HIP(hipMemcpy(cube_host, x.cube[x.cur ^ 1], n, hipMemcpyDeviceToHost));
    XENG_HIP(hipMemcpy(hits_host, x.hits[x.cur ^ 1], n, hipMemcpyDeviceToHost));
    return XENG_STATUS_SUCCESS;
}

int xengCandfoldCheckGuards(int* intact) { return beam_context_check_guards(g_cfmu, g_cf, g_cf.alloc, "Candfold", intact); }
int xengCandfoldMark(unsigned long long* ticket) { return beam_context_mark(g_cfmu, g_cf, "Candfold", ticket); }
int xengCandfoldWait(unsigned long long ticket) { return beam_context_wait(g_cfmu, g_cf, "Candfold", ticket); }
int xengCandfoldTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_cfmu, g_cf, "Candfold", ticket, done); }
int xengCandfoldSync(void) { return beam_context_sync(g_cfmu, g_cf, "Candfold"); }

int xengCandfoldDestroy(void) {
    std::lock_guard<std::mutex> lk(g_cfmu);
    return candfold_destroy_locked();
}

}  // extern "C"
