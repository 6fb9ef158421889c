// Host side of the phase folder (BeamFold; fold_kernels.h): a process-global context of its own on the beamformer's stream
// (BeamStreamContext, xeng_common.h).  The oscillators, the window counts and the hits live here, on the host: the device
// holds the profile, a copy of the oscillators, the rotations, the weights and (for a dump) the hits.
#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "fold_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct FoldContext : BeamStreamContext {
    int npair = 0, nfine = 0, nwin = 0, nbin = 0, nprod = 0;
    GuardedState prof_alloc;            // the profile between its guard bands (xengFoldCheckGuards)
    float* prof = nullptr;              // f32[npair][nbin][nfine][nprod], inside prof_alloc
    FoldOsc* osc_dev = nullptr;         // [npair]
    int* rot = nullptr;                 // i32[npair][nfine]
    float* w = nullptr;                 // f32[nfine]
    uint32_t* hits_dev = nullptr;       // u32[npair][nbin], uploaded by a normalising dump
    std::vector<FoldOsc> osc;           // the oscillators in use
    std::vector<uint32_t> hits;         // [npair][nbin] since the last clear
    bool have_phase = false, have_rot = false;
    long long nwindows = 0;             // windows taken since the last reset
    long long n_ref = 0;                // the window at which the oscillators have m = 0
    long long nfolded = 0;              // windows taken since the last clear

    size_t prof_words() const { return (size_t)npair * nbin * nfine * nprod; }
    size_t prof_bytes() const { return prof_words() * sizeof(float); }
};
static std::mutex g_fomu;
static FoldContext g_fo;

static void fold_free(FoldContext& x) {
    x.prof_alloc.free();
    if (x.osc_dev) (void)hipFree(x.osc_dev);
    if (x.rot) (void)hipFree(x.rot);
    if (x.w) (void)hipFree(x.w);
    if (x.hits_dev) (void)hipFree(x.hits_dev);
}

static int fold_destroy_locked() {
    if (!g_fo.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_fo);
    fold_free(g_fo);
    g_fo = FoldContext();
    return XENG_STATUS_SUCCESS;
}

static void fold_clear_launch(const FoldContext& x) {
    const size_t n = x.prof_words();
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(fold_clear_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, x.stream, x.prof, n);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengFoldInitialize(int gpu, int npair, int nfine, int nwin, int nbin, int nprod) {
    if (npair <= 0 || nfine <= 0 || nwin <= 0 || nbin <= 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: bad sizes npair=%d nfine=%d nwin=%d nbin=%d", npair, nfine, nwin, nbin);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: nprod %d not 1 (I) or 4 (XX, YY, Re XY*, Im XY*)", nprod);
    if (nbin > 65536 || npair > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: %d bins (at most 65536) or %d pairs (at most 65535)", nbin, npair);
    const double bytes = (double)npair * nbin * (double)nfine * nprod * sizeof(float);
    if (bytes > (double)XENG_FOLD_MAX_PROFILE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: a profile of %d pairs x %d bins x %d channels x %d is %.3g GB, above the limit of %.3g GB", npair,
                  nbin, nfine, nprod, bytes * 1e-9, (double)XENG_FOLD_MAX_PROFILE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_fomu);
    fold_destroy_locked();
    FoldContext& x = g_fo;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.npair = npair; x.nfine = nfine; x.nwin = nwin; x.nbin = nbin; x.nprod = nprod;
    const std::vector<float> ones((size_t)nfine, 1.f);
    if (x.prof_alloc.open(x.prof_bytes()) != hipSuccess || hipMalloc(&x.osc_dev, (size_t)npair * sizeof(FoldOsc)) != hipSuccess ||
        hipMalloc(&x.rot, (size_t)npair * nfine * sizeof(int)) != hipSuccess || hipMalloc(&x.w, (size_t)nfine * sizeof(float)) != hipSuccess ||
        hipMalloc(&x.hits_dev, (size_t)npair * nbin * sizeof(uint32_t)) != hipSuccess || hip_memset_now(x.osc_dev, 0, (size_t)npair * sizeof(FoldOsc)) != hipSuccess ||
        hip_memset_now(x.rot, 0, (size_t)npair * nfine * sizeof(int)) != hipSuccess || hip_memset_now(x.hits_dev, 0, (size_t)npair * nbin * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(x.w, ones.data(), (size_t)nfine * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        fold_free(x);
        x = FoldContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Fold: cannot allocate %.3g MB of profile", bytes * 1e-6);
    }
    x.prof = (float*)x.prof_alloc.data();
    x.osc.assign((size_t)npair, FoldOsc{0, 0, 0, 0, 0});
    x.hits.assign((size_t)npair * nbin, 0u);
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengFoldSetPhase(const unsigned long long* phi0, const unsigned long long* dphi, const long long* ddphi, const unsigned char* active, long long n_ref) {
    if (!phi0 || !dphi || !ddphi || !active) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldSetPhase: null array");
    if ((uintptr_t)phi0 % 8 || (uintptr_t)dphi % 8 || (uintptr_t)ddphi % 8) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldSetPhase: an array is not aligned to 8 bytes");
    std::lock_guard<std::mutex> lk(g_fomu);
    FoldContext& x = g_fo;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: not initialized (call xengFoldInitialize)");
    if (n_ref < 0 || n_ref > x.nwindows) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldSetPhase: n_ref %lld outside 0..%lld windows taken so far", n_ref, x.nwindows);
    std::vector<FoldOsc> osc((size_t)x.npair);
    for (int p = 0; p < x.npair; p++) osc[p] = FoldOsc{phi0[p], dphi[p], ddphi[p], active[p] ? 1u : 0u, 0u};
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the oscillators)
    XENG_HIP(hipMemcpy(x.osc_dev, osc.data(), osc.size() * sizeof(FoldOsc), hipMemcpyHostToDevice));
    x.osc.swap(osc);
    x.n_ref = n_ref;
    x.have_phase = true;
    return XENG_STATUS_SUCCESS;
}

int xengFoldSetRotations(const int* rot) {
    if ((uintptr_t)rot % sizeof(int)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldSetRotations: table %p not aligned to int", (const void*)rot);
    std::lock_guard<std::mutex> lk(g_fomu);
    FoldContext& x = g_fo;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: not initialized (call xengFoldInitialize)");
    const size_t n = (size_t)x.npair * x.nfine;
    std::vector<int> r(n, 0);
    if (rot)
        for (size_t i = 0; i < n; i++) {
            if (rot[i] < 0 || rot[i] >= x.nbin)
                XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldSetRotations: rotation %d of pair %d, channel %d outside 0..%d", rot[i], (int)(i / x.nfine),
                          (int)(i % x.nfine), x.nbin - 1);
            r[i] = rot[i];
        }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (a dump in flight reads the rotations)
    XENG_HIP(hipMemcpy(x.rot, r.data(), n * sizeof(int), hipMemcpyHostToDevice));
    x.have_rot = true;
    return XENG_STATUS_SUCCESS;
}

int xengFoldSetWeights(const float* weights) {
    if ((uintptr_t)weights % sizeof(float)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldSetWeights: weights %p not aligned to float", (const void*)weights);
    std::lock_guard<std::mutex> lk(g_fomu);
    FoldContext& x = g_fo;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: not initialized (call xengFoldInitialize)");
    std::vector<float> w((size_t)x.nfine, 1.f);
    if (weights)
        for (int q = 0; q < x.nfine; q++) {
            if (!std::isfinite(weights[q])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldSetWeights: weight %d is not finite", q);
            w[q] = weights[q];
        }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (a dump in flight reads the weights)
    XENG_HIP(hipMemcpy(x.w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengFoldRun(const void* in_dev, int nwin_call) {
    if (!in_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: null input");
    if ((uintptr_t)in_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: input %p not 16-byte aligned", in_dev);
    std::lock_guard<std::mutex> lk(g_fomu);
    FoldContext& x = g_fo;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: not initialized (call xengFoldInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    if (!x.have_phase) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: no phase model (call xengFoldSetPhase)");
    const long long m0 = x.nwindows - x.n_ref;
    if (m0 + nwin_call - 1 >= (1LL << 31))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Fold: window %lld after the phase reference is beyond 2^31 - 1 (call xengFoldSetPhase)", m0 + nwin_call - 1);
    XENG_HIP(hipSetDevice(x.gpu));
    const dim3 grid((unsigned)(((size_t)x.nfine * x.nprod + 255) / 256), (unsigned)x.npair);
    if (x.nprod == 1)
        hipLaunchKernelGGL((fold_kernel<1>), grid, dim3(256), 0, x.stream, (const float*)in_dev, x.prof, x.osc_dev, x.npair, x.nfine, x.nbin, (unsigned)m0, nwin_call);
    else
        hipLaunchKernelGGL((fold_kernel<4>), grid, dim3(256), 0, x.stream, (const float*)in_dev, x.prof, x.osc_dev, x.npair, x.nfine, x.nbin, (unsigned)m0, nwin_call);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    for (int p = 0; p < x.npair; p++) {
        if (!x.osc[p].active) continue;
        uint32_t* h = x.hits.data() + (size_t)p * x.nbin;
        for (int i = 0; i < nwin_call; i++) h[fold_bin(x.osc[p], (uint64_t)(m0 + i), (uint32_t)x.nbin)]++;
    }
    x.nwindows += nwin_call;
    x.nfolded += nwin_call;
    return XENG_STATUS_SUCCESS;
}

int xengFoldDump(void* out_dev, unsigned int* hits_host, int nfscr, int normalise, int clear) {
    if (!out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldDump: null output");
    if ((uintptr_t)out_dev % 16 || (uintptr_t)hits_host % sizeof(unsigned int))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldDump: output %p not 16-byte aligned or hits %p not aligned", out_dev, (void*)hits_host);
    std::lock_guard<std::mutex> lk(g_fomu);
    FoldContext& x = g_fo;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: not initialized (call xengFoldInitialize)");
    if (nfscr < 1 || x.nfine % nfscr) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldDump: nfscr %d does not divide %d channels", nfscr, x.nfine);
    if (!x.have_rot) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: no rotations (call xengFoldSetRotations; NULL means none)");
    XENG_HIP(hipSetDevice(x.gpu));
    if (normalise) {
        XENG_HIP(hipStreamSynchronize(x.stream));   // (an earlier dump in flight reads the hits)
        XENG_HIP(hipMemcpy(x.hits_dev, x.hits.data(), x.hits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    const int gpw = nfscr >= FOLD_QC ? 1 : FOLD_QC / nfscr;
    const long long ngroups = x.nfine / nfscr, ngb = (ngroups + gpw - 1) / gpw, nbt = (x.nbin + FOLD_BT - 1) / FOLD_BT;
    if (ngb * nbt > 0x7fffffffLL) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldDump: %lld channel blocks x %lld bin tiles is more than one launch takes", ngb, nbt);
    const dim3 grid((unsigned)(ngb * nbt), (unsigned)x.npair);
    if (x.nprod == 1)
        hipLaunchKernelGGL((fold_dump_kernel<1>), grid, dim3(256), 0, x.stream, x.prof, x.osc_dev, x.rot, x.w, x.hits_dev, (float*)out_dev, x.nfine, x.nbin, nfscr,
                           gpw, normalise ? 1 : 0, clear ? 1 : 0);
    else
        hipLaunchKernelGGL((fold_dump_kernel<4>), grid, dim3(256), 0, x.stream, x.prof, x.osc_dev, x.rot, x.w, x.hits_dev, (float*)out_dev, x.nfine, x.nbin, nfscr,
                           gpw, normalise ? 1 : 0, clear ? 1 : 0);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    if (hits_host) memcpy(hits_host, x.hits.data(), x.hits.size() * sizeof(uint32_t));
    if (clear) {
        std::fill(x.hits.begin(), x.hits.end(), 0u);
        x.nfolded = 0;
    }
    return XENG_STATUS_SUCCESS;
}

int xengFoldReset(void) {
    std::lock_guard<std::mutex> lk(g_fomu);
    FoldContext& x = g_fo;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: not initialized");
    XENG_HIP(hipSetDevice(x.gpu));
    fold_clear_launch(x);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    std::fill(x.hits.begin(), x.hits.end(), 0u);
    x.nwindows = 0;
    x.n_ref = 0;                        // (the oscillators stay: the next window has m = 0)
    x.nfolded = 0;
    return XENG_STATUS_SUCCESS;
}

int xengFoldGetInfo(long long* nwindows_since_reset, long long* nwindows_folded) {
    if (!nwindows_since_reset || !nwindows_folded) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FoldGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_fomu);
    FoldContext& x = g_fo;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Fold: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nwindows_folded = x.nfolded;
    return XENG_STATUS_SUCCESS;
}

int xengFoldCheckGuards(int* intact) { return beam_context_check_guards(g_fomu, g_fo, g_fo.prof_alloc, "Fold", intact); }
int xengFoldMark(unsigned long long* ticket) { return beam_context_mark(g_fomu, g_fo, "Fold", ticket); }
int xengFoldWait(unsigned long long ticket) { return beam_context_wait(g_fomu, g_fo, "Fold", ticket); }
int xengFoldTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_fomu, g_fo, "Fold", ticket, done); }
int xengFoldSync(void) { return beam_context_sync(g_fomu, g_fo, "Fold"); }

int xengFoldDestroy(void) {
    std::lock_guard<std::mutex> lk(g_fomu);
    return fold_destroy_locked();
}

}  // extern "C"
