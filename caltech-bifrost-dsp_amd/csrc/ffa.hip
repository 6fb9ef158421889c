// Host side of the fast-folding search (BeamFfaSearch; ffa_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "ffa_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct FfaContext : BeamStreamContext {
    int npair = 0, ndm = 0, nwin = 0, nprod = 0, nds = 0, nt = 0, noct = 0, pmin = 0, pmax = 0, nwidth = 0;
    int nser = 0;                       // npair * ndm
    int np = 0;                         // pmax - pmin + 1
    int xw = 0;                         // words of a series in xbuf: N_0 + ... + N_{noct-1}
    size_t lds[FA_MAX_OCT] = {};        // bytes of dynamic LDS of the fold kernel, per octave
    FfaRinv rinv;
    GuardedState alloc;                 // the state between its guard bands (xengFfaCheckGuards)
    FfaRecord* table = nullptr;         // [nser][noct][np][nwidth], inside alloc
    float* tbuf = nullptr;              // f32[nser][nt], behind it
    float* xbuf = nullptr;              // f32[nser][xw]
    float* stats = nullptr;             // f32[nser][noct][4]
    float* part = nullptr;              // f32[2][nser]
    float* rho = nullptr;               // f32[FA_MAX_WIDTH][FA_RHO_STRIDE]
    int par = 0;                        // the half of part the next ingest reads
    long long nwindows = 0;             // windows taken since the last reset
    long long nsegs = 0;                // segments completed since the last reset

    size_t state_bytes() const {
        return (size_t)nser * noct * np * nwidth * sizeof(FfaRecord) +
               ((size_t)nser * nt + (size_t)nser * xw + (size_t)nser * noct * 4 + 2 * (size_t)nser + FA_MAX_WIDTH * FA_RHO_STRIDE) * sizeof(float);
    }
};
static std::mutex g_famu;
static FfaContext g_fa;

static int ffa_destroy_locked() {
    if (!g_fa.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_fa);
    g_fa.alloc.free();
    g_fa = FfaContext();
    return XENG_STATUS_SUCCESS;
}

// the largest M * p over the base periods at a segment of n samples, M the largest power of two with M * p <= n
static int ffa_max_words(int n, int pmin, int pmax) {
    int best = 0;
    for (int p = pmin; p <= pmax; p++) {
        int w = p;
        while (2 * w <= n) w *= 2;
        if (w > best) best = w;
    }
    return best;
}

// the windows [pos, pos + nc) of the segment in progress
static void ffa_ingest(FfaContext& x, const float* in, int pos, int nc) {
    const int nk = (pos + nc - 1) / x.nds - pos / x.nds + 1;
    const dim3 g((unsigned)((x.nser + FA_TILE - 1) / FA_TILE), (unsigned)((nk + FA_TILE - 1) / FA_TILE));
    const float* pin = x.part + (size_t)x.par * x.nser;
    float* pout = x.part + (size_t)(x.par ^ 1) * x.nser;
    if (x.nprod == 1)
        hipLaunchKernelGGL((ffa_ingest_kernel<1>), g, dim3(256), 0, x.stream, in, x.tbuf, pin, pout, x.nser, x.nt, x.nds, pos, nc);
    else
        hipLaunchKernelGGL((ffa_ingest_kernel<4>), g, dim3(256), 0, x.stream, in, x.tbuf, pin, pout, x.nser, x.nt, x.nds, pos, nc);
    x.par ^= 1;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengFfaInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nds, int nt, int noct, int pmin, int pmax, int nwidth) {
    if (npair <= 0 || ndm <= 0 || nwin <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: bad sizes npair=%d ndm=%d nwin=%d", npair, ndm, nwin);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: nprod %d not 1 (I) or 4 (XX, YY, Re XY*, Im XY*)", nprod);
    if (nds < 1 || nds > XENG_FFA_MAX_NDS) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: %d windows a sample, not 1 to %d", nds, XENG_FFA_MAX_NDS);
    if (noct < 1 || noct > FA_MAX_OCT) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: %d octaves, not 1 to %d", noct, FA_MAX_OCT);
    if (nt < (1 << 8) || nt > (1 << 14) || nt % (1 << (noct - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: a segment of %d samples, not a multiple of 2^(noct-1) = %d from 2^8 to 2^14", nt, 1 << (noct - 1));
    if (pmin < 16 || pmax < pmin || 2 * (long long)pmax > (nt >> (noct - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: base periods %d..%d, not 16 <= pmin <= pmax <= %d, half the top octave's segment", pmin, pmax,
                  (nt >> (noct - 1)) / 2);
    if (nwidth < 1 || nwidth > FA_MAX_WIDTH || (1 << (nwidth - 1)) > pmin / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: %d boxcar widths, not 1 to %d with 2^(nwidth-1) <= pmin/2 = %d", nwidth, FA_MAX_WIDTH, pmin / 2);
    if ((long long)nwin > (long long)nt * nds)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: %d windows a call are more than a segment of %d x %d", nwin, nt, nds);
    if ((long long)npair * ndm > (1LL << 24))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: %d pairs x %d trials is more than one launch takes", npair, ndm);
    FfaContext y;
    y.npair = npair; y.ndm = ndm; y.nwin = nwin; y.nprod = nprod; y.nds = nds; y.nt = nt; y.noct = noct; y.pmin = pmin; y.pmax = pmax; y.nwidth = nwidth;
    y.np = pmax - pmin + 1;
    for (int o = 0; o < noct; o++) y.xw += nt >> o;
    const double need = (double)npair * ndm * ((double)noct * y.np * nwidth * 16.0 + 4.0 * (nt + y.xw + 4 * noct + 2)) + 512.0;
    if (need > (double)XENG_FFA_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: %d series of %d samples, %d octaves, %d periods and %d widths need %.3g GB of state, above the limit of %.3g GB",
                  npair * ndm, nt, noct, y.np, nwidth, need * 1e-9, (double)XENG_FFA_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_famu);
    ffa_destroy_locked();
    FfaContext& x = g_fa;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    y.gpu = x.gpu;
    y.stream = x.stream;
    x = y;
    x.nser = npair * ndm;
    size_t ldsmax = 0;
    for (int o = 0; o < noct; o++) {
        x.lds[o] = 2 * sizeof(float) * (size_t)ffa_max_words(nt >> o, pmin, pmax);
        if (x.lds[o] > ldsmax) ldsmax = x.lds[o];
        x.rinv.r[o] = (float)(1.0 / (double)(nt >> o));
    }
    int lds = 0;
    bool fits = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, x.gpu) == hipSuccess;
    if (fits && ldsmax > (64 << 10))    // (above 64 KiB a kernel has to ask: the device's answer is the check)
        fits = hipFuncSetAttribute((const void*)ffa_fold_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsmax) == hipSuccess;
    else if (fits)
        fits = ldsmax + 256 <= (size_t)lds;
    if (!fits) {
        (void)hipGetLastError();
        x = FfaContext();
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: the folds of a segment of %d samples need %zu bytes of LDS, a work-group may take %d", nt, ldsmax, lds);
    }
    std::vector<float> rho((size_t)FA_MAX_WIDTH * FA_RHO_STRIDE, 0.f);
    for (int iw = 0; iw < FA_MAX_WIDTH; iw++)
        for (int lm = 0; lm < FA_RHO_STRIDE; lm++) rho[(size_t)iw * FA_RHO_STRIDE + lm] = (float)(1.0 / std::sqrt((double)(1 << iw) * (double)(1 << lm)));
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = FfaContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Ffa: cannot allocate %.3g MB of state", need * 1e-6);
    }
    x.table = (FfaRecord*)x.alloc.data();
    x.tbuf = (float*)(x.table + (size_t)x.nser * noct * x.np * nwidth);
    x.xbuf = x.tbuf + (size_t)x.nser * nt;
    x.stats = x.xbuf + (size_t)x.nser * x.xw;
    x.part = x.stats + (size_t)x.nser * noct * 4;
    x.rho = x.part + 2 * (size_t)x.nser;
    if (hipMemcpy(x.rho, rho.data(), rho.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = FfaContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Ffa: cannot upload the score table");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengFfaRun(const void* in_dev, int nwin_call, void* out_dev, int* completed) {
    if (!in_dev || !completed) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: null %s", in_dev ? "result" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_famu);
    FfaContext& x = g_fa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Ffa: not initialized (call xengFfaInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    const int seg = x.nt * x.nds;                                       // windows of a segment
    const int pos = (int)(x.nwindows % seg);
    const int head = nwin_call < seg - pos ? nwin_call : seg - pos;     // windows of the call that go into the segment in progress
    const bool seg_done = pos + head == seg;
    if (seg_done && !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Ffa: the call completes a segment and has a null output");
    XENG_HIP(hipSetDevice(x.gpu));
    const float* in = (const float*)in_dev;
    ffa_ingest(x, in, pos, head);
    if (seg_done) {
        hipLaunchKernelGGL(ffa_prepare_kernel, dim3((unsigned)x.nser), dim3(FA_THREADS), 0, x.stream, x.tbuf, x.xbuf, x.stats, x.rinv, x.nt, x.noct);
        for (int o = 0; o < x.noct; o++)
            hipLaunchKernelGGL(ffa_fold_kernel, dim3((unsigned)x.nser, (unsigned)x.np), dim3(FA_THREADS), x.lds[o], x.stream, x.xbuf, x.stats, x.rho, x.table,
                               x.nt, x.noct, o, x.pmin, x.np, x.nwidth);
        const long long nrec = (long long)x.nser * x.noct * x.nwidth;
        hipLaunchKernelGGL(ffa_reduce_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, x.stream, x.table, (FfaRecord*)out_dev, nrec, x.np,
                           x.nwidth);
        if (nwin_call > head) ffa_ingest(x, in + (size_t)head * x.nser * x.nprod, 0, nwin_call - head);
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows += nwin_call;
    if (seg_done) x.nsegs++;
    *completed = seg_done ? 1 : 0;
    return XENG_STATUS_SUCCESS;
}

int xengFfaReset(void) {
    std::lock_guard<std::mutex> lk(g_famu);
    FfaContext& x = g_fa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Ffa: not initialized");
    x.nwindows = 0;                     // (the partial segment and the partial sample are dropped by index: the next window opens
    x.nsegs = 0;                        //  sample 0 of a new segment, which reads no carried sum)
    return XENG_STATUS_SUCCESS;
}

int xengFfaGetInfo(long long* nwindows_since_reset, long long* nsegments_complete) {
    if (!nwindows_since_reset || !nsegments_complete) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FfaGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_famu);
    FfaContext& x = g_fa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Ffa: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nsegments_complete = x.nsegs;
    return XENG_STATUS_SUCCESS;
}

int xengFfaGetStats(float* stats_host) {
    if (!stats_host) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "FfaGetStats: null result");
    std::lock_guard<std::mutex> lk(g_famu);
    FfaContext& x = g_fa;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Ffa: not initialized");
    if (x.nsegs == 0) XENG_FAIL(XENG_STATUS_INVALID_STATE, "FfaGetStats: no segment is complete since the reset");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    XENG_HIP(hipMemcpy(stats_host, x.stats, (size_t)x.nser * x.noct * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return XENG_STATUS_SUCCESS;
}

int xengFfaCheckGuards(int* intact) { return beam_context_check_guards(g_famu, g_fa, g_fa.alloc, "Ffa", intact); }
int xengFfaMark(unsigned long long* ticket) { return beam_context_mark(g_famu, g_fa, "Ffa", ticket); }
int xengFfaWait(unsigned long long ticket) { return beam_context_wait(g_famu, g_fa, "Ffa", ticket); }
int xengFfaTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_famu, g_fa, "Ffa", ticket, done); }
int xengFfaSync(void) { return beam_context_sync(g_famu, g_fa, "Ffa"); }

int xengFfaDestroy(void) {
    std::lock_guard<std::mutex> lk(g_famu);
    return ffa_destroy_locked();
}

}  // extern "C"
