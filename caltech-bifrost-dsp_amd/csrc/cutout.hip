// Host side of the single-pulse cut-outs (BeamPulseCutout; cutout_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).  The host keeps the window count, the pending requests and the per-trial
// largest delays, and decides what a call serves before anything is enqueued.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "cutout_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct CutoutPending {
    xengCutoutReq q;
    long long first, last;              // the windows the request needs
};

struct CutoutContext : BeamStreamContext {
    int npair = 0, nfine = 0, nwin = 0, ndmf = 0, nhist = 0, nband = 0, nt = 0, tscr = 0, tshift = 0, ndmc = 0, nwidth = 0, nreq_max = 0;
    int ntu = 0;                        // nt * tscr
    int L = 0;                          // nhist + nwin, slots of the ring per (pair, channel)
    float k_mad = 0.f;
    CutoutRho rho = {};
    GuardedState alloc;                 // the state between its guard bands (xengCutoutCheckGuards)
    float* ring = nullptr;              // [npair][nfine][L]
    int* s = nullptr;                   // [ndmf][nfine]
    float* w = nullptr;                 // [nfine]
    CutoutRow* rowrec = nullptr;        // [nreq_max][ndmc]
    std::vector<int> smax;              // [ndmf]: the largest delay of every trial; empty: no table yet
    std::vector<CutoutPending> pending;
    long long nwindows = 0;             // windows taken since the last reset

    static size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
    size_t ring_bytes() const { return up16((size_t)npair * nfine * L * 4); }
    size_t s_bytes() const { return up16((size_t)ndmf * nfine * 4); }
    size_t w_bytes() const { return up16((size_t)nfine * 4); }
    size_t state_bytes() const { return ring_bytes() + s_bytes() + w_bytes() + up16((size_t)nreq_max * ndmc * sizeof(CutoutRow)); }
    size_t rec_bytes() const { return (size_t)nreq_max * sizeof(CutoutRecord); }
    size_t out_bytes() const { return rec_bytes() + (size_t)nreq_max * 4 * nt * ((size_t)nband + ndmc); }
};
static_assert(sizeof(CutoutRecord) == 32 && sizeof(CutoutRow) == 16 && sizeof(xengCutoutReq) == 24, "the records of include/xeng.h");
static std::mutex g_comu;
static CutoutContext g_co;

static int cutout_destroy_locked() {
    if (!g_co.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_co);
    g_co.alloc.free();
    g_co = CutoutContext();
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengCutoutInitialize(int gpu, int npair, int nfine, int nwin, int ndmf, int nhist, int nband, int nt, int tscr, int ndmc, int nwidth, int nreq_max,
                         float k_mad) {
    if (npair < 1 || npair > 65535 || nfine < 1 || nwin < 1 || ndmf < 1 || (long long)ndmf * nfine > (1LL << 28))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: bad sizes npair=%d nfine=%d nwin=%d ndmf=%d", npair, nfine, nwin, ndmf);
    if (nband < 1 || nband > 256 || nfine % nband) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: %d bands, not a divisor of nfine = %d in 1..256", nband, nfine);
    if (tscr < 1 || tscr > 64 || (tscr & (tscr - 1))) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: tscr %d, not a power of two in 1..64", tscr);
    if (nt < 16 || nt > 1024 || (nt & 1)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: nt %d, not an even number in 16..1024", nt);
    if (ndmc < 1 || ndmc > 256) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: ndmc %d outside 1..256", ndmc);
    if (nwidth < 1 || nwidth > CO_MAX_WIDTH || (1 << (nwidth - 1)) > nt / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: nwidth %d: the widest boxcar, 2^(nwidth-1), must not exceed nt/2 = %d", nwidth, nt / 2);
    if (nreq_max < 1 || nreq_max > CO_MAX_REQ) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: nreq_max %d outside 1..%d", nreq_max, CO_MAX_REQ);
    if (!std::isfinite(k_mad) || !(k_mad > 0.f)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: k_mad %g is not finite and positive", k_mad);
    if (nhist < nt * tscr) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: a history of %d windows is shorter than a cut-out of %d", nhist, nt * tscr);
    const unsigned long long hist = ((unsigned long long)nhist + nwin) * npair * nfine * 4;
    if (hist >= (unsigned long long)XENG_CUTOUT_MAX_HISTORY_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: a history of %d + %d windows x %d pairs x %d channels needs %.3g GB, the limit is %.3g GB", nhist, nwin,
                  npair, nfine, (double)hist * 1e-9, (double)XENG_CUTOUT_MAX_HISTORY_BYTES * 1e-9);
    CutoutContext y;
    y.npair = npair; y.nfine = nfine; y.nwin = nwin; y.ndmf = ndmf; y.nhist = nhist; y.nband = nband; y.nt = nt; y.tscr = tscr; y.ndmc = ndmc;
    y.nwidth = nwidth; y.nreq_max = nreq_max;
    while ((1 << y.tshift) < tscr) y.tshift++;
    y.ntu = nt * tscr;
    y.L = nhist + nwin;
    y.k_mad = k_mad;
    for (int iw = 0; iw < nwidth; iw++) y.rho.rho[iw] = (float)std::pow(2.0, -0.5 * iw);
    std::lock_guard<std::mutex> lk(g_comu);
    cutout_destroy_locked();
    CutoutContext& x = g_co;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    y.gpu = x.gpu;
    y.stream = x.stream;
    x = y;
    const std::vector<float> ones((size_t)nfine, 1.f);
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = CutoutContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Cutout: cannot allocate %.3g MB of state", (double)y.state_bytes() * 1e-6);
    }
    char* p = (char*)x.alloc.data();    // (every piece starts at a multiple of 16 bytes)
    x.ring = (float*)p; p += x.ring_bytes();
    x.s = (int*)p; p += x.s_bytes();
    x.w = (float*)p; p += x.w_bytes();
    x.rowrec = (CutoutRow*)p;
    if (hipMemcpy(x.w, ones.data(), (size_t)nfine * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = CutoutContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Cutout: cannot set the weights");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengCutoutSetDelays(const int* delays) {
    if (!delays) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutSetDelays: null table");
    if ((uintptr_t)delays % sizeof(int)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutSetDelays: table %p not aligned to int", (const void*)delays);
    std::lock_guard<std::mutex> lk(g_comu);
    CutoutContext& x = g_co;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: not initialized (call xengCutoutInitialize)");
    std::vector<int> smax((size_t)x.ndmf, 0);
    for (int d = 0; d < x.ndmf; d++)
        for (int q = 0; q < x.nfine; q++) {
            const int s = delays[(size_t)d * x.nfine + q];
            if (s < 0 || s > x.nhist - x.ntu)
                XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutSetDelays: delay %d of trial %d, channel %d outside 0..nhist - ntu = %d", s, d, q, x.nhist - x.ntu);
            if (s > smax[d]) smax[d] = s;
        }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the table)
    XENG_HIP(hipMemcpy(x.s, delays, (size_t)x.ndmf * x.nfine * 4, hipMemcpyHostToDevice));
    x.smax = smax;
    x.pending.clear();
    x.nwindows = 0;
    return XENG_STATUS_SUCCESS;
}

int xengCutoutSetWeights(const float* weights) {
    if ((uintptr_t)weights % sizeof(float)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutSetWeights: weights %p not aligned to float", (const void*)weights);
    std::lock_guard<std::mutex> lk(g_comu);
    CutoutContext& x = g_co;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: not initialized (call xengCutoutInitialize)");
    std::vector<float> w((size_t)x.nfine, 1.f);
    if (weights)
        for (int q = 0; q < x.nfine; q++) {
            if (!std::isfinite(weights[q])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutSetWeights: weight %d is not finite", q);
            w[q] = weights[q];
        }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the weights)
    XENG_HIP(hipMemcpy(x.w, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    return XENG_STATUS_SUCCESS;
}

int xengCutoutRequest(int nreq, const xengCutoutReq* reqs) {
    if (nreq < 0 || (nreq > 0 && !reqs)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutRequest: %d requests at %p", nreq, (const void*)reqs);
    if ((uintptr_t)reqs % 8) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutRequest: requests %p not aligned to 8 bytes", (const void*)reqs);
    std::lock_guard<std::mutex> lk(g_comu);
    CutoutContext& x = g_co;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: not initialized (call xengCutoutInitialize)");
    if (x.smax.empty()) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: no delay table (call xengCutoutSetDelays)");
    if ((long long)x.pending.size() + nreq > XENG_CUTOUT_MAX_PENDING)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutRequest: %zu waiting and %d more is above %d", x.pending.size(), nreq, XENG_CUTOUT_MAX_PENDING);
    std::vector<CutoutPending> add;
    const int c = x.ndmc / 2;
    for (int k = 0; k < nreq; k++) {
        const xengCutoutReq& q = reqs[k];
        if (q.pair < 0 || q.pair >= x.npair) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutRequest: request %d: pair %d outside 0..%d", k, q.pair, x.npair - 1);
        if (q.ic < 0 || q.ic >= x.ndmf) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutRequest: request %d: centre trial %d outside 0..%d", k, q.ic, x.ndmf - 1);
        if (q.n_c < 0 || q.n_c >= (1LL << 62)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutRequest: request %d: window %lld outside 0..2^62", k, q.n_c);
        if (q.dstep < 1 || q.dstep > (1 << 20)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutRequest: request %d: dstep %d outside 1..2^20", k, q.dstep);
        int S = 0;
        for (int i = 0; i < x.ndmc; i++) {
            const long long d = (long long)q.ic + (long long)(i - c) * q.dstep;
            if (d >= 0 && d < x.ndmf && x.smax[(size_t)d] > S) S = x.smax[(size_t)d];
        }
        CutoutPending pe;
        pe.q = q;
        pe.first = q.n_c - x.ntu / 2;
        pe.last = pe.first + x.ntu - 1 + S;
        add.push_back(pe);
    }
    x.pending.insert(x.pending.end(), add.begin(), add.end());
    return XENG_STATUS_SUCCESS;
}

int xengCutoutRun(const void* in_dev, int nwin_call, void* out_dev, int* nserved, int* served_ids, int* nexpired, int* expired_ids) {
    if (!in_dev || !nserved || !served_ids || !nexpired || !expired_ids) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: null input or result");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_comu);
    CutoutContext& x = g_co;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: not initialized (call xengCutoutInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    if (x.smax.empty()) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: no delay table (call xengCutoutSetDelays)");
    // what the call serves, from the host's counts alone
    const long long n0 = x.nwindows, n = n0 + nwin_call;
    CutoutSlots sl = {};
    std::vector<CutoutPending> keep;
    std::vector<int> expired;
    int r = 0;
    for (const CutoutPending& pe : x.pending) {
        if (pe.first < n - x.nhist) {
            expired.push_back(pe.q.id);
        } else if (pe.last < n && r < x.nreq_max) {
            sl.id[r] = pe.q.id;
            sl.pair[r] = pe.q.pair;
            sl.ic[r] = pe.q.ic;
            sl.dstep[r] = pe.q.dstep;
            sl.slot0[r] = (int)(((pe.first % x.L) + x.L) % x.L);
            sl.a0[r] = pe.first < (1LL << 30) ? (int)pe.first : (1 << 30);
            r++;
        } else {
            keep.push_back(pe);
        }
    }
    if (r && !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cutout: null output on a call that serves %d requests", r);
    XENG_HIP(hipSetDevice(x.gpu));
    const dim3 gi((unsigned)((x.nfine + DD_TILE - 1) / DD_TILE), (unsigned)x.npair, (unsigned)((nwin_call + DD_TILE - 1) / DD_TILE));
    hipLaunchKernelGGL(dedisp_ingest_kernel<1>, gi, dim3(256), 0, x.stream, (const float4*)in_dev, x.ring, x.npair, x.nfine, x.L, (int)(n0 % x.L), nwin_call);
    if (r) {
        char* o = (char*)out_dev;
        float* W = (float*)(o + x.rec_bytes());
        float* P = W + (size_t)x.nreq_max * x.nband * x.nt;
        hipLaunchKernelGGL(cutout_partials_kernel, dim3((unsigned)((x.ntu + CO_THREADS - 1) / CO_THREADS), (unsigned)x.ndmc, (unsigned)r), dim3(CO_THREADS),
                           CO_PARTIALS_LDS_BYTES, x.stream, (const float*)x.ring, (const int*)x.s, (const float*)x.w, sl, W, P, x.nfine, x.L, x.ndmf, x.nband, x.nt,
                           x.tshift, x.ndmc);
        hipLaunchKernelGGL(cutout_score_kernel, dim3((unsigned)x.ndmc, (unsigned)r), dim3(CO_THREADS), cutout_score_lds_bytes(x.nt), x.stream, (const float*)P, sl,
                           x.rowrec, x.ndmf, x.ndmc, x.nt, x.nwidth, x.k_mad, x.rho);
        hipLaunchKernelGGL(cutout_pick_kernel, dim3((unsigned)x.nreq_max), dim3(CO_THREADS), CO_PICK_LDS_BYTES, x.stream, (const CutoutRow*)x.rowrec, sl,
                           (CutoutRecord*)o, x.ndmc, r);
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows = n;
    x.pending.swap(keep);
    *nserved = r;
    for (int k = 0; k < r; k++) served_ids[k] = sl.id[k];
    *nexpired = (int)expired.size();
    for (size_t k = 0; k < expired.size(); k++) expired_ids[k] = expired[k];
    return XENG_STATUS_SUCCESS;
}

int xengCutoutReset(void) {
    std::lock_guard<std::mutex> lk(g_comu);
    CutoutContext& x = g_co;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: not initialized");
    x.nwindows = 0;                     // (nothing is launched or cleared: the kernels decide by index what lies before window 0)
    x.pending.clear();
    return XENG_STATUS_SUCCESS;
}

int xengCutoutGetInfo(long long* nwindows_since_reset, int* npending, long long* out_bytes) {
    if (!nwindows_since_reset || !npending || !out_bytes) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CutoutGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_comu);
    CutoutContext& x = g_co;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cutout: not initialized");
    *nwindows_since_reset = x.nwindows;
    *npending = (int)x.pending.size();
    *out_bytes = (long long)x.out_bytes();
    return XENG_STATUS_SUCCESS;
}

int xengCutoutCheckGuards(int* intact) { return beam_context_check_guards(g_comu, g_co, g_co.alloc, "Cutout", intact); }
int xengCutoutMark(unsigned long long* ticket) { return beam_context_mark(g_comu, g_co, "Cutout", ticket); }
int xengCutoutWait(unsigned long long ticket) { return beam_context_wait(g_comu, g_co, "Cutout", ticket); }
int xengCutoutTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_comu, g_co, "Cutout", ticket, done); }
int xengCutoutSync(void) { return beam_context_sync(g_comu, g_co, "Cutout"); }

int xengCutoutDestroy(void) {
    std::lock_guard<std::mutex> lk(g_comu);
    return cutout_destroy_locked();
}

}  // extern "C"
