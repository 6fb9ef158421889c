// Host side of the acceleration search of the long-segment spectra (BeamAccelSearch; accel_kernels.h): a process-global context of
// its own on the beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "accel_kernels.h"
#include "xeng_common.h"

namespace xeng {

constexpr long long AC_MAX_SCRATCH_BYTES = 1LL << 31;   // scr, P, S, part and mv of one batch
constexpr int AC_MAX_BATCH = 32768;                     // (a batch is the y extent of a grid)

struct AccelContext : BeamStreamContext {
    int npair = 0, ndm = 0, nwin = 0, nprod = 0, nt = 0, nlevel = 0, nwhite = 0, nband = 0, ntrial = 0, izero = -1;
    int nser = 0;                       // npair * ndm
    int LN = 0, LN1 = 0, LN2 = 0, lb = 0;   // log2 (nt / 2) = LN1 + LN2, log2 nwhite
    int sb_alloc = 0, sb = 0;           // series per batch: what the scratch holds, and what the launches take (xengAccelSetBatch)
    std::vector<double> alpha;          // [ntrial]
    GuardedState alloc;                 // the state between its guard bands (xengAccelCheckGuards)
    float* tbuf = nullptr;              // f32[nser][nt], inside alloc
    PlongRecord* trec = nullptr;        // [ntrial][nser][nlevel][nband], behind it: the trial records of the segment that completed last
    float2* scr = nullptr;              // cf32[sb_alloc][nt/2]
    float* P = nullptr;                 // f32[sb_alloc][nt/2]
    float* S = nullptr;                 // f32[sb_alloc][nt/2], the whitened spectrum of one trial
    PlongRecord* part = nullptr;        // [sb_alloc][nlevel][nband][16]
    PlongMean* mv = nullptr;            // [sb_alloc], of one trial
    float2* tw = nullptr;               // float2[nt/2], then tws float2[nt/4], tw1 float2[N1/2] and tw2 float2[N2/2]
    float2* tws = nullptr;
    float2* tw1 = nullptr;
    float2* tw2 = nullptr;
    float* cnt = nullptr;               // f32[nt/2 / nwhite]
    int* kedge = nullptr;               // i32[nband + 1]
    uint8_t* keep = nullptr;            // u8[nt/2]
    long long nwindows = 0;             // windows taken since the last reset
    long long nsegs = 0;                // segments completed since the last reset
    bool have = false;                  // trec holds a segment's records

    size_t nrec() const { return (size_t)nser * nlevel * nband; }                   // records of one trial
    size_t part_words() const { return (size_t)nlevel * nband * PL_NTILE; }         // partial records of one series
    size_t twiddle_words() const { return (size_t)nt / 2 + (size_t)nt / 4 + (((size_t)1 << LN1) + ((size_t)1 << LN2)) / 2; }
    size_t state_bytes() const {
        const size_t n = (size_t)nt / 2;
        return (size_t)nser * nt * sizeof(float) + (size_t)ntrial * nrec() * sizeof(PlongRecord) +
               (size_t)sb_alloc * (n * (sizeof(float2) + 2 * sizeof(float)) + part_words() * sizeof(PlongRecord) + sizeof(PlongMean)) +
               twiddle_words() * sizeof(float2) + n / nwhite * sizeof(float) + ((size_t)nband + 1) * sizeof(int) + n;
    }
};
static std::mutex g_acmu;
static AccelContext g_ac;

static int accel_destroy_locked() {
    if (!g_ac.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_ac);
    g_ac.alloc.free();
    g_ac = AccelContext();
    return XENG_STATUS_SUCCESS;
}

static int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}

// the mask and, per whitening block, the number of its bins that count (k >= 1, kept), uploaded; the caller has made the stream idle
static hipError_t accel_upload_mask(const AccelContext& x, const unsigned char* keep) {
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
static void accel_ingest(const AccelContext& x, const float* in, int nc, int slot0) {
    const dim3 g((unsigned)((x.nser + PL_TILE - 1) / PL_TILE), (unsigned)((nc + PL_TILE - 1) / PL_TILE));
    hipLaunchKernelGGL((plong_ingest_kernel<NPROD>), g, dim3(PL_THREADS), 0, x.stream, in, x.tbuf, x.nser, x.nt, slot0, nc);
}

// the launches of a completed segment: per batch and, inside it, per trial the gathered mean and columns pass, then plong's rows
// pass, untangle, whitening, sums and reduce on the batch's buffers; behind the last batch the best over the trials
static void accel_segment(const AccelContext& x, AccelRecord* out) {
    const unsigned N1 = 1u << x.LN1, N2 = 1u << x.LN2;
    const int lr = pl_lrows(x.LN2), lw = pl_lwhite(x.lb);
    const size_t lds_cols = (size_t)N1 * PL_TC * sizeof(float2), lds_rows = ((size_t)N2 << lr) * sizeof(float2);
    const size_t lds_power = (size_t)PL_TC * (N1 + PL_PPAD) * sizeof(float), lds_white = sizeof(float) << lw;
    const size_t per = (size_t)x.nlevel * x.nband;
    for (int s0 = 0; s0 < x.nser; s0 += x.sb) {
        const unsigned ns = (unsigned)(x.nser - s0 < x.sb ? x.nser - s0 : x.sb);
        const long long nrec = (long long)ns * (long long)per;
        for (int a = 0; a < x.ntrial; a++) {
            const double al = x.alpha[a];
            hipLaunchKernelGGL(accel_mean_kernel, dim3(ns), dim3(PL_THREADS), 0, x.stream, x.tbuf, x.mv, x.LN, s0, al);
            hipLaunchKernelGGL(accel_cols_kernel, dim3(N2 / PL_TC, ns), dim3(PL_THREADS), lds_cols, x.stream, x.tbuf, x.mv, x.scr, x.tw1, x.LN1, x.LN2, s0, al);
            hipLaunchKernelGGL(plong_rows_kernel, dim3(N1 >> lr, ns), dim3(PL_THREADS), lds_rows, x.stream, x.scr, x.tws, x.tw2, x.LN1, x.LN2);
            hipLaunchKernelGGL(plong_power_kernel, dim3(N2 / PL_TC, ns), dim3(PL_THREADS), lds_power, x.stream, x.scr, x.tw, x.P, x.LN1, x.LN2);
            hipLaunchKernelGGL(plong_whiten_kernel, dim3(1u << (x.LN - lw), ns), dim3(PL_THREADS), lds_white, x.stream, x.P, x.S, x.keep, x.cnt, x.mv, x.LN, x.lb,
                               1, 0);
            hipLaunchKernelGGL(plong_sums_kernel, dim3(PL_NTILE, ns), dim3(PL_THREADS), 0, x.stream, x.S, x.kedge, x.part, x.LN, x.nlevel, x.nband, 0);
            hipLaunchKernelGGL(plong_reduce_kernel, dim3((unsigned)((nrec + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, x.stream, x.part,
                               x.trec + (size_t)a * x.nrec() + (size_t)s0 * per, nrec);
        }
    }
    const long long nall = (long long)x.nrec();
    hipLaunchKernelGGL(accel_best_kernel, dim3((unsigned)((nall + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, x.stream, x.trec, out, nall, x.ntrial,
                       x.izero);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengAccelInitialize(int gpu, int npair, int ndm, int nwin, int nprod, int nt, int nlevel, int nwhite, int nband, const int* kedge, int ntrial,
                        const double* alpha) {
    if (npair <= 0 || ndm <= 0 || nwin <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: bad sizes npair=%d ndm=%d nwin=%d", npair, ndm, nwin);
    if (nprod != 1 && nprod != 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: nprod %d not 1 (I) or 4 (XX, YY, Re XY*, Im XY*)", nprod);
    if (nt < (1 << 15) || nt > (1 << 20) || (nt & (nt - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: a segment of %d windows, not a power of two from 2^15 to 2^20", nt);
    if (nlevel < 1 || nlevel > PL_MAX_LEVEL) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: %d harmonic levels, not 1 to %d", nlevel, PL_MAX_LEVEL);
    if (nwhite < 8 || nwhite > (1 << 13) || (nwhite & (nwhite - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: a whitening block of %d bins, not a power of two from 8 to 2^13", nwhite);
    if (nband < 1 || nband > PL_MAX_BAND) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: %d bands, not 1 to %d", nband, PL_MAX_BAND);
    if (!kedge) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: null band edges");
    if (kedge[0] < 1 || kedge[0] >= nt / 32) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: the lowest edge %d not in 1 .. nt/32 - 1 = %d", kedge[0], nt / 32 - 1);
    for (int b = 0; b < nband; b++)
        if (kedge[b + 1] <= kedge[b] || kedge[b + 1] > nt / 2)
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: edge %d is %d after %d: not strictly ascending up to nt/2 = %d", b + 1, kedge[b + 1], kedge[b], nt / 2);
    if (nwin > nt) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: %d windows a call are more than a segment of %d", nwin, nt);
    if ((long long)npair * ndm > (1LL << 24))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: %d pairs x %d trials is more than one launch takes", npair, ndm);
    if (ntrial < 1 || ntrial > AC_MAX_TRIAL) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: %d acceleration trials, not 1 to %d", ntrial, AC_MAX_TRIAL);
    if (!alpha) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: null trial table");
    int izero = -1;
    for (int a = 0; a < ntrial; a++) {
        if (!std::isfinite(alpha[a])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: alpha of trial %d is not finite", a);
        // beyond this the index map would leave the segment (and run backwards)
        if (std::fabs(alpha[a]) * (double)nt > 0.5)
            XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: |alpha| = %.6g of trial %d is above 0.5 / nt = %.6g", std::fabs(alpha[a]), a, 0.5 / (double)nt);
        if (izero < 0 && alpha[a] == 0.0) izero = a;
    }
    // the batch: as many series as 2 GiB of scratch hold
    const double per_series = (double)nt / 2 * 16.0 + (double)nlevel * nband * PL_NTILE * 8.0 + 8.0;
    long long sb = (long long)((double)AC_MAX_SCRATCH_BYTES / per_series);
    if (sb > AC_MAX_BATCH) sb = AC_MAX_BATCH;
    if (sb > (long long)npair * ndm) sb = (long long)npair * ndm;
    if (sb < 1) sb = 1;
    const double state = (double)npair * ndm * ((double)nt * 4.0 + (double)ntrial * nlevel * nband * 8.0) + (double)sb * per_series + (double)nt * 8.0;
    if (state > (double)XENG_ACCEL_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: %d series of %d windows and %d trials need %.3g GB of state, above the limit of %.3g GB", npair * ndm, nt,
                  ntrial, state * 1e-9, (double)XENG_ACCEL_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_acmu);
    accel_destroy_locked();
    AccelContext& x = g_ac;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.npair = npair; x.ndm = ndm; x.nwin = nwin; x.nprod = nprod; x.nt = nt; x.nlevel = nlevel; x.nwhite = nwhite; x.nband = nband;
    x.ntrial = ntrial; x.izero = izero;
    x.alpha.assign(alpha, alpha + ntrial);
    x.nser = npair * ndm;
    x.sb_alloc = x.sb = (int)sb;
    const int n = nt / 2;
    x.LN = ilog2(n);
    x.LN1 = pl_ln1(x.LN);
    x.LN2 = x.LN - x.LN1;
    x.lb = ilog2(nwhite);
    const size_t N1 = (size_t)1 << x.LN1, N2 = (size_t)1 << x.LN2;
    size_t need = N1 * PL_TC * sizeof(float2);
    if ((N2 << pl_lrows(x.LN2)) * sizeof(float2) > need) need = (N2 << pl_lrows(x.LN2)) * sizeof(float2);
    if (sizeof(float) << pl_lwhite(x.lb) > need) need = sizeof(float) << pl_lwhite(x.lb);
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, x.gpu) != hipSuccess || (size_t)lds < need) {
        (void)hipGetLastError();
        x = AccelContext();
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: a segment of %d windows needs %zu bytes of LDS, a work-group may take %d", nt, need, lds);
    }
    // twiddles: float64, rounded once; tw, tws, tw1 and tw2 one behind the other (the tables of plong.hip)
    std::vector<float2> tw;
    tw.reserve(x.twiddle_words());
    for (size_t len : {(size_t)nt, (size_t)n, N1, N2}) {
        const double step = -2.0 * 3.14159265358979323846 / (double)len;
        for (size_t k = 0; k < len / 2; k++) tw.push_back(make_float2((float)std::cos(step * (double)k), (float)std::sin(step * (double)k)));
    }
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = AccelContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Accel: cannot allocate %.3g MB of state", state * 1e-6);
    }
    x.tbuf = (float*)x.alloc.data();
    x.scr = (float2*)(x.tbuf + (size_t)x.nser * nt);
    x.trec = (PlongRecord*)(x.scr + (size_t)x.sb_alloc * n);
    x.part = x.trec + (size_t)ntrial * x.nrec();
    x.mv = (PlongMean*)(x.part + (size_t)x.sb_alloc * x.part_words());
    x.tw = (float2*)(x.mv + x.sb_alloc);
    x.tws = x.tw + n;
    x.tw1 = x.tws + n / 2;
    x.tw2 = x.tw1 + N1 / 2;
    x.P = (float*)(x.tw2 + N2 / 2);
    x.S = x.P + (size_t)x.sb_alloc * n;
    x.cnt = x.S + (size_t)x.sb_alloc * n;
    x.kedge = (int*)(x.cnt + n / nwhite);
    x.keep = (uint8_t*)(x.kedge + nband + 1);
    if (hipMemcpy(x.tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(x.kedge, kedge, ((size_t)nband + 1) * sizeof(int), hipMemcpyHostToDevice) != hipSuccess || accel_upload_mask(x, nullptr) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = AccelContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Accel: cannot upload the twiddles, the edges and the mask");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengAccelSetMask(const unsigned char* keep) {
    std::lock_guard<std::mutex> lk(g_acmu);
    AccelContext& x = g_ac;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Accel: not initialized (call xengAccelInitialize)");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the mask)
    XENG_HIP(accel_upload_mask(x, keep));
    return XENG_STATUS_SUCCESS;
}

int xengAccelSetBatch(int nser_batch) {
    std::lock_guard<std::mutex> lk(g_acmu);
    AccelContext& x = g_ac;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Accel: not initialized (call xengAccelInitialize)");
    if (nser_batch < 0 || nser_batch > x.sb_alloc) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: a batch of %d series, not 0 to %d", nser_batch, x.sb_alloc);
    x.sb = nser_batch ? nser_batch : x.sb_alloc;
    return XENG_STATUS_SUCCESS;
}

int xengAccelGetBatch(int* nser_batch, int* nser_batch_max) {
    if (!nser_batch || !nser_batch_max) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "AccelGetBatch: null result");
    std::lock_guard<std::mutex> lk(g_acmu);
    AccelContext& x = g_ac;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Accel: not initialized");
    *nser_batch = x.sb;
    *nser_batch_max = x.sb_alloc;
    return XENG_STATUS_SUCCESS;
}

int xengAccelRun(const void* in_dev, int nwin_call, void* out_dev, int* completed) {
    if (!in_dev || !completed) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: null %s", in_dev ? "result" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_acmu);
    AccelContext& x = g_ac;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Accel: not initialized (call xengAccelInitialize)");
    if (nwin_call < 1 || nwin_call > x.nwin) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: %d windows in a call, not 1 to %d", nwin_call, x.nwin);
    const int pos = (int)(x.nwindows % x.nt);
    const int head = nwin_call < x.nt - pos ? nwin_call : x.nt - pos;   // windows of the call that go into the segment in progress
    const bool seg_done = pos + head == x.nt;
    if (seg_done && !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Accel: the call completes a segment and has a null output");
    XENG_HIP(hipSetDevice(x.gpu));
    const float* in = (const float*)in_dev;
    if (x.nprod == 1)
        accel_ingest<1>(x, in, head, pos);
    else
        accel_ingest<4>(x, in, head, pos);
    if (seg_done) {
        accel_segment(x, (AccelRecord*)out_dev);
        if (nwin_call > head) {
            in += (size_t)head * x.nser * x.nprod;
            if (x.nprod == 1)
                accel_ingest<1>(x, in, nwin_call - head, 0);
            else
                accel_ingest<4>(x, in, nwin_call - head, 0);
        }
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.nwindows += nwin_call;
    if (seg_done) {
        x.nsegs++;
        x.have = true;
    }
    *completed = seg_done ? 1 : 0;
    return XENG_STATUS_SUCCESS;
}

int xengAccelReset(void) {
    std::lock_guard<std::mutex> lk(g_acmu);
    AccelContext& x = g_ac;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Accel: not initialized");
    x.nwindows = 0;                     // (the partial segment is dropped by index: the next one fills the time buffer from slot 0)
    x.nsegs = 0;
    x.have = false;
    return XENG_STATUS_SUCCESS;
}

int xengAccelGetInfo(long long* nwindows_since_reset, long long* nsegments_complete) {
    if (!nwindows_since_reset || !nsegments_complete) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "AccelGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_acmu);
    AccelContext& x = g_ac;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Accel: not initialized");
    *nwindows_since_reset = x.nwindows;
    *nsegments_complete = x.nsegs;
    return XENG_STATUS_SUCCESS;
}

int xengAccelGetTrialRecords(int series0, int nser, void* records_host) {
    if (!records_host) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "AccelGetTrialRecords: null result");
    std::lock_guard<std::mutex> lk(g_acmu);
    AccelContext& x = g_ac;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Accel: not initialized");
    if (series0 < 0 || nser < 1 || (long long)series0 + nser > x.nser)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "AccelGetTrialRecords: series [%d, %lld) not a non-empty range of the %d", series0, (long long)series0 + nser, x.nser);
    if (!x.have) XENG_FAIL(XENG_STATUS_INVALID_STATE, "AccelGetTrialRecords: no segment is complete since the reset");
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));
    const size_t per = (size_t)x.nlevel * x.nband, run = (size_t)nser * per;
    for (int a = 0; a < x.ntrial; a++)
        XENG_HIP(hipMemcpy((PlongRecord*)records_host + (size_t)a * run, x.trec + (size_t)a * x.nrec() + (size_t)series0 * per, run * sizeof(PlongRecord),
                           hipMemcpyDeviceToHost));
    return XENG_STATUS_SUCCESS;
}

int xengAccelCheckGuards(int* intact) { return beam_context_check_guards(g_acmu, g_ac, g_ac.alloc, "Accel", intact); }
int xengAccelMark(unsigned long long* ticket) { return beam_context_mark(g_acmu, g_ac, "Accel", ticket); }
int xengAccelWait(unsigned long long ticket) { return beam_context_wait(g_acmu, g_ac, "Accel", ticket); }
int xengAccelTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_acmu, g_ac, "Accel", ticket, done); }
int xengAccelSync(void) { return beam_context_sync(g_acmu, g_ac, "Accel"); }

int xengAccelDestroy(void) {
    std::lock_guard<std::mutex> lk(g_acmu);
    return accel_destroy_locked();
}

}  // extern "C"
