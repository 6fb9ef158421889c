// Host side of the long-transform coherent dedisperser (BeamCoherentDedisperseLong; cdlong_kernels.h): a process-global context of
// its own on the beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "cdlong_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct CdlongContext : BeamStreamContext {
    int nchan = 0, nbeam = 0, ntime = 0, pair0 = 0, npair = 0, nfft = 0, overlap = 0;
    int nrow = 0, step = 0, LN = 0, LN1 = 0, LN2 = 0;   // nchan * 2 npair, nfft - overlap, log2 nfft = LN1 + LN2
    GuardedState alloc;                 // the state between its guard bands (xengCdlongCheckGuards)
    float2* tbuf = nullptr;             // cf32[nrow][nfft], inside alloc
    float2* scr = nullptr;              // cf32[nrow][nfft], the matrix between the passes, behind it
    float2* tab = nullptr;              // cf32[npair][nchan][nfft] in pass B's order
    float2* tws = nullptr;              // float2[nfft / 2], then tw1 float2[N1 / 2] and tw2 float2[N2 / 2]
    float2* tw1 = nullptr;
    float2* tw2 = nullptr;
    long long nsamples = 0;             // samples taken since the last reset
    long long nblocks = 0;              // blocks completed since the last reset
    int fill = 0;                       // samples of the block in progress that the time buffer holds

    size_t pair_words() const { return (size_t)nchan * nfft; }
    size_t twiddle_words() const { return ((size_t)nfft + ((size_t)1 << LN1) + ((size_t)1 << LN2)) / 2; }
    size_t state_bytes() const { return (2 * (size_t)nrow * nfft + (size_t)npair * pair_words() + twiddle_words()) * sizeof(float2); }
};
static std::mutex g_clmu;
static CdlongContext g_cl;

static int cdlong_destroy_locked() {
    if (!g_cl.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_cl);
    g_cl.alloc.free();
    g_cl = CdlongContext();
    return XENG_STATUS_SUCCESS;
}

static long long blocks_after(const CdlongContext& x, long long nsamples) {
    return nsamples < x.nfft ? 0 : (nsamples - x.nfft) / x.step + 1;
}

static uint32_t bitrev(uint32_t j, int bits) {
    uint32_t k = 0;
    for (int b = 0; b < bits; b++) k |= ((j >> b) & 1u) << (bits - 1 - b);
    return k;
}

// one pair's table, cf32[nchan][nfft] in natural order, put into the order pass B meets it (element r * N2 + j is bin
// bitrev(r) + N1 * bitrev(j)) and uploaded; the caller has made the stream idle.  table null: 1 / nfft everywhere
static hipError_t cdlong_upload_pair(const CdlongContext& x, int pair, const float* table) {
    const size_t n = (size_t)x.nfft, N1 = (size_t)1 << x.LN1, N2 = (size_t)1 << x.LN2;
    std::vector<float2> t(x.pair_words(), make_float2(1.0f / (float)x.nfft, 0.f));
    if (table) {
        std::vector<uint32_t> bin(n);
        for (size_t r = 0; r < N1; r++)
            for (size_t j = 0; j < N2; j++) bin[r * N2 + j] = bitrev((uint32_t)r, x.LN1) + (uint32_t)N1 * bitrev((uint32_t)j, x.LN2);
        for (size_t c = 0; c < (size_t)x.nchan; c++)
            for (size_t i = 0; i < n; i++) t[c * n + i] = make_float2(table[2 * (c * n + bin[i])], table[2 * (c * n + bin[i]) + 1]);
    }
    return hipMemcpy(x.tab + (size_t)pair * x.pair_words(), t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengCdlongInitialize(int gpu, int nchan, int nbeam, int ntime, int pair0, int npair, int nfft, int overlap) {
    if (nchan <= 0 || nbeam <= 0 || ntime <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: bad sizes nchan=%d nbeam=%d ntime=%d", nchan, nbeam, ntime);
    if (pair0 < 0 || npair <= 0 || (long long)pair0 + npair > nbeam / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: pairs [%d, %lld) not a non-empty range of the %d pairs of %d beams", pair0, (long long)pair0 + npair,
                  nbeam / 2, nbeam);
    if (nfft < (1 << 14) || nfft > (1 << 20) || (nfft & (nfft - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: a transform of %d points, not a power of two from 2^14 to 2^20", nfft);
    if (overlap < 0 || (overlap & 1) || overlap > nfft / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: an overlap of %d samples, not an even number from 0 to nfft/2 = %d", overlap, nfft / 2);
    if ((long long)nchan * 2 * npair > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: %d channels x %d beams is more than one launch takes", nchan, 2 * npair);
    // the state: time buffer and scratch (2 npair rows per channel each), the table (npair), the twiddles (less than a row)
    const double state = ((double)nchan * 5 * npair + 1) * nfft * 8.0;
    if ((double)nchan * nbeam * ntime * 8.0 > (double)XENG_CDLONG_MAX_STATE_BYTES || state > (double)XENG_CDLONG_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: an input of %.3g GB or a state of %.3g GB, above the limit of %.3g GB", (double)nchan * nbeam * ntime * 8e-9,
                  state * 1e-9, (double)XENG_CDLONG_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_clmu);
    cdlong_destroy_locked();
    CdlongContext& x = g_cl;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nchan = nchan; x.nbeam = nbeam; x.ntime = ntime; x.pair0 = pair0; x.npair = npair; x.nfft = nfft; x.overlap = overlap;
    x.nrow = nchan * 2 * npair;
    x.step = nfft - overlap;
    while ((1 << x.LN) < nfft) x.LN++;
    x.LN1 = cl_ln1(x.LN);
    x.LN2 = x.LN - x.LN1;
    const size_t N1 = (size_t)1 << x.LN1, N2 = (size_t)1 << x.LN2;
    const size_t need = (N1 * CL_TC > (N2 << cl_lrows(x.LN2)) ? N1 * CL_TC : (N2 << cl_lrows(x.LN2))) * sizeof(float2);
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, x.gpu) != hipSuccess || (size_t)lds < need) {
        (void)hipGetLastError();
        x = CdlongContext();
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: a transform of %d points needs %zu bytes of LDS, a work-group may take %d", nfft, need, lds);
    }
    // twiddles: float64, rounded once; tws, tw1 and tw2 one behind the other
    std::vector<float2> tw;
    tw.reserve(x.twiddle_words());
    for (size_t n : {(size_t)nfft, N1, N2}) {
        const double step = -2.0 * 3.14159265358979323846 / (double)n;
        for (size_t k = 0; k < n / 2; k++) tw.push_back(make_float2((float)std::cos(step * (double)k), (float)std::sin(step * (double)k)));
    }
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = CdlongContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Cdlong: cannot allocate %.3g MB of state", state * 1e-6);
    }
    x.tbuf = (float2*)x.alloc.data();
    x.scr = x.tbuf + (size_t)x.nrow * nfft;
    x.tab = x.scr + (size_t)x.nrow * nfft;
    x.tws = x.tab + (size_t)npair * x.pair_words();
    x.tw1 = x.tws + (size_t)nfft / 2;
    x.tw2 = x.tw1 + N1 / 2;
    hipError_t e = hipMemcpy(x.tws, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice);
    for (int p = 0; p < npair && e == hipSuccess; p++) e = cdlong_upload_pair(x, p, nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = CdlongContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Cdlong: cannot upload the twiddles and the table");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengCdlongSetChirp(int pair, const float* table) {
    if (!table) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdlongSetChirp: null table");
    if (pair < 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdlongSetChirp: pair %d", pair);
    std::lock_guard<std::mutex> lk(g_clmu);
    CdlongContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdlong: not initialized (call xengCdlongInitialize)");
    if (pair >= x.npair) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdlongSetChirp: pair %d of %d", pair, x.npair);
    for (size_t i = 0; i < 2 * x.pair_words(); i++)
        if (!std::isfinite(table[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdlongSetChirp: table word %zu is not finite", i);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the table)
    XENG_HIP(cdlong_upload_pair(x, pair, table));
    return XENG_STATUS_SUCCESS;
}

int xengCdlongRun(const void* in_dev, void* out_dev, int* nblocks) {
    if (!in_dev || !nblocks) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: null %s", in_dev ? "result" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_clmu);
    CdlongContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdlong: not initialized (call xengCdlongInitialize)");
    const int nb = (int)(blocks_after(x, x.nsamples + x.ntime) - x.nblocks);     // the blocks this call completes
    if (nb > 0 && !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdlong: the call completes %d block(s) and has a null output", nb);
    XENG_HIP(hipSetDevice(x.gpu));
    const float2* in = (const float2*)in_dev;
    float2* out = (float2*)out_dev;
    const unsigned N1 = 1u << x.LN1, N2 = 1u << x.LN2, nrow = (unsigned)x.nrow;
    const int lr = cl_lrows(x.LN2);
    const size_t lds_cols = (size_t)N1 * CL_TC * sizeof(float2), lds_rows = ((size_t)N2 << lr) * sizeof(float2);
    int done = 0, fill = x.fill;
    for (int t = 0; t < x.ntime;) {
        const int n = x.ntime - t < x.nfft - fill ? x.ntime - t : x.nfft - fill;
        hipLaunchKernelGGL(cdlong_ingest_kernel, dim3((unsigned)((n + CL_THREADS - 1) / CL_THREADS), nrow), dim3(CL_THREADS), 0, x.stream, in, x.tbuf,
                           x.nbeam, x.ntime, 2 * x.pair0, 2 * x.npair, x.nfft, t, fill, n);
        t += n;
        fill += n;
        if (fill == x.nfft) {
            // A, the overlap behind it (cdlong_kernels.h: why there is no race), B, C
            hipLaunchKernelGGL(cdlong_cols_fwd_kernel, dim3(N2 / CL_TC, nrow), dim3(CL_THREADS), lds_cols, x.stream, x.tbuf, x.scr, x.tw1, x.LN1, x.LN2);
            if (x.overlap)
                hipLaunchKernelGGL(cdlong_tail_kernel, dim3((unsigned)((x.overlap + CL_THREADS - 1) / CL_THREADS), nrow), dim3(CL_THREADS), 0, x.stream, x.tbuf,
                                   x.nfft, x.overlap);
            hipLaunchKernelGGL(cdlong_rows_kernel, dim3(N1 >> lr, nrow), dim3(CL_THREADS), lds_rows, x.stream, x.scr, x.tab, x.tws, x.tw2, x.LN1, x.LN2,
                               2 * x.npair, x.nchan);
            hipLaunchKernelGGL(cdlong_cols_inv_kernel, dim3(N2 / CL_TC, nrow), dim3(CL_THREADS), lds_cols, x.stream, x.scr, out + (size_t)done * x.nrow * x.step,
                               x.tw1, x.LN1, x.LN2, x.overlap);
            done++;
            fill = x.overlap;
        }
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.fill = fill;
    x.nsamples += x.ntime;
    x.nblocks += done;
    *nblocks = done;
    return XENG_STATUS_SUCCESS;
}

int xengCdlongReset(void) {
    std::lock_guard<std::mutex> lk(g_clmu);
    CdlongContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdlong: not initialized");
    x.nsamples = 0;                     // (the partial block is dropped by index: the next sample goes to slot 0)
    x.nblocks = 0;
    x.fill = 0;
    return XENG_STATUS_SUCCESS;
}

int xengCdlongGetInfo(int* step, int* max_blocks_per_call, long long* nsamples_since_reset, long long* nblocks_since_reset) {
    if (!step || !max_blocks_per_call || !nsamples_since_reset || !nblocks_since_reset) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdlongGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_clmu);
    CdlongContext& x = g_cl;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdlong: not initialized");
    *step = x.step;
    *max_blocks_per_call = (x.ntime + x.step - 1) / x.step;
    *nsamples_since_reset = x.nsamples;
    *nblocks_since_reset = x.nblocks;
    return XENG_STATUS_SUCCESS;
}

int xengCdlongCheckGuards(int* intact) { return beam_context_check_guards(g_clmu, g_cl, g_cl.alloc, "Cdlong", intact); }
int xengCdlongMark(unsigned long long* ticket) { return beam_context_mark(g_clmu, g_cl, "Cdlong", ticket); }
int xengCdlongWait(unsigned long long ticket) { return beam_context_wait(g_clmu, g_cl, "Cdlong", ticket); }
int xengCdlongTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_clmu, g_cl, "Cdlong", ticket, done); }
int xengCdlongSync(void) { return beam_context_sync(g_clmu, g_cl, "Cdlong"); }

int xengCdlongDestroy(void) {
    std::lock_guard<std::mutex> lk(g_clmu);
    return cdlong_destroy_locked();
}

}  // extern "C"
