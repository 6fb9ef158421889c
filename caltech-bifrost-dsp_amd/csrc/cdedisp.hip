// Host side of the coherent dedisperser (BeamCoherentDedisperse; cdedisp_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "cdedisp_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct CdedispContext : BeamStreamContext {
    int nchan = 0, nbeam = 0, ntime = 0, pair0 = 0, npair = 0, nfft = 0, overlap = 0;
    int nrow = 0, step = 0, LN = 0;     // nchan * 2 npair, nfft - overlap, log2 nfft
    GuardedState alloc;                 // the state between its guard bands (xengCdedispCheckGuards)
    float2* tbuf = nullptr;             // cf32[nrow][nfft], inside alloc
    float2* tab = nullptr;              // cf32[npair][nchan][nfft], bit-reversed along the last axis, behind it
    float2* tw = nullptr;               // float2[nfft / 2]
    long long nsamples = 0;             // samples taken since the last reset
    long long nblocks = 0;              // blocks completed since the last reset
    int fill = 0;                       // samples of the block in progress that the time buffer holds

    size_t table_words() const { return (size_t)npair * nchan * nfft; }
    size_t state_bytes() const { return ((size_t)nrow * nfft + table_words() + (size_t)nfft / 2) * sizeof(float2); }
};
static std::mutex g_cdmu;
static CdedispContext g_cd;

static int cdedisp_destroy_locked() {
    if (!g_cd.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_cd);
    g_cd.alloc.free();
    g_cd = CdedispContext();
    return XENG_STATUS_SUCCESS;
}

static long long blocks_after(const CdedispContext& x, long long nsamples) {
    return nsamples < x.nfft ? 0 : (nsamples - x.nfft) / x.step + 1;
}

// the table in the kernel's order (bit-reversed along the last axis), uploaded; the caller has made the stream idle.  table null:
// 1 / nfft everywhere
static hipError_t cdedisp_upload_table(const CdedispContext& x, const float* table) {
    const size_t n = (size_t)x.nfft;
    std::vector<float2> t(x.table_words());
    std::vector<uint32_t> rev(n);
    for (uint32_t j = 0; j < n; j++) {
        uint32_t k = 0;
        for (int b = 0; b < x.LN; b++) k |= ((j >> b) & 1u) << (x.LN - 1 - b);
        rev[j] = k;
    }
    const float inv = 1.0f / (float)x.nfft;
    for (size_t r = 0; r < (size_t)x.npair * x.nchan; r++)
        for (size_t j = 0; j < n; j++)
            t[r * n + j] = table ? make_float2(table[2 * (r * n + rev[j])], table[2 * (r * n + rev[j]) + 1]) : make_float2(inv, 0.f);
    return hipMemcpy(x.tab, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengCdedispInitialize(int gpu, int nchan, int nbeam, int ntime, int pair0, int npair, int nfft, int overlap) {
    if (nchan <= 0 || nbeam <= 0 || ntime <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: bad sizes nchan=%d nbeam=%d ntime=%d", nchan, nbeam, ntime);
    if (pair0 < 0 || npair <= 0 || (long long)pair0 + npair > nbeam / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: pairs [%d, %lld) not a non-empty range of the %d pairs of %d beams", pair0, (long long)pair0 + npair,
                  nbeam / 2, nbeam);
    if (nfft < (1 << 8) || nfft > (1 << 13) || (nfft & (nfft - 1)))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: a transform of %d points, not a power of two from 2^8 to 2^13", nfft);
    if (overlap < 0 || (overlap & 1) || overlap > nfft / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: an overlap of %d samples, not an even number from 0 to nfft/2 = %d", overlap, nfft / 2);
    if ((long long)nchan * 2 * npair > 65535) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: %d channels x %d beams is more than one launch takes", nchan, 2 * npair);
    if ((double)nchan * nbeam * ntime * 8.0 > (double)XENG_CDEDISP_MAX_STATE_BYTES || (double)nchan * 3 * npair * nfft * 8.0 > (double)XENG_CDEDISP_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: an input of %.3g GB or a state of %.3g GB, above the limit of %.3g GB", (double)nchan * nbeam * ntime * 8e-9,
                  (double)nchan * 3 * npair * nfft * 8e-9, (double)XENG_CDEDISP_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_cdmu);
    cdedisp_destroy_locked();
    CdedispContext& x = g_cd;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nchan = nchan; x.nbeam = nbeam; x.ntime = ntime; x.pair0 = pair0; x.npair = npair; x.nfft = nfft; x.overlap = overlap;
    x.nrow = nchan * 2 * npair;
    x.step = nfft - overlap;
    while ((1 << x.LN) < nfft) x.LN++;
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, x.gpu) != hipSuccess || (size_t)lds < (size_t)nfft * sizeof(float2)) {
        (void)hipGetLastError();
        x = CdedispContext();
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: a transform of %d points needs %zu bytes of LDS, a work-group may take %d", nfft,
                  (size_t)nfft * sizeof(float2), lds);
    }
    // twiddles: float64, rounded once
    std::vector<float2> tw((size_t)nfft / 2);
    const double step = -2.0 * 3.14159265358979323846 / (double)nfft;
    for (int k = 0; k < nfft / 2; k++) tw[k] = make_float2((float)std::cos(step * k), (float)std::sin(step * k));
    if (x.alloc.open(x.state_bytes()) != hipSuccess) {
        (void)hipGetLastError();
        x = CdedispContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Cdedisp: cannot allocate %.3g MB of state", (double)nchan * 3 * npair * nfft * 8e-6);
    }
    x.tbuf = (float2*)x.alloc.data();
    x.tab = x.tbuf + (size_t)x.nrow * nfft;
    x.tw = x.tab + x.table_words();
    if (hipMemcpy(x.tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess || cdedisp_upload_table(x, nullptr) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = CdedispContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Cdedisp: cannot upload the twiddles and the table");
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengCdedispSetChirp(const float* table) {
    if (!table) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdedispSetChirp: null table");
    std::lock_guard<std::mutex> lk(g_cdmu);
    CdedispContext& x = g_cd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdedisp: not initialized (call xengCdedispInitialize)");
    for (size_t i = 0; i < 2 * x.table_words(); i++)
        if (!std::isfinite(table[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdedispSetChirp: table word %zu is not finite", i);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the table)
    XENG_HIP(cdedisp_upload_table(x, table));
    return XENG_STATUS_SUCCESS;
}

int xengCdedispRun(const void* in_dev, void* out_dev, int* nblocks) {
    if (!in_dev || !nblocks) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: null %s", in_dev ? "result" : "input");
    if ((uintptr_t)in_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: input %p or output %p not 16-byte aligned", in_dev, out_dev);
    std::lock_guard<std::mutex> lk(g_cdmu);
    CdedispContext& x = g_cd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdedisp: not initialized (call xengCdedispInitialize)");
    const int nb = (int)(blocks_after(x, x.nsamples + x.ntime) - x.nblocks);     // the blocks this call completes
    if (nb > 0 && !out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Cdedisp: the call completes %d block(s) and has a null output", nb);
    XENG_HIP(hipSetDevice(x.gpu));
    const float2* in = (const float2*)in_dev;
    float2* out = (float2*)out_dev;
    int done = 0, fill = x.fill;
    for (int t = 0; t < x.ntime;) {
        const int n = x.ntime - t < x.nfft - fill ? x.ntime - t : x.nfft - fill;
        hipLaunchKernelGGL(cdedisp_ingest_kernel, dim3((unsigned)((n + CD_THREADS - 1) / CD_THREADS), (unsigned)x.nrow), dim3(CD_THREADS), 0, x.stream, in,
                           x.tbuf, x.nbeam, x.ntime, 2 * x.pair0, 2 * x.npair, x.nfft, t, fill, n);
        t += n;
        fill += n;
        if (fill == x.nfft) {
            hipLaunchKernelGGL(cdedisp_filter_kernel, dim3((unsigned)x.nrow), dim3(CD_THREADS), (size_t)x.nfft * sizeof(float2), x.stream, x.tbuf, x.tab, x.tw,
                               out + (size_t)done * x.nrow * x.step, x.LN, x.overlap, 2 * x.npair, x.nchan);
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

int xengCdedispReset(void) {
    std::lock_guard<std::mutex> lk(g_cdmu);
    CdedispContext& x = g_cd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdedisp: not initialized");
    x.nsamples = 0;                     // (the partial block is dropped by index: the next sample goes to slot 0)
    x.nblocks = 0;
    x.fill = 0;
    return XENG_STATUS_SUCCESS;
}

int xengCdedispGetInfo(int* step, int* max_blocks_per_call, long long* nsamples_since_reset, long long* nblocks_since_reset) {
    if (!step || !max_blocks_per_call || !nsamples_since_reset || !nblocks_since_reset) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "CdedispGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_cdmu);
    CdedispContext& x = g_cd;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Cdedisp: not initialized");
    *step = x.step;
    *max_blocks_per_call = (x.ntime + x.step - 1) / x.step;
    *nsamples_since_reset = x.nsamples;
    *nblocks_since_reset = x.nblocks;
    return XENG_STATUS_SUCCESS;
}

int xengCdedispCheckGuards(int* intact) { return beam_context_check_guards(g_cdmu, g_cd, g_cd.alloc, "Cdedisp", intact); }
int xengCdedispMark(unsigned long long* ticket) { return beam_context_mark(g_cdmu, g_cd, "Cdedisp", ticket); }
int xengCdedispWait(unsigned long long ticket) { return beam_context_wait(g_cdmu, g_cd, "Cdedisp", ticket); }
int xengCdedispTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_cdmu, g_cd, "Cdedisp", ticket, done); }
int xengCdedispSync(void) { return beam_context_sync(g_cdmu, g_cd, "Cdedisp"); }

int xengCdedispDestroy(void) {
    std::lock_guard<std::mutex> lk(g_cdmu);
    return cdedisp_destroy_locked();
}

}  // extern "C"
