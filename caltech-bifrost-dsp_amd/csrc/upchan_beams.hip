// Host side of the fine-channel power beams from live beams (UpchanSumBeams; upchan_beams_kernels.h): a process-global context
// of its own on the beamformer's stream (BeamStreamContext, xeng_common.h).
#include <mutex>

#include "upchan_beams_kernels.h"
#include "upchan_pfb.h"
#include "xeng_common.h"

namespace xeng {

struct UpchanBeamsContext : PfbContext {      // pfb.hist holds both halves of the ping-pong history: pfb_row is two float2 rows
    int nchan = 0, nbeam = 0, pair0 = 0, npair = 0, nframe_sum = 0;
    int nframe = 0;                     // frames per gulp (F)
    int wf = 0;                         // frames per fp32 chain: min(W, F)
    int gpw = 1;                        // gulps per window (G = W / F when F | W, else 1)
    int pos = 0;                        // gulps of the window in progress already run
    float* acc = nullptr;               // f32[npair][nchan][N][4]: the window in progress when gpw > 1
    int cur = 0;                        // the half of pfb.hist the next gulp reads

    size_t hist_half() const { return (size_t)nchan * 2 * npair * (size_t)(pfb.ntap - 1) * nupchan; }     // float2 per half
};
static std::mutex g_ubmu;
static UpchanBeamsContext g_ub;

static int upchan_beams_destroy_locked() {
    if (!g_ub.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_ub);
    if (g_ub.acc) (void)hipFree(g_ub.acc);
    g_ub.pfb.release();
    g_ub = UpchanBeamsContext();
    return XENG_STATUS_SUCCESS;
}

// frames per pass (threads / 2): whole waves, no more than the gulp needs or the LDS holds
static int upchan_beams_frames(int nupchan, int nframe) {
    const int fmax = ub_max_frames(nupchan), need = (nframe + 31) / 32 * 32;
    return need < fmax ? need : fmax;
}

static size_t upchan_beams_lds(int nupchan, int ft, int ntap) { return ((size_t)ub_lds_words(nupchan, ft, ntap) + 16) * sizeof(float4); }

template <int N>
static void upchan_beams_launch(const UpchanBeamsContext& x, const float2* in, float* out) {
    const int ft = upchan_beams_frames(N, x.nframe);
    const dim3 grid((unsigned)(x.nchan * x.npair)), block((unsigned)(2 * ft));
    const size_t lds = upchan_beams_lds(N, ft, x.pfb.h ? x.pfb.ntap : 1);
    float2* hist = (float2*)x.pfb.hist;
    const UbPfb q{x.pfb.h, hist ? hist + x.cur * x.hist_half() : nullptr, hist ? hist + (1 - x.cur) * x.hist_half() : nullptr, x.pfb.ntap,
                  x.pfb.valid ? 1 : 0};
    if (x.pfb.h)
        hipLaunchKernelGGL((upchan_sum_beams_kernel<N, true>), grid, block, lds, x.stream, in, out, x.acc, x.nchan, x.nbeam, x.ntime, x.pair0,
                           x.npair, x.wf, x.gpw, x.pos, q);
    else
        hipLaunchKernelGGL((upchan_sum_beams_kernel<N, false>), grid, block, lds, x.stream, in, out, x.acc, x.nchan, x.nbeam, x.ntime, x.pair0,
                           x.npair, x.wf, x.gpw, x.pos, q);
}

// what can be refused without a context
static int upchan_beams_check_in(const char* who, const void* in_dev) {
    if (!in_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s: null input", who);
    if ((uintptr_t)in_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "%s: input %p not 16-byte aligned", who, in_dev);
    return XENG_STATUS_SUCCESS;
}

static int upchan_beams_run(const void* in_dev, void* out_dev) {
    int rc = upchan_beams_check_in("UpchanSumBeams", in_dev);
    if (rc) return rc;
    if ((uintptr_t)out_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: output %p not 16-byte aligned", out_dev);
    std::lock_guard<std::mutex> lk(g_ubmu);
    UpchanBeamsContext& x = g_ub;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSumBeams: not initialized (call xengUpchanSumBeamsInitialize)");
    if (!out_dev && x.pos == x.gpw - 1)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: null output for a gulp that completes a window (gulp %d of %d)", x.pos + 1, x.gpw);
    XENG_HIP(hipSetDevice(x.gpu));
    const float2* in = (const float2*)in_dev;
    float* out = (float*)out_dev;
    switch (x.nupchan) {
    case 8: upchan_beams_launch<8>(x, in, out); break;
    case 16: upchan_beams_launch<16>(x, in, out); break;
    case 32: upchan_beams_launch<32>(x, in, out); break;
    default: upchan_beams_launch<64>(x, in, out); break;
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    if (x.pfb.hist) {                   // (the kernel wrote the other half)
        x.cur = 1 - x.cur;
        x.pfb.valid = true;
    }
    x.pos = (x.pos + 1) % x.gpw;
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengUpchanSumBeamsInitialize(int gpu, int nchan, int nbeam, int ntime, int nupchan, int pair0, int npair, int nframe_sum) {
    if (nchan <= 0 || nbeam <= 0 || ntime <= 0 || npair <= 0 || nframe_sum <= 0 || pair0 < 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: bad sizes nchan=%d nbeam=%d ntime=%d pair0=%d npair=%d nframe_sum=%d", nchan, nbeam,
                  ntime, pair0, npair, nframe_sum);
    if (nupchan != 8 && nupchan != 16 && nupchan != 32 && nupchan != 64)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: nupchan %d not one of 8, 16, 32, 64", nupchan);
    if (ntime % nupchan) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: ntime %d not a multiple of nupchan %d", ntime, nupchan);
    const int nframe = ntime / nupchan;
    if (nframe % nframe_sum && nframe_sum % nframe)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: nframe_sum %d neither divides nor is a multiple of the %d frames of a gulp",
                  nframe_sum, nframe);
    if ((long long)pair0 + npair > nbeam / 2)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: pairs [%d, %d) outside the %d pairs of %d beams", pair0, pair0 + npair, nbeam / 2, nbeam);
    if ((long long)nchan * npair > 0x7FFFFFFFLL || (long long)nchan * nbeam * ntime > (1LL << 40))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeams: %d channels x %d beams x %d samples is more than one launch takes", nchan, nbeam, ntime);
    std::lock_guard<std::mutex> lk(g_ubmu);
    upchan_beams_destroy_locked();
    UpchanBeamsContext& x = g_ub;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nchan = nchan; x.nbeam = nbeam; x.ntime = ntime; x.nupchan = nupchan; x.pair0 = pair0; x.npair = npair; x.nframe_sum = nframe_sum;
    x.nframe = nframe;
    x.pfb_row = 2 * (size_t)nchan * 2 * npair * sizeof(float2);    // a "sample" of history: one float2 per selected (channel, beam) row, twice
    x.wf = nframe_sum < nframe ? nframe_sum : nframe;
    x.gpw = nframe_sum > nframe ? nframe_sum / nframe : 1;
    if (x.gpw > 1 && hipMalloc(&x.acc, (size_t)npair * nchan * nupchan * 4 * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        x = UpchanBeamsContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "UpchanSumBeams: cannot allocate %.3g MB of window accumulator", (double)npair * nchan * nupchan * 16 * 1e-6);
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSumBeamsGetInfo(int* gulps_per_window, int* windows_per_gulp, int* pos) {
    if (!gulps_per_window || !windows_per_gulp || !pos) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSumBeamsGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_ubmu);
    UpchanBeamsContext& x = g_ub;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSumBeams: not initialized");
    *gulps_per_window = x.gpw;
    *windows_per_gulp = x.nframe / x.wf;
    *pos = x.pos;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSumBeamsRun(const void* in_dev, void* out_dev) {
    return upchan_beams_run(in_dev, out_dev);
}

int xengUpchanSumBeamsSetPfb(int ntap, const float* coeffs) {
    std::unique_lock<std::mutex> lk(g_ubmu, std::defer_lock);
    int rc = pfb_configure(lk, g_ub, "UpchanSumBeams", ntap, coeffs);
    if (!rc) g_ub.cur = 0;
    return rc;
}

int xengUpchanSumBeamsPrime(const void* in_dev) {
    int rc = upchan_beams_check_in("UpchanSumBeamsPrime", in_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_ubmu);
    UpchanBeamsContext& x = g_ub;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSumBeams: not initialized (call xengUpchanSumBeamsInitialize)");
    if (!x.pfb.hist) return XENG_STATUS_SUCCESS;        // (no history without taps before the frame's own)
    XENG_HIP(hipSetDevice(x.gpu));
    const int nh = (x.pfb.ntap - 1) * x.nupchan;
    const long long total = (long long)x.nchan * 2 * x.npair * nh;
    const long long nblk = (total + 255) / 256;
    hipLaunchKernelGGL(upchan_sum_beams_prime_kernel, dim3((unsigned)(nblk < 4096 ? nblk : 4096)), dim3(256), 0, x.stream, (const float2*)in_dev,
                       (float2*)x.pfb.hist + (1 - x.cur) * x.hist_half(), x.nchan, x.nbeam, x.ntime, x.pair0, x.npair, nh);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.cur = 1 - x.cur;
    x.pfb.valid = true;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSumBeamsReset(void) {
    std::lock_guard<std::mutex> lk(g_ubmu);
    UpchanBeamsContext& x = g_ub;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSumBeams: not initialized");
    x.pos = 0;
    x.pfb.valid = false;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSumBeamsMark(unsigned long long* ticket) { return beam_context_mark(g_ubmu, g_ub, "UpchanSumBeams", ticket); }
int xengUpchanSumBeamsWait(unsigned long long ticket) { return beam_context_wait(g_ubmu, g_ub, "UpchanSumBeams", ticket); }
int xengUpchanSumBeamsTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_ubmu, g_ub, "UpchanSumBeams", ticket, done); }
int xengUpchanSumBeamsSync(void) { return beam_context_sync(g_ubmu, g_ub, "UpchanSumBeams"); }

int xengUpchanSumBeamsDestroy(void) {
    std::lock_guard<std::mutex> lk(g_ubmu);
    return upchan_beams_destroy_locked();
}

}  // extern "C"
