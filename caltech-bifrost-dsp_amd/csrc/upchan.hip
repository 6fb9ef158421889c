// Host side of the upchannelising beamformer (UpchanBeamform; upchan_kernels.h): a process-global context of its own, beside
// (not inside) the Beamform context, whose kernels run on the beamformer's stream (STREAM_BEAM) and tick its clock, so that
// rings declared 'beam' and their span stamps cover them unchanged.
#include <mutex>

#include "upchan_kernels.h"
#include "upchan_pfb.h"
#include "xeng_common.h"

namespace xeng {

struct UpchanContext : PfbContext {
    int ninput = 0, nchan = 0, nbeam = 0, nframe_sum = 0;
    bool dual = false;                  // xengUpchanInitializeDualPol: [XX, YY, Re XY*, Im XY*] per pair of beams
};
static std::mutex g_umu;
static UpchanContext g_u;

static int upchan_destroy_locked() {
    if (!g_u.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_u);
    g_u.pfb.release();
    g_u = UpchanContext();
    return XENG_STATUS_SUCCESS;
}

// frames per work-group: UC_FT in voltage mode; in power mode whole windows (as many as fit in UC_FT frames, or one longer one)
static int upchan_run_frames(int nframe_sum) {
    if (nframe_sum == 0) return UC_FT;
    return nframe_sum <= UC_FT ? nframe_sum * (UC_FT / nframe_sum) : nframe_sum;
}

static int upchan_threads(int nbeam, int nupchan) {
    const int units = nbeam * nupchan;
    return units >= 256 ? 256 : (units + 63) / 64 * 64;
}

// pfb...: nothing (the plain FFT) or one UcPfb (the PFB instantiations)
template <int N, typename... Pfb>
static void upchan_launch_n(int ppt, dim3 grid, dim3 block, hipStream_t s, const uint8_t* in0, const uint8_t* in1, int ntime0,
                            const float2* w, float* out, const UpchanContext& x, int nframe, int run, Pfb... pfb) {
    if (x.dual) {                       // (ppt beams per thread: whole pairs, 2 or 4)
        if (ppt == 2) hipLaunchKernelGGL((upchan_beamform_kernel<N, 2, true, Pfb...>), grid, block, 0, s, in0, in1, ntime0, w, out, x.nchan, x.ninput, x.nbeam, nframe, x.nframe_sum, run, pfb...);
        else hipLaunchKernelGGL((upchan_beamform_kernel<N, 4, true, Pfb...>), grid, block, 0, s, in0, in1, ntime0, w, out, x.nchan, x.ninput, x.nbeam, nframe, x.nframe_sum, run, pfb...);
        return;
    }
    switch (ppt) {
    case 1: hipLaunchKernelGGL((upchan_beamform_kernel<N, 1, false, Pfb...>), grid, block, 0, s, in0, in1, ntime0, w, out, x.nchan, x.ninput, x.nbeam, nframe, x.nframe_sum, run, pfb...); break;
    case 2: hipLaunchKernelGGL((upchan_beamform_kernel<N, 2, false, Pfb...>), grid, block, 0, s, in0, in1, ntime0, w, out, x.nchan, x.ninput, x.nbeam, nframe, x.nframe_sum, run, pfb...); break;
    default: hipLaunchKernelGGL((upchan_beamform_kernel<N, 4, false, Pfb...>), grid, block, 0, s, in0, in1, ntime0, w, out, x.nchan, x.ninput, x.nbeam, nframe, x.nframe_sum, run, pfb...); break;
    }
}

template <int N>
static void upchan_launch_pfb(int ppt, dim3 grid, dim3 block, hipStream_t s, const uint8_t* in0, const uint8_t* in1, int ntime0,
                              const float2* w, float* out, const UpchanContext& x, int nframe, int run) {
    if (x.pfb.h) upchan_launch_n<N>(ppt, grid, block, s, in0, in1, ntime0, w, out, x, nframe, run, x.pfb.args());
    else upchan_launch_n<N>(ppt, grid, block, s, in0, in1, ntime0, w, out, x, nframe, run);
}

static int upchan_run(const void* in0_dev, int ntime0, const void* in1_dev, void* out_dev, const void* weights_dev) {
    if (!out_dev || !weights_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: null buffer");
    if ((uintptr_t)weights_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: weights %p / output %p not 16-byte aligned", weights_dev, out_dev);
    std::unique_lock<std::mutex> lk(g_umu, std::defer_lock);
    UpchanContext& x = g_u;
    int rc = gulp_begin(lk, x, "Upchan", "", in0_dev, &in1_dev, &ntime0);
    if (rc) return rc;
    XENG_HIP(hipSetDevice(x.gpu));
    const int nframe = x.ntime / x.nupchan, run = upchan_run_frames(x.nframe_sum);
    // a thread owns ppt beams of one fine channel.  Dual-pol: ppt / 2 whole pairs (1 or 2, as nbeam / 2 * nupchan <= 512) on the
    // power mode's thread count, so that phase A has as many threads (with fewer, each would run two FFTs per chunk: 1.6x the
    // time at 4 beams); the threads past the last pair only help with phase A
    const int nthr = upchan_threads(x.nbeam, x.nupchan);
    const int ppt = x.dual ? (x.nbeam / 2 * x.nupchan + nthr - 1) / nthr * 2 : (x.nbeam * x.nupchan + nthr - 1) / nthr;
    const dim3 grid((unsigned)(x.nchan * ((nframe + run - 1) / run))), block((unsigned)nthr);
    const uint8_t* a = (const uint8_t*)in0_dev;
    const uint8_t* b = (const uint8_t*)in1_dev;
    const float2* w = (const float2*)weights_dev;
    float* o = (float*)out_dev;
    switch (x.nupchan) {
    case 8: upchan_launch_pfb<8>(ppt, grid, block, x.stream, a, b, ntime0, w, o, x, nframe, run); break;
    case 16: upchan_launch_pfb<16>(ppt, grid, block, x.stream, a, b, ntime0, w, o, x, nframe, run); break;
    case 32: upchan_launch_pfb<32>(ppt, grid, block, x.stream, a, b, ntime0, w, o, x, nframe, run); break;
    default: upchan_launch_pfb<64>(ppt, grid, block, x.stream, a, b, ntime0, w, o, x, nframe, run); break;
    }
    if ((rc = pfb_after_launch(x, a, ntime0, b))) return rc;
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

static int upchan_initialize(int gpu, int ninput, int nchan, int ntime, int nupchan, int nbeam, int nframe_sum, bool dual) {
    if (ninput <= 0 || ninput % 4 || nchan <= 0 || ntime <= 0 || nbeam <= 0 || nframe_sum < 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: bad sizes ninput=%d nchan=%d ntime=%d nbeam=%d nframe_sum=%d (inputs a multiple of 4)",
                  ninput, nchan, ntime, nbeam, nframe_sum);
    if (nupchan != 8 && nupchan != 16 && nupchan != 32 && nupchan != 64)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: nupchan %d not one of 8, 16, 32, 64", nupchan);
    if (ntime % nupchan) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: ntime %d not a multiple of nupchan %d", ntime, nupchan);
    const int nframe = ntime / nupchan;
    if (nframe_sum > 0 && nframe % nframe_sum)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: nframe_sum %d does not divide the %d frames of a gulp", nframe_sum, nframe);
    if ((long long)nbeam * nupchan > UC_MAXB)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: nbeam %d x nupchan %d above %d", nbeam, nupchan, UC_MAXB);
    if ((long long)nchan * nframe > 0x7FFFFFFFLL || (long long)ninput * nchan > 0x7FFFFFFFLL)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: %d channels x %d inputs x %d frames is more than one launch takes", nchan, ninput, nframe);
    if (dual && (nbeam % 2 || nframe_sum == 0))
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: dual-pol needs an even nbeam (%d) and nframe_sum > 0 (%d)", nbeam, nframe_sum);
    std::lock_guard<std::mutex> lk(g_umu);
    upchan_destroy_locked();
    UpchanContext& x = g_u;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.ninput = ninput; x.nchan = nchan; x.ntime = ntime; x.nupchan = nupchan; x.nbeam = nbeam; x.nframe_sum = nframe_sum;
    x.pfb_row = (size_t)nchan * ninput;
    x.dual = dual;
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengUpchanInitialize(int gpu, int ninput, int nchan, int ntime, int nupchan, int nbeam, int nframe_sum) {
    return upchan_initialize(gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum, false);
}

int xengUpchanInitializeDualPol(int gpu, int ninput, int nchan, int ntime, int nupchan, int nbeam, int nframe_sum) {
    return upchan_initialize(gpu, ninput, nchan, ntime, nupchan, nbeam, nframe_sum, true);
}

// weights_version: the kernel reads the fp32 weights as they are (no prepared copy), so any version means "as they are now"
int xengUpchanRun(const void* in_dev, void* out_dev, const void* weights_dev, long long weights_version) {
    (void)weights_version;
    return upchan_run(in_dev, 0, nullptr, out_dev, weights_dev);
}

int xengUpchanRunParts(const void* in0_dev, int ntime0, const void* in1_dev, void* out_dev, const void* weights_dev, long long weights_version) {
    (void)weights_version;
    if (!in1_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Upchan: null second part");
    return upchan_run(in0_dev, ntime0, in1_dev, out_dev, weights_dev);
}

int xengUpchanSetPfb(int ntap, const float* coeffs) {
    std::unique_lock<std::mutex> lk(g_umu, std::defer_lock);
    return pfb_configure(lk, g_u, "Upchan", ntap, coeffs);
}

int xengUpchanReset(void) {
    std::lock_guard<std::mutex> lk(g_umu);
    UpchanContext& x = g_u;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Upchan: not initialized");
    x.pfb.valid = false;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanMark(unsigned long long* ticket) { return beam_context_mark(g_umu, g_u, "Upchan", ticket); }
int xengUpchanWait(unsigned long long ticket) { return beam_context_wait(g_umu, g_u, "Upchan", ticket); }
int xengUpchanTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_umu, g_u, "Upchan", ticket, done); }
int xengUpchanSync(void) { return beam_context_sync(g_umu, g_u, "Upchan"); }

int xengUpchanDestroy(void) {
    std::lock_guard<std::mutex> lk(g_umu);
    return upchan_destroy_locked();
}

}  // extern "C"
