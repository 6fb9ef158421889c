// Host side of the per-input fine-channel spectra (UpchanSpectra; upchan_spectra_kernels.h): a process-global context of its
// own on the beamformer's stream (BeamStreamContext, xeng_common.h).
#include <mutex>

#include "upchan_pfb.h"
#include "upchan_spectra_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct UpchanSpectraContext : PfbContext {
    int ninput = 0, nchan = 0, nframe_sum = 0;
    int nframe = 0;                     // frames per gulp (F)
    int wf = 0;                         // frames per launch window: min(W, F)
    int gpw = 1;                        // gulps per window (G = W / F when F | W, else 1)
    int pos = 0;                        // gulps of the window in progress already run
    float* acc = nullptr;               // f32[2][nchan][N][ninput]: the window in progress when gpw > 1
};
static std::mutex g_usmu;
static UpchanSpectraContext g_us;

static int upchan_spectra_destroy_locked() {
    if (!g_us.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_us);
    if (g_us.acc) (void)hipFree(g_us.acc);
    g_us.pfb.release();
    g_us = UpchanSpectraContext();
    return XENG_STATUS_SUCCESS;
}

// frame slots per work-group: part of the configuration (it fixes the order of every sum)
static int upchan_spectra_nslot(int nupchan, int wf) {
    int nslot = US_DEFSLOT;
    if (const char* e = diag_env("XENG_SPECTRA_NSLOT")) nslot = atoi(e);          // (diagnostic builds: profiles/upchan_spectra_probe.py)
    if (nslot > us_maxslot(nupchan)) nslot = us_maxslot(nupchan);
    if (nslot > wf) nslot = wf;
    return nslot < 1 ? 1 : nslot;
}

template <int N>
static void upchan_spectra_launch(const UpchanSpectraContext& x, const uint8_t* in0, const uint8_t* in1, int ntime0, float* out, int mode) {
    const int nslot = upchan_spectra_nslot(N, x.wf);
    const int nxb = (x.ninput + US_LANES - 1) / US_LANES;
    const dim3 grid((unsigned)((x.nframe / x.wf) * x.nchan * nxb)), block((unsigned)(US_LANES * nslot));
    if (x.pfb.h)
        hipLaunchKernelGGL((upchan_spectra_kernel<N, UcPfb>), grid, block, 0, x.stream, in0, in1, ntime0, out, x.acc, x.nchan, x.ninput, x.wf, mode,
                           x.pfb.args());
    else
        hipLaunchKernelGGL((upchan_spectra_kernel<N>), grid, block, 0, x.stream, in0, in1, ntime0, out, x.acc, x.nchan, x.ninput, x.wf, mode);
}

static int upchan_spectra_run(const void* in0_dev, int ntime0, const void* in1_dev, void* out_dev) {
    if ((uintptr_t)out_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: output %p not 16-byte aligned", out_dev);
    std::unique_lock<std::mutex> lk(g_usmu, std::defer_lock);
    UpchanSpectraContext& x = g_us;
    int rc = gulp_begin(lk, x, "UpchanSpectra", "", in0_dev, &in1_dev, &ntime0);
    if (rc) return rc;
    if (!out_dev && x.pos == x.gpw - 1)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: null output for a gulp that completes a window (gulp %d of %d)", x.pos + 1, x.gpw);
    XENG_HIP(hipSetDevice(x.gpu));
    const int mode = x.gpw == 1 ? US_OUT : x.pos == x.gpw - 1 ? US_FINISH : x.pos == 0 ? US_ASSIGN : US_ADD;
    const uint8_t* a = (const uint8_t*)in0_dev;
    const uint8_t* b = (const uint8_t*)in1_dev;
    float* out = (float*)out_dev;
    switch (x.nupchan) {
    case 1: upchan_spectra_launch<1>(x, a, b, ntime0, out, mode); break;
    case 2: upchan_spectra_launch<2>(x, a, b, ntime0, out, mode); break;
    case 4: upchan_spectra_launch<4>(x, a, b, ntime0, out, mode); break;
    case 8: upchan_spectra_launch<8>(x, a, b, ntime0, out, mode); break;
    case 16: upchan_spectra_launch<16>(x, a, b, ntime0, out, mode); break;
    case 32: upchan_spectra_launch<32>(x, a, b, ntime0, out, mode); break;
    default: upchan_spectra_launch<64>(x, a, b, ntime0, out, mode); break;
    }
    if ((rc = pfb_after_launch(x, a, ntime0, b))) return rc;
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.pos = (x.pos + 1) % x.gpw;
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengUpchanSpectraInitialize(int gpu, int ninput, int nchan, int ntime, int nupchan, int nframe_sum) {
    if (ninput <= 0 || nchan <= 0 || ntime <= 0 || nframe_sum <= 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: bad sizes ninput=%d nchan=%d ntime=%d nframe_sum=%d", ninput, nchan, ntime, nframe_sum);
    if (nupchan != 1 && nupchan != 2 && nupchan != 4 && nupchan != 8 && nupchan != 16 && nupchan != 32 && nupchan != 64)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: nupchan %d not one of 1, 2, 4, 8, 16, 32, 64", nupchan);
    if (ntime % nupchan) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: ntime %d not a multiple of nupchan %d", ntime, nupchan);
    const int nframe = ntime / nupchan;
    if (nframe % nframe_sum && nframe_sum % nframe)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: nframe_sum %d neither divides nor is a multiple of the %d frames of a gulp", nframe_sum,
                  nframe);
    const int wf = nframe_sum < nframe ? nframe_sum : nframe;
    const long long nxb = ((long long)ninput + US_LANES - 1) / US_LANES;
    if ((size_t)nchan * ninput > US_MAXROW || (long long)(nframe / wf) * nchan * nxb > 0x7FFFFFFFLL || (long long)nchan * nupchan > 0x7FFFFFFFLL)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: %d inputs x %d channels x %d windows is more than one launch takes", ninput, nchan,
                  nframe / wf);
    std::lock_guard<std::mutex> lk(g_usmu);
    upchan_spectra_destroy_locked();
    UpchanSpectraContext& x = g_us;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.ninput = ninput; x.nchan = nchan; x.ntime = ntime; x.nupchan = nupchan; x.nframe_sum = nframe_sum;
    x.nframe = nframe;
    x.wf = wf;
    x.pfb_row = (size_t)nchan * ninput;
    x.gpw = nframe_sum > nframe ? nframe_sum / nframe : 1;
    const size_t nacc = (size_t)2 * nchan * nupchan * ninput;
    if (x.gpw > 1 && hipMalloc(&x.acc, nacc * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        x = UpchanSpectraContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "UpchanSpectra: cannot allocate %.3g MB of window accumulator", (double)nacc * 4e-6);
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSpectraGetInfo(int* gulps_per_window, int* windows_per_gulp, int* pos) {
    if (!gulps_per_window || !windows_per_gulp || !pos) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized");
    *gulps_per_window = x.gpw;
    *windows_per_gulp = x.nframe / x.wf;
    *pos = x.pos;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSpectraRun(const void* in_dev, void* out_dev) {
    return upchan_spectra_run(in_dev, 0, nullptr, out_dev);
}

int xengUpchanSpectraRunParts(const void* in0_dev, int ntime0, const void* in1_dev, void* out_dev) {
    if (!in1_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: null second part");
    return upchan_spectra_run(in0_dev, ntime0, in1_dev, out_dev);
}

int xengUpchanSpectraSetPfb(int ntap, const float* coeffs) {
    std::unique_lock<std::mutex> lk(g_usmu, std::defer_lock);
    return pfb_configure(lk, g_us, "UpchanSpectra", ntap, coeffs);
}

int xengUpchanSpectraPrime(const void* in_dev) {
    return pfb_prime(g_usmu, g_us, "UpchanSpectra", in_dev, 0, nullptr);
}

int xengUpchanSpectraPrimeParts(const void* in0_dev, int ntime0, const void* in1_dev) {
    if (!in1_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraPrime: null second part");
    return pfb_prime(g_usmu, g_us, "UpchanSpectra", in0_dev, ntime0, in1_dev);
}

int xengUpchanSpectraReset(void) {
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized");
    x.pos = 0;                          // (the next gulp assigns the accumulator)
    x.pfb.valid = false;                // (the next gulp's first frames see zeros before it)
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSpectraMark(unsigned long long* ticket) { return beam_context_mark(g_usmu, g_us, "UpchanSpectra", ticket); }
int xengUpchanSpectraWait(unsigned long long ticket) { return beam_context_wait(g_usmu, g_us, "UpchanSpectra", ticket); }
int xengUpchanSpectraTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_usmu, g_us, "UpchanSpectra", ticket, done); }
int xengUpchanSpectraSync(void) { return beam_context_sync(g_usmu, g_us, "UpchanSpectra"); }

int xengUpchanSpectraDestroy(void) {
    std::lock_guard<std::mutex> lk(g_usmu);
    return upchan_spectra_destroy_locked();
}

}  // extern "C"
