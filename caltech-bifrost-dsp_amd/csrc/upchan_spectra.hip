// Host side of the per-input fine-channel spectra (UpchanSpectra; upchan_spectra_kernels.h): a process-global context of its
// own, beside the Beamform, Upchan, UpchanCorr and UpchanSumBeams contexts, whose kernel runs on the beamformer's stream
// (STREAM_BEAM) and ticks its clock, so that rings declared 'beam' and their span stamps cover it unchanged.
#include <mutex>

#include "upchan_pfb.h"
#include "upchan_spectra_kernels.h"
#include "xeng_common.h"

namespace xeng {

struct UpchanSpectraContext {
    bool live = false;
    int gpu = 0, ninput = 0, nchan = 0, ntime = 0, nupchan = 0, nframe_sum = 0;
    int nframe = 0;                     // frames per gulp (F)
    int wf = 0;                         // frames per launch window: min(W, F)
    int gpw = 1;                        // gulps per window (G = W / F when F | W, else 1)
    int pos = 0;                        // gulps of the window in progress already run
    float* acc = nullptr;               // f32[2][nchan][N][ninput]: the window in progress when gpw > 1
    PfbState pfb;                       // xengUpchanSpectraSetPfb (ntap 1 without coefficients: the plain FFT)
    hipStream_t stream = nullptr;
    TicketRing tickets;                 // xengUpchanSpectraMark / Wait / TicketDone
};
static std::mutex g_usmu;
static UpchanSpectraContext g_us;

static int upchan_spectra_destroy_locked() {
    if (!g_us.live) return XENG_STATUS_SUCCESS;
    (void)hipSetDevice(g_us.gpu);
    if (g_us.stream) (void)hipStreamSynchronize(g_us.stream);
    stream_clocks_forget(g_us.gpu, STREAM_BEAM);         // (the mark events lent to the stream clock go away below)
    g_us.tickets.destroy();
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

// Every argument is checked before the context is looked at where it can be (a bad call is told apart from a missing
// context, and nothing is launched); what depends on the context's state is checked right after.
static int upchan_spectra_run(const void* in0_dev, int ntime0, const void* in1_dev, void* out_dev) {
    if (!in0_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: null input");
    if (in1_dev && ntime0 <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: first part of %d samples", ntime0);
    if ((uintptr_t)out_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: output %p not 16-byte aligned", out_dev);
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized (call xengUpchanSpectraInitialize)");
    if (!out_dev && x.pos == x.gpw - 1)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectra: null output for a gulp that completes a window (gulp %d of %d)", x.pos + 1, x.gpw);
    int rc = gulp_parts("UpchanSpectra", in0_dev, &in1_dev, &ntime0, x.ntime, x.nupchan);
    if (rc) return rc;
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
    if (x.pfb.hist) {                   // the history for the next gulp, before the tick: the input span's stamp covers the copies
        XENG_HIP(hipGetLastError());
        if ((rc = pfb_refresh(x.pfb, x.stream, a, ntime0, b, x.ntime, x.nupchan, (size_t)x.nchan * x.ninput))) return rc;
    }
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.pos = (x.pos + 1) % x.gpw;
    return XENG_STATUS_SUCCESS;
}

// xengUpchanSpectraPrime[Parts]: the history from this gulp's tail, nothing summed
static int upchan_spectra_prime(const void* in0_dev, int ntime0, const void* in1_dev) {
    if (!in0_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraPrime: null input");
    if (in1_dev && ntime0 <= 0) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraPrime: first part of %d samples", ntime0);
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized (call xengUpchanSpectraInitialize)");
    int rc = gulp_parts("UpchanSpectraPrime", in0_dev, &in1_dev, &ntime0, x.ntime, x.nupchan);
    if (rc || !x.pfb.hist) return rc;   // (no history without taps before the frame's own)
    XENG_HIP(hipSetDevice(x.gpu));
    if ((rc = pfb_refresh(x.pfb, x.stream, (const uint8_t*)in0_dev, ntime0, (const uint8_t*)in1_dev, x.ntime, x.nupchan, (size_t)x.nchan * x.ninput)))
        return rc;
    stream_tick(STREAM_BEAM);
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
    x.gpu = gpu < 0 ? 0 : gpu;
    XENG_HIP(hipSetDevice(x.gpu));
    int rc = get_stream(STREAM_BEAM, &x.stream);
    if (rc) return rc;
    x.ninput = ninput; x.nchan = nchan; x.ntime = ntime; x.nupchan = nupchan; x.nframe_sum = nframe_sum;
    x.nframe = nframe;
    x.wf = wf;
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
    int rc = pfb_check_args("UpchanSpectraSetPfb", ntap, coeffs);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized (call xengUpchanSpectraInitialize)");
    if ((rc = pfb_check_sizes("UpchanSpectraSetPfb", ntap, coeffs, x.nupchan, x.ntime))) return rc;
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the coefficients and the history)
    return pfb_set("UpchanSpectraSetPfb", x.pfb, ntap, coeffs, x.nupchan, (size_t)x.nchan * x.ninput);
}

int xengUpchanSpectraPrime(const void* in_dev) {
    return upchan_spectra_prime(in_dev, 0, nullptr);
}

int xengUpchanSpectraPrimeParts(const void* in0_dev, int ntime0, const void* in1_dev) {
    if (!in1_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraPrime: null second part");
    return upchan_spectra_prime(in0_dev, ntime0, in1_dev);
}

int xengUpchanSpectraReset(void) {
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized");
    x.pos = 0;                          // (the next gulp assigns the accumulator)
    x.pfb.valid = false;                // (the next gulp's first frames see zeros before it)
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSpectraMark(unsigned long long* ticket) {
    if (!ticket) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraMark: null ticket");
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized");
    XENG_HIP(hipSetDevice(x.gpu));
    return x.tickets.mark(x.stream, STREAM_BEAM, ticket);
}

int xengUpchanSpectraWait(unsigned long long ticket) {
    hipEvent_t ev = nullptr;
    int gpu = 0;
    {
        std::lock_guard<std::mutex> lk(g_usmu);
        UpchanSpectraContext& x = g_us;
        if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized");
        if (!(ev = x.tickets.find(ticket))) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraWait: unknown ticket %llu", ticket);
        gpu = x.gpu;
    }
    XENG_HIP(hipSetDevice(gpu));
    XENG_HIP(hipEventSynchronize(ev));          // (outside the lock)
    return XENG_STATUS_SUCCESS;
}

int xengUpchanSpectraTicketDone(unsigned long long ticket, int* done) {
    if (!done) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraTicketDone: null result");
    std::lock_guard<std::mutex> lk(g_usmu);
    UpchanSpectraContext& x = g_us;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanSpectra: not initialized");
    const hipEvent_t ev = x.tickets.find(ticket);
    if (!ev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanSpectraTicketDone: unknown ticket %llu", ticket);
    XENG_HIP(hipSetDevice(x.gpu));
    return TicketRing::query(ev, done);
}

int xengUpchanSpectraSync(void) {
    std::lock_guard<std::mutex> lk(g_usmu);
    return context_sync("UpchanSpectra", g_us.live, g_us.gpu, g_us.stream);
}

int xengUpchanSpectraDestroy(void) {
    std::lock_guard<std::mutex> lk(g_usmu);
    return upchan_spectra_destroy_locked();
}

}  // extern "C"
