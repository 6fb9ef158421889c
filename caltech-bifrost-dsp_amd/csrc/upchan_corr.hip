// Host side of the upchannelised correlator (UpchanCorr; upchan_corr_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <mutex>

#include "upchan_corr_kernels.h"
#include "upchan_pfb.h"
#include "xeng_common.h"

namespace xeng {

struct UpchanCorrContext : PfbContext {
    int ninput = 0, nchan = 0, fine_lo = 0, fine_hi = 0, nstage = 0;
    int nfine = 0, npad = 0, ntile = 0, ntp = 0, nframe = 0, nfp = 0;
    size_t fine_stride = 0;             // float2 per fine channel of the staging buffer: nstage * nfp * npad
    float2* stage = nullptr;            // [nfine][nstage * nfp][npad]
    float* acc = nullptr;               // [nfine][ntp][Re, Im][16][64]
    int staged = 0;                     // gulps staged since the last contraction
    bool fresh = true;                  // nothing contracted since the last dump / reset: the next contraction starts from zero
};
static std::mutex g_ccmu;
static UpchanCorrContext g_cc;

// staging budget of the default depth: up to 8 gulps, within 4 GiB
static constexpr size_t UCC_STAGE_BUDGET = (size_t)4 << 30;
static constexpr int UCC_MAX_STAGE = 8;

static int upchan_corr_destroy_locked() {
    if (!g_cc.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_cc);
    if (g_cc.stage) (void)hipFree(g_cc.stage);
    if (g_cc.acc) (void)hipFree(g_cc.acc);
    g_cc.pfb.release();
    g_cc = UpchanCorrContext();
    return XENG_STATUS_SUCCESS;
}

// the staged gulps into the accumulator, in frame order
static int upchan_corr_contract_locked(UpchanCorrContext& x) {
    if (!x.staged) return XENG_STATUS_SUCCESS;
    const long long items = (long long)x.nfine * x.ntp;
    const dim3 grid((unsigned)((items + UCC_WPB - 1) / UCC_WPB)), block(64 * UCC_WPB);
    hipLaunchKernelGGL(upchan_corr_mfma_kernel, grid, block, 0, x.stream, x.stage, x.acc, x.nfine, x.ntp, x.npad, x.fine_stride,
                       x.staged, x.nfp, (int)x.fresh);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.staged = 0;
    x.fresh = false;
    return XENG_STATUS_SUCCESS;
}

template <int N>
static void upchan_corr_stage_n(dim3 grid, const UpchanCorrContext& x, const uint8_t* in0, const uint8_t* in1, int ntime0, int c_lo) {
    if (x.pfb.h)
        hipLaunchKernelGGL((upchan_corr_stage_kernel<N, UcPfb>), grid, dim3(UCC_SB), 0, x.stream, in0, in1, ntime0, x.stage, x.nchan, x.ninput, x.npad,
                           x.nframe, x.nfp, x.fine_stride, x.staged * x.nfp, x.fine_lo, x.fine_hi, c_lo, x.pfb.args());
    else
        hipLaunchKernelGGL((upchan_corr_stage_kernel<N>), grid, dim3(UCC_SB), 0, x.stream, in0, in1, ntime0, x.stage, x.nchan, x.ninput, x.npad,
                           x.nframe, x.nfp, x.fine_stride, x.staged * x.nfp, x.fine_lo, x.fine_hi, c_lo);
}

static int upchan_corr_accumulate(const void* in0_dev, int ntime0, const void* in1_dev) {
    std::unique_lock<std::mutex> lk(g_ccmu, std::defer_lock);
    UpchanCorrContext& x = g_cc;
    int rc = gulp_begin(lk, x, "UpchanCorr", "", in0_dev, &in1_dev, &ntime0);
    if (rc) return rc;
    XENG_HIP(hipSetDevice(x.gpu));
    const int c_lo = x.fine_lo / x.nupchan, c_hi = (x.fine_hi - 1) / x.nupchan + 1;
    const int nxb = (x.npad + UCC_SB - 1) / UCC_SB;
    const dim3 grid((unsigned)(nxb * x.nfp * (c_hi - c_lo)));
    const uint8_t* a = (const uint8_t*)in0_dev;
    const uint8_t* b = (const uint8_t*)in1_dev;
    switch (x.nupchan) {
    case 1: upchan_corr_stage_n<1>(grid, x, a, b, ntime0, c_lo); break;
    case 2: upchan_corr_stage_n<2>(grid, x, a, b, ntime0, c_lo); break;
    case 4: upchan_corr_stage_n<4>(grid, x, a, b, ntime0, c_lo); break;
    case 8: upchan_corr_stage_n<8>(grid, x, a, b, ntime0, c_lo); break;
    case 16: upchan_corr_stage_n<16>(grid, x, a, b, ntime0, c_lo); break;
    case 32: upchan_corr_stage_n<32>(grid, x, a, b, ntime0, c_lo); break;
    default: upchan_corr_stage_n<64>(grid, x, a, b, ntime0, c_lo); break;
    }
    if ((rc = pfb_after_launch(x, a, ntime0, b))) return rc;
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    if (++x.staged == x.nstage) return upchan_corr_contract_locked(x);
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengUpchanCorrInitialize(int gpu, int ninput, int nchan, int ntime, int nupchan, int fine_lo, int fine_hi, int nstage) {
    if (ninput <= 0 || nchan <= 0 || ntime <= 0 || nstage < 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: bad sizes ninput=%d nchan=%d ntime=%d nstage=%d", ninput, nchan, ntime, nstage);
    if (nupchan != 1 && nupchan != 2 && nupchan != 4 && nupchan != 8 && nupchan != 16 && nupchan != 32 && nupchan != 64)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: nupchan %d not one of 1, 2, 4, 8, 16, 32, 64", nupchan);
    if (ntime % nupchan) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: ntime %d not a multiple of nupchan %d", ntime, nupchan);
    if ((long long)nchan * nupchan > 0x7FFFFFFFLL || fine_lo < 0 || fine_hi <= fine_lo || (long long)fine_hi > (long long)nchan * nupchan)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: fine channels [%d, %d) not a non-empty range within [0, %lld)", fine_lo, fine_hi,
                  (long long)nchan * nupchan);
    const int npad = (int)(((long long)ninput + UCC_T - 1) / UCC_T * UCC_T);
    const long long ntile = npad / UCC_T, ntp = ntile * (ntile + 1) / 2, nfine = fine_hi - fine_lo;
    const int nframe = ntime / nupchan, nfp = nframe + (nframe & 1);
    const size_t gulp_stage = (size_t)nfine * nfp * npad * 8;
    if (nstage == 0) {
        const size_t fit = UCC_STAGE_BUDGET / gulp_stage;
        nstage = fit < 1 ? 1 : fit > (size_t)UCC_MAX_STAGE ? UCC_MAX_STAGE : (int)fit;
    }
    if (ninput > (1 << 20) || nstage > 1024 || (long long)nstage * nfp > (1LL << 24) || nfine * ntp > 0x7FFFFFFFLL ||
        nfine * ntile * ntile > 0x7FFFFFFFLL || (long long)((npad + UCC_SB - 1) / UCC_SB) * nfp * nchan > 0x7FFFFFFFLL)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: %d inputs x %lld fine channels x %d frames x %d gulps is more than one launch takes",
                  ninput, nfine, nframe, nstage);
    std::lock_guard<std::mutex> lk(g_ccmu);
    upchan_corr_destroy_locked();
    UpchanCorrContext& x = g_cc;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.ninput = ninput; x.nchan = nchan; x.ntime = ntime; x.nupchan = nupchan; x.fine_lo = fine_lo; x.fine_hi = fine_hi; x.nstage = nstage;
    x.nfine = (int)nfine; x.npad = npad; x.ntile = (int)ntile; x.ntp = (int)ntp; x.nframe = nframe; x.nfp = nfp;
    x.fine_stride = (size_t)nstage * nfp * npad;
    x.pfb_row = (size_t)nchan * ninput;
    if (hipMalloc(&x.stage, (size_t)nfine * x.fine_stride * sizeof(float2)) != hipSuccess ||
        hipMalloc(&x.acc, (size_t)nfine * ntp * 2048 * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        if (x.stage) (void)hipFree(x.stage);
        x = UpchanCorrContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "UpchanCorr: cannot allocate %.3g GB of staging and %.3g GB of accumulators",
                  (double)nfine * nstage * nfp * npad * 8 * 1e-9, (double)nfine * ntp * 8192 * 1e-9);
    }
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanCorrGetInfo(int* nfine, int* nstage) {
    if (!nfine || !nstage) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorrGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_ccmu);
    UpchanCorrContext& x = g_cc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanCorr: not initialized");
    *nfine = x.nfine;
    *nstage = x.nstage;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanCorrAccumulate(const void* in_dev) {
    return upchan_corr_accumulate(in_dev, 0, nullptr);
}

int xengUpchanCorrAccumulateParts(const void* in0_dev, int ntime0, const void* in1_dev) {
    if (!in1_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: null second part");
    return upchan_corr_accumulate(in0_dev, ntime0, in1_dev);
}

int xengUpchanCorrDump(void* out_dev) {
    if (!out_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: null output");
    if ((uintptr_t)out_dev % 16) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorr: output %p not 16-byte aligned", out_dev);
    std::lock_guard<std::mutex> lk(g_ccmu);
    UpchanCorrContext& x = g_cc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanCorr: not initialized (call xengUpchanCorrInitialize)");
    XENG_HIP(hipSetDevice(x.gpu));
    int rc = upchan_corr_contract_locked(x);
    if (rc) return rc;
    const dim3 grid((unsigned)((long long)x.nfine * x.ntile * x.ntile)), block(256);
    hipLaunchKernelGGL(upchan_corr_dump_kernel, grid, block, 0, x.stream, x.acc, (float2*)out_dev, x.ninput, x.ntile, x.ntp, (int)x.fresh);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    x.fresh = true;
    return XENG_STATUS_SUCCESS;
}

int xengUpchanCorrReset(void) {
    std::lock_guard<std::mutex> lk(g_ccmu);
    UpchanCorrContext& x = g_cc;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "UpchanCorr: not initialized");
    x.staged = 0;                       // (staged frames are overwritten by the next gulps; the next contraction starts from zero)
    x.fresh = true;
    x.pfb.valid = false;                // (the next gulp's first frames see zeros before it)
    return XENG_STATUS_SUCCESS;
}

int xengUpchanCorrSetPfb(int ntap, const float* coeffs) {
    std::unique_lock<std::mutex> lk(g_ccmu, std::defer_lock);
    return pfb_configure(lk, g_cc, "UpchanCorr", ntap, coeffs);
}

int xengUpchanCorrPrime(const void* in_dev) {
    return pfb_prime(g_ccmu, g_cc, "UpchanCorr", in_dev, 0, nullptr);
}

int xengUpchanCorrPrimeParts(const void* in0_dev, int ntime0, const void* in1_dev) {
    if (!in1_dev) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "UpchanCorrPrime: null second part");
    return pfb_prime(g_ccmu, g_cc, "UpchanCorr", in0_dev, ntime0, in1_dev);
}

int xengUpchanCorrMark(unsigned long long* ticket) { return beam_context_mark(g_ccmu, g_cc, "UpchanCorr", ticket); }
int xengUpchanCorrWait(unsigned long long ticket) { return beam_context_wait(g_ccmu, g_cc, "UpchanCorr", ticket); }
int xengUpchanCorrTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_ccmu, g_cc, "UpchanCorr", ticket, done); }
int xengUpchanCorrSync(void) { return beam_context_sync(g_ccmu, g_cc, "UpchanCorr"); }

int xengUpchanCorrDestroy(void) {
    std::lock_guard<std::mutex> lk(g_ccmu);
    return upchan_corr_destroy_locked();
}

}  // extern "C"
