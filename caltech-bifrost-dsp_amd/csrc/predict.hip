// Host side of the component subtraction (UpchanPredict; predict_kernels.h): a process-global context of its own on the
// beamformer's stream (BeamStreamContext, xeng_common.h).
#include <cmath>
#include <mutex>
#include <vector>

#include "predict_kernels.h"
#include "xeng_common.h"

namespace xeng {

static_assert(XENG_PREDICT_MAX_NCOMP == PR_MAX_NCOMP && XENG_PREDICT_MAX_NSTAND == PR_MAX_NSTAND, "the limits of include/xeng.h are the kernel's");

struct PredictContext : BeamStreamContext {
    int nstand = 0, nfine = 0, nfavg = 0, ndir = 0, ncomp_max = 0, cross = 0, mode = XENG_PREDICT_SUBTRACT;
    long long nfilled = 0;              // filled records of the list in force
    GuardedState alloc;                 // the state between its guard bands (xengPredictCheckGuards)
    pr_record* rec = nullptr;           // [ngroup][ncomp_max], inside alloc (first: 32-byte records on a 256-byte boundary)
    double* freq = nullptr;             // f64[nfine], behind it
    double* tau = nullptr;              // f64[ndir][nstand]
    int* nrec = nullptr;                // i32[ngroup]: one past the last filled record
    bool geometry = false;

    int ngroup() const { return nfine / nfavg; }
    size_t nrecords() const { return (size_t)ngroup() * ncomp_max; }
    size_t state_bytes() const {
        const size_t n = nrecords() * sizeof(pr_record) + ((size_t)nfine + (size_t)ndir * nstand) * sizeof(double) + (size_t)ngroup() * sizeof(int);
        return (n + 15) & ~(size_t)15;
    }
    int ntile() const { return (nstand + PR_T - 1) / PR_T; }
};
static std::mutex g_prmu;
static PredictContext g_pr;

static int predict_destroy_locked() {
    if (!g_pr.live) return XENG_STATUS_SUCCESS;
    beam_context_close(g_pr);
    g_pr.alloc.free();
    g_pr = PredictContext();
    return XENG_STATUS_SUCCESS;
}

}  // namespace xeng

using namespace xeng;

extern "C" {

int xengPredictInitialize(int gpu, int nstand, int nfine, int nfavg, int ndir, int ncomp_max, int cross) {
    if (nstand <= 0 || nfine <= 0 || nfavg <= 0 || ndir <= 0 || ncomp_max <= 0)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: bad sizes nstand=%d nfine=%d nfavg=%d ndir=%d ncomp_max=%d", nstand, nfine, nfavg, ndir, ncomp_max);
    if (nfine % nfavg) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: nfavg %d does not divide nfine %d", nfavg, nfine);
    if (ncomp_max > XENG_PREDICT_MAX_NCOMP) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: %d components, %d at the most", ncomp_max, XENG_PREDICT_MAX_NCOMP);
    if (nstand > XENG_PREDICT_MAX_NSTAND) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: %d stands, %d at the most", nstand, XENG_PREDICT_MAX_NSTAND);
    if (cross != 0 && cross != 1) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: cross is %d, not 0 or 1", cross);
    if (nfine > 65535 || ndir > (1 << 24) || (double)ndir * nstand * 8.0 > (double)XENG_IMAGE_MAX_STATE_BYTES)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: %d channels x %d directions x %d stands is more than one launch or a table of %.3g GB takes", nfine, ndir,
                  nstand, (double)XENG_IMAGE_MAX_STATE_BYTES * 1e-9);
    std::lock_guard<std::mutex> lk(g_prmu);
    predict_destroy_locked();
    PredictContext& x = g_pr;
    int rc = beam_context_open(x, gpu);
    if (rc) return rc;
    x.nstand = nstand; x.nfine = nfine; x.nfavg = nfavg; x.ndir = ndir; x.ncomp_max = ncomp_max; x.cross = cross;
    // every byte 0xFF: pixel -1 in every record; the tables and nrec behind them stay 0
    if (x.alloc.open(x.state_bytes()) != hipSuccess || hip_memset_now(x.alloc.data(), 0xFF, x.nrecords() * sizeof(pr_record)) != hipSuccess) {
        (void)hipGetLastError();
        x.alloc.free();
        x = PredictContext();
        XENG_FAIL(XENG_STATUS_DEVICE_ERROR, "Predict: cannot allocate %.3g MB of state", ((double)ndir * nstand * 8 + (double)(nfine / nfavg) * ncomp_max * 32) * 1e-6);
    }
    x.rec = (pr_record*)x.alloc.data();
    x.freq = (double*)(x.rec + x.nrecords());
    x.tau = x.freq + nfine;
    x.nrec = (int*)(x.tau + (size_t)ndir * nstand);
    x.live = true;
    return XENG_STATUS_SUCCESS;
}

int xengPredictGetInfo(int* ntile, int* ngroup, int* lds_bytes, long long* span_bytes, long long* state_bytes, long long* nfilled, int* mode) {
    if (!ntile || !ngroup || !lds_bytes || !span_bytes || !state_bytes || !nfilled || !mode) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictGetInfo: null result");
    std::lock_guard<std::mutex> lk(g_prmu);
    PredictContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Predict: not initialized");
    *ntile = x.ntile();
    *ngroup = x.ntile() * (x.ntile() + 1) / 2 * x.nfine;
    *lds_bytes = (int)predict_lds_bytes();
    *span_bytes = (long long)x.nfine * (2LL * x.nstand) * (2LL * x.nstand) * (long long)sizeof(float2);
    *state_bytes = (long long)x.state_bytes();
    *nfilled = x.nfilled;
    *mode = x.mode;
    return XENG_STATUS_SUCCESS;
}

int xengPredictSetGeometry(const double* tau, const double* freq) {
    if (!tau || !freq) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetGeometry: null %s", tau ? "frequencies" : "delays");
    std::lock_guard<std::mutex> lk(g_prmu);
    PredictContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Predict: not initialized (call xengPredictInitialize)");
    for (int c = 0; c < x.nfine; c++)
        if (!std::isfinite(freq[c])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetGeometry: frequency %d is not finite", c);
    for (size_t i = 0; i < (size_t)x.ndir * x.nstand; i++)
        if (!std::isfinite(tau[i])) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetGeometry: delay %zu is not finite", i);
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the tables)
    XENG_HIP(hipMemcpy(x.freq, freq, (size_t)x.nfine * sizeof(double), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.tau, tau, (size_t)x.ndir * x.nstand * sizeof(double), hipMemcpyHostToDevice));
    x.geometry = true;
    return XENG_STATUS_SUCCESS;
}

int xengPredictSetComponents(const void* records) {
    if (!records) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetComponents: null records");
    if ((uintptr_t)records % 4) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetComponents: records %p not 4-byte aligned", records);
    std::lock_guard<std::mutex> lk(g_prmu);
    PredictContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Predict: not initialized (call xengPredictInitialize)");
    // (the caller's buffer need not have the alignment of pr_record: the words are read one by one)
    const int32_t* wi = (const int32_t*)records;
    const float* wf = (const float*)records;
    std::vector<int> nrec((size_t)x.ngroup(), 0);
    long long filled = 0;
    for (int g = 0; g < x.ngroup(); g++)
        for (int k = 0; k < x.ncomp_max; k++) {
            const size_t o = ((size_t)g * x.ncomp_max + k) * 8;
            const int pixel = wi[o];
            if (pixel < -1 || pixel >= x.ndir)
                XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetComponents: record %d of group %d has pixel %d, outside [-1, %d)", k, g, pixel, x.ndir);
            if (pixel < 0) continue;
            for (int e = 0; e < (x.cross ? 4 : 2); e++)
                if (!std::isfinite(wf[o + 2 + e]))
                    XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetComponents: word %d of record %d of group %d is not finite", e, k, g);
            nrec[g] = k + 1;
            filled++;
        }
    XENG_HIP(hipSetDevice(x.gpu));
    XENG_HIP(hipStreamSynchronize(x.stream));   // (launches in flight read the records: they apply to the next Run only)
    XENG_HIP(hipMemcpy(x.rec, records, x.nrecords() * sizeof(pr_record), hipMemcpyHostToDevice));
    XENG_HIP(hipMemcpy(x.nrec, nrec.data(), nrec.size() * sizeof(int), hipMemcpyHostToDevice));
    x.nfilled = filled;
    return XENG_STATUS_SUCCESS;
}

int xengPredictSetMode(int mode) {
    if (mode != XENG_PREDICT_SUBTRACT && mode != XENG_PREDICT_MODEL) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "PredictSetMode: mode %d", mode);
    std::lock_guard<std::mutex> lk(g_prmu);
    PredictContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Predict: not initialized (call xengPredictInitialize)");
    x.mode = mode;                              // (a launch argument: the Runs in flight keep theirs)
    return XENG_STATUS_SUCCESS;
}

int xengPredictRun(const void* vis_dev, void* out_dev) {
    std::lock_guard<std::mutex> lk(g_prmu);
    PredictContext& x = g_pr;
    if (!x.live) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Predict: not initialized (call xengPredictInitialize)");
    const bool model = x.mode == XENG_PREDICT_MODEL;
    if (!out_dev || (!vis_dev && !model)) XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: null %s", !out_dev ? "output" : "input");
    if ((uintptr_t)vis_dev % 16 || (uintptr_t)out_dev % 16)
        XENG_FAIL(XENG_STATUS_INVALID_ARGUMENT, "Predict: input %p or output %p not 16-byte aligned", vis_dev, out_dev);
    if (!x.geometry) XENG_FAIL(XENG_STATUS_INVALID_STATE, "Predict: no geometry (call xengPredictSetGeometry)");
    XENG_HIP(hipSetDevice(x.gpu));
    const int nt = x.ntile();
    const dim3 grid((unsigned)(nt * (nt + 1) / 2), (unsigned)x.nfine);
    if (x.cross)
        hipLaunchKernelGGL(predict_kernel<true>, grid, dim3(PR_THREADS), 0, x.stream, (const float2*)vis_dev, x.freq, x.tau, x.rec, x.nrec, (float2*)out_dev, x.nstand,
                           x.nfavg, x.ncomp_max, model ? 1 : 0);
    else
        hipLaunchKernelGGL(predict_kernel<false>, grid, dim3(PR_THREADS), 0, x.stream, (const float2*)vis_dev, x.freq, x.tau, x.rec, x.nrec, (float2*)out_dev, x.nstand,
                           x.nfavg, x.ncomp_max, model ? 1 : 0);
    stream_tick(STREAM_BEAM);
    XENG_HIP(hipGetLastError());
    return XENG_STATUS_SUCCESS;
}

int xengPredictCheckGuards(int* intact) { return beam_context_check_guards(g_prmu, g_pr, g_pr.alloc, "Predict", intact); }
int xengPredictMark(unsigned long long* ticket) { return beam_context_mark(g_prmu, g_pr, "Predict", ticket); }
int xengPredictWait(unsigned long long ticket) { return beam_context_wait(g_prmu, g_pr, "Predict", ticket); }
int xengPredictTicketDone(unsigned long long ticket, int* done) { return beam_context_ticket_done(g_prmu, g_pr, "Predict", ticket, done); }
int xengPredictSync(void) { return beam_context_sync(g_prmu, g_pr, "Predict"); }

int xengPredictDestroy(void) {
    std::lock_guard<std::mutex> lk(g_prmu);
    return predict_destroy_locked();
}

}  // extern "C"
