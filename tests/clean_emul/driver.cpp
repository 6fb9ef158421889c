// Runs clean_step_kernel of csrc/clean_kernels.h on host threads, one work-group after another and one launch after another, the way
// clean.hip enqueues them: steps 0 .. niter on (ntile, ngroup) work-groups, step niter + 1 on (1, ngroup).  The dynamic LDS starts as
// NaN before every work-group: nothing may depend on what it held.  Every buffer is a heap block of its exact size, so the address
// sanitizer this is built with sees any access outside it; the output and the hand-over buffers start as a pattern no result has, so a
// word nobody wrote shows.  clean_kernels_host.h is that header with its one `extern __shared__` line replaced (the test writes it).
#include "clean_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
dim3e gridDim;
pthread_barrier_t g_bar;
uint8_t* g_lds;
using namespace xeng;
// args: nstand nfine nfavg npix autos niter gain threshold fraction norm dsum in.bin out.bin
// in: image f32[ngroup][4][npix], freq f64[nfine], tau f64[npix][nstand], w f32[nstand], mask u8[npix]; out: the span of one Run
int main(int argc, char** argv) {
    if (argc != 14) return 2;
    const int nstand = atoi(argv[1]), nfine = atoi(argv[2]), nfavg = atoi(argv[3]), npix = atoi(argv[4]), niter = atoi(argv[6]);
    const float gain = (float)atof(argv[7]), threshold = (float)atof(argv[8]), fraction = (float)atof(argv[9]);
    const float norm = (float)atof(argv[10]), dsum = (float)atof(argv[11]);
    const int ng = nfine / nfavg, ntile = (npix + CLN_PX - 1) / CLN_PX;
    const size_t nimg = (size_t)ng * 4 * npix, ncomp = (size_t)ng * niter * CLN_REC, nrec = (size_t)2 * ng * ntile * CLN_REC;
    float* img = (float*)malloc(nimg * 4);
    double* freq = (double*)malloc(nfine * 8);
    double* tau = (double*)malloc((size_t)npix * nstand * 8);
    double* tauT = (double*)malloc((size_t)npix * nstand * 8);
    float* w = (float*)malloc(nstand * 4);
    uint8_t* mask = (uint8_t*)malloc(npix);
    float* res = (float*)malloc(nimg * 4);
    int* comp = (int*)malloc(ncomp * 4 + 4);     // (niter = 0: a block of its own all the same)
    int* stats = (int*)malloc((size_t)ng * 16);
    int* rec = (int*)malloc(nrec * 4);
    int* gstate = (int*)malloc((size_t)2 * ng * 16);
    FILE* f = fopen(argv[12], "rb");
    if (!f || fread(img, 4, nimg, f) != nimg || fread(freq, 8, nfine, f) != (size_t)nfine || fread(tau, 8, (size_t)npix * nstand, f) != (size_t)npix * nstand ||
        fread(w, 4, nstand, f) != (size_t)nstand || fread(mask, 1, npix, f) != (size_t)npix) return 2;
    fclose(f);
    for (int p = 0; p < npix; p++)
        for (int s = 0; s < nstand; s++) tauT[(size_t)s * npix + p] = tau[(size_t)p * nstand + s];
    for (size_t i = 0; i < nimg; i++) res[i] = -777.f;
    memset(comp, 0x5A, ncomp * 4);
    memset(stats, 0x5A, (size_t)ng * 16);
    memset(rec, 0x5A, nrec * 4);
    memset(gstate, 0x5A, (size_t)2 * ng * 16);
    const size_t nlds = clean_lds_bytes(nstand);
    pthread_barrier_init(&g_bar, nullptr, CLN_PX);
    for (int step = 0; step <= niter + 1; step++) {
        gridDim.x = step <= niter ? ntile : 1;
        gridDim.y = ng;
        for (int by = 0; by < gridDim.y; by++)
            for (int bx = 0; bx < gridDim.x; bx++) {
                uint8_t* lds = (uint8_t*)aligned_alloc(16, (nlds + 15) / 16 * 16);
                memset(lds, 0xFF, nlds);        // NaN: whatever was there must not matter
                g_lds = lds;
                std::vector<std::thread> th;
                for (int t = 0; t < CLN_PX; t++) th.emplace_back([&, t, bx, by] {
                    threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                    clean_step_kernel(img, res, comp, stats, freq, tauT, w, mask, rec, gstate, nstand, npix, ntile, nfavg, niter, step, gain, threshold,
                                      fraction, norm, dsum);
                });
                for (auto& t : th) t.join();
                free(lds);
            }
    }
    f = fopen(argv[13], "wb");
    fwrite(res, 4, nimg, f);
    fwrite(comp, 4, ncomp, f);
    fwrite(stats, 4, (size_t)ng * 4, f);
    fclose(f);
    free(img); free(freq); free(tau); free(tauT); free(w); free(mask); free(res); free(comp); free(stats); free(rec); free(gstate);
    return 0;
}
