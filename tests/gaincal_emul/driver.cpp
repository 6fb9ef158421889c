// Runs gaincal_kernel of csrc/gaincal_kernels.h on host threads, one work-group after another, the way gaincal.hip launches it.  The
// dynamic LDS starts as NaN before every work-group: nothing may depend on what it held.  Every buffer is a heap block of its exact
// size, so the address sanitizer this is built with sees any access outside it.  gaincal_kernels_host.h is that header with its
// vector typedef and its one `extern __shared__` line replaced (the test writes it).
#include "gaincal_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar, g_wbar[4];
uint8_t* g_lds;
float g_slot[256], g_a[256], g_b[256];
using namespace xeng;
// args: nstand nfine nsrc niter tol refant passes in.bin out.bin ; in: vis cf32, freq f64, tau f64, flux f32, w f32 ; out: gains, stats
// The grid runs `passes` times: the first cold, the later ones warm from the keep the one before left.
int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int nstand = atoi(argv[1]), nfine = atoi(argv[2]), nsrc = atoi(argv[3]), niter = atoi(argv[4]), refant = atoi(argv[6]), passes = atoi(argv[7]);
    const float tol = (float)atof(argv[5]);
    const size_t nin = 2 * (size_t)nstand, ng = (size_t)nfine * 2 * nstand;
    float2* vis = (float2*)malloc(nfine * nin * nin * 8);
    double* freq = (double*)malloc(nfine * 8);
    double* tau = (double*)malloc((size_t)nsrc * nstand * 8);
    float* flux = (float*)malloc((size_t)nfine * nsrc * 4);
    float* w = (float*)malloc(nstand * 4);
    float2* gains = (float2*)malloc(ng * 8);
    float* stats = (float*)malloc((size_t)nfine * 8 * 4);
    float2* keep_g = (float2*)malloc(ng * 8);
    int* keep_ok = (int*)calloc((size_t)nfine * 2, 4);
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(vis, 8, nfine * nin * nin, f) != nfine * nin * nin || fread(freq, 8, nfine, f) != (size_t)nfine ||
        fread(tau, 8, (size_t)nsrc * nstand, f) != (size_t)nsrc * nstand || fread(flux, 4, (size_t)nfine * nsrc, f) != (size_t)nfine * nsrc ||
        fread(w, 4, nstand, f) != (size_t)nstand) return 2;
    fclose(f);
    memset(keep_g, 0xFF, ng * 8);           // NaN: a cold start must not read it
    const size_t nlds = gaincal_lds_bytes(nstand);
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (int k = 0; k < 4; k++) pthread_barrier_init(&g_wbar[k], nullptr, 64);
    for (int pass = 0; pass < passes; pass++) {
        for (size_t i = 0; i < ng; i++) gains[i] = make_float2(-777.f, -777.f);
        for (int bx = 0; bx < nfine; bx++)
            for (int by = 0; by < 2; by++) {
                uint8_t* lds = (uint8_t*)malloc(nlds);
                memset(lds, 0xFF, nlds);    // NaN: whatever was there must not matter
                g_lds = lds;
                std::vector<std::thread> th;
                for (int t = 0; t < 256; t++) th.emplace_back([&, t, bx, by] {
                    threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                    gaincal_kernel(vis, freq, tau, flux, w, gains, stats, keep_g, keep_ok, nstand, nsrc, niter, tol, refant, pass > 0);
                });
                for (auto& t : th) t.join();
                free(lds);
            }
    }
    f = fopen(argv[9], "wb");
    fwrite(gains, 8, ng, f);
    fwrite(stats, 4, (size_t)nfine * 8, f);
    fclose(f);
    free(vis); free(freq); free(tau); free(flux); free(w); free(gains); free(stats); free(keep_g); free(keep_ok);
    return 0;
}
