// Runs peel_steer_kernel, peel_solve_kernel and peel_subtract_kernel of csrc/peel_kernels.h on host threads, one work-group after
// another, the way peel.hip launches them.  The LDS starts as NaN before every work-group: nothing may depend on what it held.  Every
// buffer is a heap block of its exact size, so the address sanitizer this is built with sees any access outside it; the outputs start
// as a pattern no result has, so a word nobody wrote shows.  peel_kernels_host.h is that header with its vector typedefs and its two
// LDS lines replaced (the test writes it).
#include "peel_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar, g_wbar[4];
uint8_t *g_lds, *g_lds2;
float g_slot[256], g_a[256], g_b[256];
using namespace xeng;
// args: nstand nfine ndir niter tol refant passes in.bin out.bin ; in: vis cf32, freq f64, tau f64, flux f32, w f32 ; out: out cf32, gains, stats
// The solve runs `passes` times: the first cold, the later ones warm from the keep the one before left; then the subtraction.
int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int nstand = atoi(argv[1]), nfine = atoi(argv[2]), ndir = atoi(argv[3]), niter = atoi(argv[4]), refant = atoi(argv[6]), passes = atoi(argv[7]);
    const float tol = (float)atof(argv[5]);
    const size_t nin = 2 * (size_t)nstand, nv = nfine * nin * nin, na = (size_t)nfine * ndir * nstand, ng = 2 * na;
    float2* vis = (float2*)aligned_alloc(16, nv * 8);
    float2* out = (float2*)aligned_alloc(16, nv * 8);
    double* freq = (double*)malloc(nfine * 8);
    double* tau = (double*)malloc((size_t)ndir * nstand * 8);
    float* flux = (float*)malloc((size_t)nfine * ndir * 4);
    float* w = (float*)malloc(nstand * 4);
    float2* a = (float2*)malloc(na * 8);
    float2* gains = (float2*)malloc(ng * 8);
    float* stats = (float*)malloc((size_t)nfine * 8 * 4);
    float2* keep_g = (float2*)malloc(ng * 8);
    int* keep_ok = (int*)calloc((size_t)nfine * 2, 4);
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(vis, 8, nv, f) != nv || fread(freq, 8, nfine, f) != (size_t)nfine || fread(tau, 8, (size_t)ndir * nstand, f) != (size_t)ndir * nstand ||
        fread(flux, 4, (size_t)nfine * ndir, f) != (size_t)nfine * ndir || fread(w, 4, nstand, f) != (size_t)nstand) return 2;
    fclose(f);
    memset(keep_g, 0xFF, ng * 8);           // NaN: a cold start must not read it
    memset(a, 0xFF, na * 8);                // NaN: every word the kernels read must have been written by the steering kernel
    for (size_t i = 0; i < nv; i++) out[i] = make_float2(-777.f, -777.f);
    for (int by = 0; by < nfine; by++)
        for (int bx = 0; bx * PL_STEER_THREADS < ndir * nstand; bx++)
            for (int t = 0; t < PL_STEER_THREADS; t++) {
                threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                peel_steer_kernel(freq, tau, a, nstand, ndir);
            }
    const size_t nlds = peel_lds_bytes(nstand);
    for (int k = 0; k < 4; k++) pthread_barrier_init(&g_wbar[k], nullptr, 64);
    pthread_barrier_init(&g_bar, nullptr, PL_THREADS);
    for (int pass = 0; pass < passes; pass++) {
        for (size_t i = 0; i < ng; i++) gains[i] = make_float2(-777.f, -777.f);
        for (int bx = 0; bx < nfine; bx++)
            for (int by = 0; by < 2; by++) {
                uint8_t* lds = (uint8_t*)aligned_alloc(16, (nlds + 15) / 16 * 16);
                memset(lds, 0xFF, nlds);    // NaN: whatever was there must not matter
                g_lds = lds;
                std::vector<std::thread> th;
                for (int t = 0; t < PL_THREADS; t++) th.emplace_back([&, t, bx, by] {
                    threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                    peel_solve_kernel(vis, a, flux, w, gains, stats, keep_g, keep_ok, nstand, ndir, niter, tol, refant, pass > 0);
                });
                for (auto& t : th) t.join();
                free(lds);
            }
    }
    pthread_barrier_destroy(&g_bar);
    pthread_barrier_init(&g_bar, nullptr, PS_THREADS);
    const size_t nlds2 = peel_subtract_lds_bytes();
    const int ntile = (nstand + PS_T - 1) / PS_T;
    for (int by = 0; by < nfine; by++)
        for (int bx = 0; bx < ntile * (ntile + 1) / 2; bx++) {
            uint8_t* lds = (uint8_t*)aligned_alloc(16, nlds2);
            memset(lds, 0xFF, nlds2);
            g_lds2 = lds;
            std::vector<std::thread> th;
            for (int t = 0; t < PS_THREADS; t++) th.emplace_back([&, t, bx, by] {
                threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                peel_subtract_kernel(vis, a, flux, gains, out, nstand, ndir);
            });
            for (auto& t : th) t.join();
            free(lds);
        }
    f = fopen(argv[9], "wb");
    fwrite(out, 8, nv, f);
    fwrite(gains, 8, ng, f);
    fwrite(stats, 4, (size_t)nfine * 8, f);
    fclose(f);
    free(vis); free(out); free(freq); free(tau); free(flux); free(w); free(a); free(gains); free(stats); free(keep_g); free(keep_ok);
    return 0;
}
