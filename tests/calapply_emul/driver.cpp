// Runs calapply_steer_kernel and calapply_kernel of csrc/calapply_kernels.h on host threads, one work-group after another, the way
// calapply.hip launches them.  The LDS starts as NaN before every work-group: nothing may depend on what it held.  Every buffer is a
// heap block of its exact size, so the address sanitizer this is built with sees any access outside it; the output starts as a
// pattern no result has, so a word nobody wrote shows.  calapply_kernels_host.h is that header with its vector typedef and its one
// `__shared__` line replaced (the test writes it).
#include "calapply_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar;
uint8_t* g_lds;
float g_a[64], g_b[64];
using namespace xeng;
// args: nstand nfine nsrc in.bin out.bin ; in: vis cf32, freq f64, tau f64, flux f32, h cf32[nfine][2][nstand] ; out: cf32 in vis's layout
int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int nstand = atoi(argv[1]), nfine = atoi(argv[2]), nsrc = atoi(argv[3]);
    const size_t nin = 2 * (size_t)nstand, nv = nfine * nin * nin, na = (size_t)nfine * nsrc * nstand, nh = (size_t)nfine * 2 * nstand;
    float2* vis = (float2*)aligned_alloc(16, nv * 8);
    double* freq = (double*)malloc(nfine * 8);
    double* tau = (double*)malloc((size_t)nsrc * nstand * 8 + 8);
    float* flux = (float*)malloc((size_t)nfine * nsrc * 4 + 4);
    float2* hf = (float2*)malloc(nh * 8);
    float2* a = (float2*)malloc(na * 8 + 8);
    float2* out = (float2*)aligned_alloc(16, nv * 8);
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(vis, 8, nv, f) != nv || fread(freq, 8, nfine, f) != (size_t)nfine || fread(tau, 8, (size_t)nsrc * nstand, f) != (size_t)nsrc * nstand ||
        fread(flux, 4, (size_t)nfine * nsrc, f) != (size_t)nfine * nsrc || fread(hf, 8, nh, f) != nh) return 2;
    fclose(f);
    for (size_t i = 0; i < nv; i++) out[i] = make_float2(-777.f, -777.f);
    memset(a, 0xFF, na * 8);                // NaN: every word the kernel reads must have been written by the steering kernel
    if (nsrc > 0)
        for (int by = 0; by < nfine; by++)
            for (int bx = 0; bx * CA_STEER_THREADS < nsrc * nstand; bx++)
                for (int t = 0; t < CA_STEER_THREADS; t++) {
                    threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                    calapply_steer_kernel(freq, tau, a, nstand, nsrc);
                }
    const size_t nlds = calapply_lds_bytes();
    const int ntile = (nstand + CA_T - 1) / CA_T;
    pthread_barrier_init(&g_bar, nullptr, CA_THREADS);
    for (int by = 0; by < nfine; by++)
        for (int bx = 0; bx < ntile * (ntile + 1) / 2; bx++) {
            uint8_t* lds = (uint8_t*)aligned_alloc(16, nlds);
            memset(lds, 0xFF, nlds);        // NaN: whatever was there must not matter
            g_lds = lds;
            std::vector<std::thread> th;
            for (int t = 0; t < CA_THREADS; t++) th.emplace_back([&, t, bx, by] {
                threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                calapply_kernel(vis, a, flux, hf, out, nstand, nsrc);
            });
            for (auto& t : th) t.join();
            free(lds);
        }
    f = fopen(argv[5], "wb");
    fwrite(out, 8, nv, f);
    fclose(f);
    free(vis); free(freq); free(tau); free(flux); free(hf); free(a); free(out);
    return 0;
}
