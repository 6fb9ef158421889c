// Runs image_kernel of csrc/image_kernels.h on host threads, one work-group after another, the way image.hip launches it.  The
// dynamic LDS starts as NaN before every work-group: nothing may depend on what it held.  Every buffer is a heap block of its exact
// size, so the address sanitizer this is built with sees any access outside it.  image_kernels_host.h is that header with its
// vector typedef and its one `extern __shared__` line replaced (the test writes it).
#include "image_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar, g_wbar[4];
uint8_t* g_lds;
float g_slot[256], g_a[256], g_b[256];
using namespace xeng;
// args: nstand nfine nfavg npix autos norm in.bin out.bin ; in: vis cf32, freq f64, tau f64, w f32
int main(int argc, char** argv) {
    const int nstand = atoi(argv[1]), nfine = atoi(argv[2]), nfavg = atoi(argv[3]), npix = atoi(argv[4]), autos = atoi(argv[5]);
    const float norm = (float)atof(argv[6]);
    const size_t nin = 2 * (size_t)nstand;
    // exact-size heap blocks: the address sanitizer sees any access outside them
    float2* vis = (float2*)malloc(nfine * nin * nin * 8);
    double* freq = (double*)malloc(nfine * 8);
    double* tau = (double*)malloc((size_t)npix * nstand * 8);
    float* w = (float*)malloc(nstand * 4);
    const int ng = nfine / nfavg;
    float* out = (float*)malloc((size_t)ng * 4 * npix * 4);
    FILE* f = fopen(argv[7], "rb");
    if (!f || fread(vis, 8, nfine * nin * nin, f) != nfine * nin * nin || fread(freq, 8, nfine, f) != (size_t)nfine ||
        fread(tau, 8, (size_t)npix * nstand, f) != (size_t)npix * nstand || fread(w, 4, nstand, f) != (size_t)nstand) return 2;
    fclose(f);
    for (size_t i = 0; i < (size_t)ng * 4 * npix; i++) out[i] = -777.f;
    const size_t nlds = image_lds_bytes(nstand);
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (int k = 0; k < 4; k++) pthread_barrier_init(&g_wbar[k], nullptr, 64);
    for (int by = 0; by < ng; by++)
        for (int bx = 0; bx < (npix + IMG_PX - 1) / IMG_PX; bx++) {
            uint8_t* lds = (uint8_t*)malloc(nlds);
            memset(lds, 0xFF, nlds);        // NaN: whatever was there must not matter
            g_lds = lds;
            std::vector<std::thread> th;
            for (int t = 0; t < 256; t++) th.emplace_back([&, t, bx, by] {
                threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                image_kernel(vis, freq, tau, w, out, nstand, npix, nfavg, autos, norm);
            });
            for (auto& t : th) t.join();
            free(lds);
        }
    f = fopen(argv[8], "wb");
    fwrite(out, 4, (size_t)ng * 4 * npix, f);
    fclose(f);
    free(vis); free(freq); free(tau); free(w); free(out);
    return 0;
}
