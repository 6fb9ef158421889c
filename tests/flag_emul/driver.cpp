// Runs flag_stats_kernel, flag_test_kernel and flag_chan_kernel of csrc/flag_kernels.h on host threads, one work-group after
// another, the way flag.hip launches them.  Every buffer is a heap block of its exact size, so the address sanitizer this is built
// with sees any access outside it; the partial sums, the autos and the outputs start as NaN or a pattern no result has, so a word
// nobody wrote shows.
#include <hip/hip_runtime.h>
#include "flag_kernels.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar;
using namespace xeng;

template <class F>
static void work_group(int nthreads, int bx, int by, F f) {
    pthread_barrier_init(&g_bar, nullptr, nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++) th.emplace_back([=] {
        threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
        f();
    });
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&g_bar);
}

// args: nstand nfine wchan in.bin out.bin ; in: vis cf32, w f32[nstand], k f32[3] = {cross, auto, chan} ;
// out: mask u8[nfine][2][nstand], stats f32[nfine][2][nstand][2], chan f32[nfine][2][4]
int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int nstand = atoi(argv[1]), nfine = atoi(argv[2]), wchan = atoi(argv[3]);
    const size_t nin = 2 * (size_t)nstand, nv = nfine * nin * nin, ncps = (size_t)nfine * 2 * nstand;
    const int ntile = (nstand + FL_T - 1) / FL_T;
    float2* vis = (float2*)aligned_alloc(16, nv * 8);
    float* w = (float*)malloc(nstand * 4);
    float k[3];
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(vis, 8, nv, f) != nv || fread(w, 4, nstand, f) != (size_t)nstand || fread(k, 4, 3, f) != 3) return 2;
    fclose(f);
    float2* zero = (float2*)aligned_alloc(16, 16);
    memset(zero, 0, 16);
    float* part = (float*)malloc(ncps * ntile * 4);
    float* au = (float*)malloc(ncps * 4);
    unsigned char* mask = (unsigned char*)malloc(ncps);
    float* stats = (float*)malloc(ncps * 2 * 4);
    float* chan = (float*)malloc((size_t)nfine * 2 * 4 * 4);
    memset(part, 0xFF, ncps * ntile * 4);
    memset(au, 0xFF, ncps * 4);
    memset(mask, 0xEE, ncps);
    memset(stats, 0xFF, ncps * 2 * 4);
    memset(chan, 0xFF, (size_t)nfine * 2 * 4 * 4);
    for (int by = 0; by < nfine; by++)
        for (int bx = 0; bx < ntile * (ntile + 1) / 2; bx++) work_group(FL_THREADS, bx, by, [=] { flag_stats_kernel(vis, w, zero, part, au, nstand); });
    for (int by = 0; by < nfine; by++)
        for (int bx = 0; bx < 2; bx++) work_group(FL_TEST_THREADS, bx, by, [=] { flag_test_kernel(part, au, w, mask, stats, chan, nstand, k[0], k[1]); });
    for (int bx = 0; bx < 2; bx++) work_group(FL_CHAN_THREADS, bx, 0, [=] { flag_chan_kernel(mask, chan, nstand, nfine, k[2], wchan); });
    f = fopen(argv[5], "wb");
    fwrite(mask, 1, ncps, f);
    fwrite(stats, 4, ncps * 2, f);
    fwrite(chan, 4, (size_t)nfine * 2 * 4, f);
    fclose(f);
    free(vis); free(w); free(zero); free(part); free(au); free(mask); free(stats); free(chan);
    return 0;
}
