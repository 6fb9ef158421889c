// Runs predict_kernel of csrc/predict_kernels.h on host threads, one work-group after another, the way predict.hip launches it.  The
// LDS starts as NaN before every work-group: nothing may depend on what it held.  Every buffer is a heap block of its exact size, so
// the address sanitizer this is built with sees any access outside it; the output starts as a pattern no result has, so a word nobody
// wrote shows.  predict_kernels_host.h is that header with its vector typedef and its one `__shared__` line replaced (the test writes
// it).  nrec is found the way xengPredictSetComponents finds it.
#include "predict_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar;
uint8_t* g_lds;
float g_a[64], g_b[64];
using namespace xeng;
// args: nstand nfine nfavg ndir ncomp_max cross model in.bin out.bin ; in: freq f64[nfine], tau f64[ndir][nstand], records
// [nfine / nfavg][ncomp_max], then (model = 0) vis cf32 ; out: cf32 in vis's layout
int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int nstand = atoi(argv[1]), nfine = atoi(argv[2]), nfavg = atoi(argv[3]), ndir = atoi(argv[4]), ncomp_max = atoi(argv[5]), cross = atoi(argv[6]),
              model = atoi(argv[7]);
    const int ngroup = nfine / nfavg;
    const size_t nin = 2 * (size_t)nstand, nv = nfine * nin * nin, nt = (size_t)ndir * nstand, nr = (size_t)ngroup * ncomp_max;
    float2* vis = model ? nullptr : (float2*)aligned_alloc(16, nv * 8);
    double* freq = (double*)malloc(nfine * 8);
    double* tau = (double*)malloc(nt * 8);
    pr_record* rec = (pr_record*)aligned_alloc(32, nr * 32);
    int* nrec = (int*)malloc(ngroup * 4);
    float2* out = (float2*)aligned_alloc(16, nv * 8);
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(freq, 8, nfine, f) != (size_t)nfine || fread(tau, 8, nt, f) != nt || fread(rec, 32, nr, f) != nr || (!model && fread(vis, 8, nv, f) != nv)) return 2;
    fclose(f);
    for (int g = 0; g < ngroup; g++) {
        nrec[g] = 0;
        for (int k = 0; k < ncomp_max; k++)
            if (rec[(size_t)g * ncomp_max + k].pixel >= 0) nrec[g] = k + 1;
    }
    for (size_t i = 0; i < nv; i++) out[i] = make_float2(-777.f, -777.f);
    const size_t nlds = predict_lds_bytes();
    const int ntile = (nstand + PR_T - 1) / PR_T;
    pthread_barrier_init(&g_bar, nullptr, PR_THREADS);
    for (int by = 0; by < nfine; by++)
        for (int bx = 0; bx < ntile * (ntile + 1) / 2; bx++) {
            uint8_t* lds = (uint8_t*)aligned_alloc(16, nlds);
            memset(lds, 0xFF, nlds);        // NaN: whatever was there must not matter
            g_lds = lds;
            std::vector<std::thread> th;
            for (int t = 0; t < PR_THREADS; t++) th.emplace_back([&, t, bx, by] {
                threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                if (cross)
                    predict_kernel<true>(vis, freq, tau, rec, nrec, out, nstand, nfavg, ncomp_max, model);
                else
                    predict_kernel<false>(vis, freq, tau, rec, nrec, out, nstand, nfavg, ncomp_max, model);
            });
            for (auto& t : th) t.join();
            free(lds);
        }
    f = fopen(argv[9], "wb");
    fwrite(out, 8, nv, f);
    fclose(f);
    free(vis); free(freq); free(tau); free(rec); free(nrec); free(out);
    return 0;
}
