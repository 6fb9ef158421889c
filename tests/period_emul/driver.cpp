// Runs period_spectrum_kernel of csrc/period_kernels.h on host threads, one work-group after another, the way period.hip launches it.
// The dynamic LDS starts as NaN before every work-group: nothing may depend on what it held.
// period_kernels_host.h is that header with its one `extern __shared__` line turned into a pointer to g_lds (the test writes it).
#include "period_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar;
float2* g_lds;
uint32_t g_slot[256];
using namespace xeng;
// args: NT nser nstack nlevel nwhite kmin in.bin(keep u8[N], z f32[nstack*NT][nser])  -> out.bin (A f32[nser][N], rec[nser][nlevel])
int main(int argc, char** argv) {
    int NT = atoi(argv[1]), nser = atoi(argv[2]), nstack = atoi(argv[3]), nlevel = atoi(argv[4]), B = atoi(argv[5]), kmin = atoi(argv[6]);
    int N = NT / 2, L = 0, lb = 0;
    while ((1 << L) < N) L++;
    while ((1 << lb) < B) lb++;
    FILE* f = fopen(argv[7], "rb");
    std::vector<unsigned char> keep(N);
    std::vector<float> z((size_t)nstack * NT * nser);
    if (fread(keep.data(), 1, N, f) != (size_t)N || fread(z.data(), 4, z.size(), f) != z.size()) return 2;
    fclose(f);
    std::vector<float> cnt(N / B, 0.f);
    for (int k = 1; k < N; k++) cnt[k / B] += keep[k] ? 1.f : 0.f;
    std::vector<float2> tw(N + N / 2);
    const double step = -2.0 * 3.14159265358979323846 / (double)NT;
    for (int k = 0; k < N; k++) tw[k] = make_float2((float)std::cos(step * k), (float)std::sin(step * k));
    for (int t = 0; t < N / 2; t++) { int k = 0; for (int b = 0; b < L; b++) k |= ((2 * t >> b) & 1) << (L - 1 - b); tw[N + t] = tw[k]; }
    std::vector<float> tbuf((size_t)nser * NT), A((size_t)nser * N, -7.f);
    std::vector<PeriodRecord> out((size_t)nser * nlevel, PeriodRecord{-5.f, -5});
    std::vector<float2> lds(N);
    g_lds = lds.data();
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (int s = 0; s < nstack; s++) {
        for (int n = 0; n < NT; n++) for (int i = 0; i < nser; i++) tbuf[(size_t)i * NT + n] = z[((size_t)s * NT + n) * nser + i];
        for (int blk = 0; blk < nser; blk++) {
            for (auto& v : lds) v = make_float2(NAN, NAN);      // whatever was there must not matter
            std::vector<std::thread> th;
            for (int t = 0; t < 256; t++) th.emplace_back([&, t, blk] {
                threadIdx.x = t; blockIdx.x = blk;
                period_spectrum_kernel(tbuf.data(), A.data(), keep.data(), cnt.data(), tw.data(), tw.data() + N, out.data(), L, lb, nlevel, kmin, s == 0, s == nstack - 1);
            });
            for (auto& x : th) x.join();
        }
    }
    f = fopen(argv[8], "wb");
    fwrite(A.data(), 4, A.size(), f); fwrite(out.data(), 8, out.size(), f); fclose(f);
    return 0;
}
