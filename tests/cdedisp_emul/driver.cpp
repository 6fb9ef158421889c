// Runs cdedisp_filter_kernel of csrc/cdedisp_kernels.h on host threads, one work-group after another, the way cdedisp.hip launches
// it: the table permuted to bit-reversed order, the twiddles from float64, the samples of every block after the first ingested
// behind the overlap that the kernel itself has moved.  The dynamic LDS starts as NaN before every work-group: nothing may depend
// on what it held.  The time buffer and the output sit between canaries, which are checked at the end (exit status 3).
// cdedisp_kernels_host.h is that header with its one `extern __shared__` line turned into a pointer to g_lds (the test writes it).
#include "cdedisp_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar;
float2* g_lds;
uint32_t g_slot[256];
using namespace xeng;
// args: NFFT M nchan npair nblk in.bin (table cf32[npair][nchan][NFFT], x cf32[nchan * 2 npair][NFFT + (nblk - 1) L]) -> out.bin (cf32[nblk][nrow][L])
int main(int argc, char** argv) {
    const int N = atoi(argv[1]), M = atoi(argv[2]), nchan = atoi(argv[3]), npair = atoi(argv[4]), nblk = atoi(argv[5]);
    const int nb = 2 * npair, nrow = nchan * nb, L = N - M, CAN = 64;
    const size_t nsamp = (size_t)N + (size_t)(nblk - 1) * L;
    int LN = 0;
    while ((1 << LN) < N) LN++;
    FILE* f = fopen(argv[6], "rb");
    std::vector<float2> table((size_t)npair * nchan * N), x((size_t)nrow * nsamp);
    if (!f || fread(table.data(), 8, table.size(), f) != table.size() || fread(x.data(), 8, x.size(), f) != x.size()) return 2;
    fclose(f);
    std::vector<float2> tab(table.size()), tw(N / 2);
    for (size_t r = 0; r < (size_t)npair * nchan; r++)
        for (int j = 0; j < N; j++) tab[r * N + j] = table[r * N + (__brev((uint32_t)j) >> (32 - LN))];
    const double step = -2.0 * 3.14159265358979323846 / (double)N;
    for (int k = 0; k < N / 2; k++) tw[k] = make_float2((float)std::cos(step * k), (float)std::sin(step * k));
    const float2 can = make_float2(-7.f, 7.f);
    std::vector<float2> tbuf((size_t)nrow * N + 2 * CAN, can), out((size_t)nblk * nrow * L + 2 * CAN, can), lds(N);
    g_lds = lds.data();
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (int j = 0; j < nblk; j++) {
        const int slot0 = j ? M : 0;
        for (int r = 0; r < nrow; r++)
            for (int s = slot0; s < N; s++) tbuf[CAN + (size_t)r * N + s] = x[(size_t)r * nsamp + (size_t)j * L + s];
        for (int blk = 0; blk < nrow; blk++) {
            for (auto& v : lds) v = make_float2(NAN, NAN);      // whatever was there must not matter
            std::vector<std::thread> th;
            for (int t = 0; t < 256; t++) th.emplace_back([&, t, blk, j] {
                threadIdx.x = t; blockIdx.x = blk;
                cdedisp_filter_kernel(tbuf.data() + CAN, tab.data(), tw.data(), out.data() + CAN + (size_t)j * nrow * L, LN, M, nb, nchan);
            });
            for (auto& t : th) t.join();
        }
    }
    for (int i = 0; i < CAN; i++) {
        const float2 c[4] = {tbuf[i], tbuf[tbuf.size() - 1 - i], out[i], out[out.size() - 1 - i]};
        for (const float2& v : c)
            if (v.x != can.x || v.y != can.y) return 3;
    }
    f = fopen(argv[7], "wb");
    fwrite(out.data() + CAN, 8, out.size() - 2 * CAN, f);
    fclose(f);
    return 0;
}
