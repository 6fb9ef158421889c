// Runs the kernels of csrc/cdlong_kernels.h on host threads, one work-group after another and one launch after another, the way
// cdlong.hip launches them: columns forward, the overlap copy, rows, columns back; the table permuted into pass B's order, the
// twiddles from float64, the samples of every block after the first ingested behind the overlap that the copy kernel has moved.
// The dynamic LDS starts as NaN before every work-group: nothing may depend on what it held.  The time buffer, the scratch buffer and
// the output sit between canaries, which are checked at the end (exit status 3).  cdlong_kernels_host.h is that header with its
// `extern __shared__` lines turned into pointers to g_lds (the test writes it).
#include "cdlong_kernels_host.h"
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar;
float2* g_lds;
uint32_t g_slot[256];
using namespace xeng;

static std::vector<float2> g_ldsbuf;

// grid (gx, gy) of 256 threads: the 256 host threads walk the work-groups together, a barrier either side of each
template <class F> static void launch(int gx, int gy, F kernel) {
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([=] {
        threadIdx.x = t;
        for (int y = 0; y < gy; y++)
            for (int x = 0; x < gx; x++) {
                if (t == 0)
                    for (auto& v : g_ldsbuf) v = make_float2(NAN, NAN);     // whatever was there must not matter
                pthread_barrier_wait(&g_bar);
                blockIdx.x = x; blockIdx.y = y;
                kernel();
                pthread_barrier_wait(&g_bar);
            }
    });
    for (auto& t : th) t.join();
}

static uint32_t rev(uint32_t j, int bits) { return bits ? __brev(j) >> (32 - bits) : 0; }

// args: NFFT M nchan npair nblk in.bin (table cf32[npair][nchan][NFFT], x cf32[nchan * 2 npair][NFFT + (nblk - 1) L]) -> out.bin (cf32[nblk][nrow][L])
int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int N = atoi(argv[1]), M = atoi(argv[2]), nchan = atoi(argv[3]), npair = atoi(argv[4]), nblk = atoi(argv[5]);
    const int nb = 2 * npair, nrow = nchan * nb, L = N - M, CAN = 64;
    const size_t nsamp = (size_t)N + (size_t)(nblk - 1) * L;
    int LN = 0;
    while ((1 << LN) < N) LN++;
    const int LN1 = cl_ln1(LN), LN2 = LN - LN1, N1 = 1 << LN1, N2 = 1 << LN2, lr = cl_lrows(LN2);
    FILE* f = fopen(argv[6], "rb");
    std::vector<float2> table((size_t)npair * nchan * N), x((size_t)nrow * nsamp);
    if (!f || fread(table.data(), 8, table.size(), f) != table.size() || fread(x.data(), 8, x.size(), f) != x.size()) return 2;
    fclose(f);
    std::vector<float2> tab(table.size()), tws, tw1, tw2;
    for (size_t r = 0; r < (size_t)npair * nchan; r++)
        for (int i = 0; i < N1; i++)
            for (int j = 0; j < N2; j++) tab[r * N + (size_t)i * N2 + j] = table[r * N + rev(i, LN1) + (size_t)N1 * rev(j, LN2)];
    auto twiddles = [](std::vector<float2>& tw, int n) {
        const double step = -2.0 * 3.14159265358979323846 / (double)n;
        for (int k = 0; k < n / 2; k++) tw.push_back(make_float2((float)std::cos(step * k), (float)std::sin(step * k)));
    };
    twiddles(tws, N);
    twiddles(tw1, N1);
    twiddles(tw2, N2);
    const float2 can = make_float2(-7.f, 7.f);
    std::vector<float2> tbuf((size_t)nrow * N + 2 * CAN, can), scr((size_t)nrow * N + 2 * CAN, can), out((size_t)nblk * nrow * L + 2 * CAN, can);
    g_ldsbuf.resize(std::max(N1 * CL_TC, N2 << lr));
    g_lds = g_ldsbuf.data();
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (int j = 0; j < nblk; j++) {
        const int slot0 = j ? M : 0;
        for (int r = 0; r < nrow; r++)
            for (int s = slot0; s < N; s++) tbuf[CAN + (size_t)r * N + s] = x[(size_t)r * nsamp + (size_t)j * L + s];
        float2* const o = out.data() + CAN + (size_t)j * nrow * L;
        launch(N2 / CL_TC, nrow, [&] { cdlong_cols_fwd_kernel(tbuf.data() + CAN, scr.data() + CAN, tw1.data(), LN1, LN2); });
        if (M) launch((M + CL_THREADS - 1) / CL_THREADS, nrow, [&] { cdlong_tail_kernel(tbuf.data() + CAN, N, M); });
        launch(N1 >> lr, nrow, [&] { cdlong_rows_kernel(scr.data() + CAN, tab.data(), tws.data(), tw2.data(), LN1, LN2, nb, nchan); });
        launch(N2 / CL_TC, nrow, [&] { cdlong_cols_inv_kernel(scr.data() + CAN, o, tw1.data(), LN1, LN2, M); });
    }
    for (int i = 0; i < CAN; i++) {
        const float2 c[6] = {tbuf[i], tbuf[tbuf.size() - 1 - i], scr[i], scr[scr.size() - 1 - i], out[i], out[out.size() - 1 - i]};
        for (const float2& v : c)
            if (v.x != can.x || v.y != can.y) return 3;
    }
    f = fopen(argv[7], "wb");
    if (!f || fwrite(out.data() + CAN, 8, out.size() - 2 * CAN, f) != out.size() - 2 * CAN) return 2;
    fclose(f);
    return 0;
}
