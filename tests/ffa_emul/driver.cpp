// Runs the four kernels of csrc/ffa_kernels.h on host threads, one work-group after another, in the order and with the arguments
// ffa.hip launches them with for a run of calls from a reset: the ingest per call (the head of a call that completes the segment,
// then -- after the segment's prepare, folds and reduce -- its tail), the carried partial sums in two halves.
// The dynamic LDS starts as NaN before every work-group: nothing may depend on what it held.
// ffa_kernels_host.h is that header with its one `extern __shared__` line turned into a pointer to g_lds (the test writes it).
#include "ffa_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar, g_wbar[4];
float* g_lds;
uint32_t g_slot[256];
static std::vector<float> g_ldsbuf;
using namespace xeng;

// a launch: 256 threads walk the grid together; LDS is NaN before every work-group
static void launch(int gx, int gy, size_t lds_words, const std::function<void()>& kernel) {
    g_ldsbuf.assign(lds_words ? lds_words : 1, NAN);     // (exactly the launch's words: the address sanitizer sees one more)
    g_lds = g_ldsbuf.data();
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int by = 0; by < gy; by++)
            for (int bx = 0; bx < gx; bx++) {
                if (t == 0) for (auto& v : g_ldsbuf) v = NAN;
                pthread_barrier_wait(&g_bar);
                threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                kernel();
                pthread_barrier_wait(&g_bar);
            }
    });
    for (auto& x : th) x.join();
}

// in.bin: i32 {nser, nprod, nds, NT, noct, pmin, pmax, nwidth, ncalls}, i32 calls[ncalls], f32 z[sum calls][nser][nprod]
// out.bin: f32 stats[nser][noct][4], FfaRecord out[nser][noct][nwidth], f32 tbuf[nser][NT] (as the last segment left it)
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[9];
    if (!f || fread(h, 4, 9, f) != 9) return 2;
    const int nser = h[0], nprod = h[1], nds = h[2], NT = h[3], noct = h[4], pmin = h[5], pmax = h[6], nwidth = h[7], ncalls = h[8];
    std::vector<int> calls(ncalls);
    if (fread(calls.data(), 4, ncalls, f) != (size_t)ncalls) return 2;
    size_t total = 0;
    for (int c : calls) total += c;
    std::vector<float> z(total * nser * nprod);
    if (fread(z.data(), 4, z.size(), f) != z.size()) return 2;
    fclose(f);
    const int np = pmax - pmin + 1;
    int xw = 0;
    FfaRinv rinv{};
    for (int o = 0; o < noct; o++) { xw += NT >> o; rinv.r[o] = (float)(1.0 / (double)(NT >> o)); }
    std::vector<float> rho(FA_MAX_WIDTH * FA_RHO_STRIDE);
    for (int iw = 0; iw < FA_MAX_WIDTH; iw++)
        for (int lm = 0; lm < FA_RHO_STRIDE; lm++) rho[iw * FA_RHO_STRIDE + lm] = (float)(1.0 / std::sqrt((double)(1 << iw) * (double)(1 << lm)));
    // exact sizes, so that the address sanitizer sees any word outside them
    std::vector<float> tbuf((size_t)nser * NT, -7.f), xbuf((size_t)nser * xw, -7.f), stats((size_t)nser * noct * 4, -7.f), part(2 * (size_t)nser, -7.f);
    std::vector<FfaRecord> table((size_t)nser * noct * np * nwidth, FfaRecord{-5.f, -5, -5, -5}), out((size_t)nser * noct * nwidth, FfaRecord{-5.f, -5, -5, -5});
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    int par = 0, ndone = 0;
    auto ingest = [&](const float* in, int pos, int nc) {
        const int nk = (pos + nc - 1) / nds - pos / nds + 1;
        const float* pin = part.data() + (size_t)par * nser;
        float* pout = part.data() + (size_t)(par ^ 1) * nser;
        // a copy of exactly the call's words: a read past them is seen
        std::vector<float> span(in, in + (size_t)nc * nser * nprod);
        launch((nser + FA_TILE - 1) / FA_TILE, (nk + FA_TILE - 1) / FA_TILE, 0, [&] {
            if (nprod == 1) ffa_ingest_kernel<1>(span.data(), tbuf.data(), pin, pout, nser, NT, nds, pos, nc);
            else ffa_ingest_kernel<4>(span.data(), tbuf.data(), pin, pout, nser, NT, nds, pos, nc);
        });
        par ^= 1;
    };
    long long nwindows = 0;
    const float* in = z.data();
    const int seg = NT * nds;
    for (int nc : calls) {
        const int pos = (int)(nwindows % seg), head = nc < seg - pos ? nc : seg - pos;
        if (nc > seg) return 3;
        ingest(in, pos, head);
        if (pos + head == seg) {
            launch(nser, 1, 0, [&] { ffa_prepare_kernel(tbuf.data(), xbuf.data(), stats.data(), rinv, NT, noct); });
            for (int o = 0; o < noct; o++) {
                int words = 0;
                for (int p = pmin; p <= pmax; p++) { int w = p; while (2 * w <= (NT >> o)) w *= 2; if (w > words) words = w; }
                launch(nser, np, 2 * (size_t)words, [&] { ffa_fold_kernel(xbuf.data(), stats.data(), rho.data(), table.data(), NT, noct, o, pmin, np, nwidth); });
            }
            const long long nrec = (long long)nser * noct * nwidth;
            launch((int)((nrec + 255) / 256), 1, 0, [&] { ffa_reduce_kernel(table.data(), out.data(), nrec, np, nwidth); });
            ndone++;
            if (nc > head) ingest(in + (size_t)head * nser * nprod, 0, nc - head);
        }
        in += (size_t)nc * nser * nprod;
        nwindows += nc;
    }
    f = fopen(argv[2], "wb");
    fwrite(stats.data(), 4, stats.size(), f);
    fwrite(out.data(), 16, out.size(), f);
    fwrite(tbuf.data(), 4, tbuf.size(), f);
    fclose(f);
    return ndone == 1 ? 0 : 4;
}
