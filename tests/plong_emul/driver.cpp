// Runs the kernels of csrc/plong_kernels.h on host threads, one work-group after another, in the order and with the arguments
// plong.hip launches them with for a run of calls from a reset: the ingest per call (the head of a call that completes the
// segment, then -- after the segment's mean and, per batch of SB series, columns, rows, untangle and whitening, and after a
// completed stack's sums and reduce -- its tail).  The dynamic LDS starts as NaN before every work-group: nothing may depend on
// what it held.  plong_kernels_host.h is that header with its `extern __shared__` lines turned into a pointer to g_lds (the test
// writes it).  Every buffer has exactly the size plong.hip gives it: the address sanitizer sees a word read or written outside.
#include "plong_kernels_host.h"
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
static void launch(int gx, int gy, size_t lds_bytes, const std::function<void()>& kernel) {
    g_ldsbuf.assign(lds_bytes ? lds_bytes / 4 : 1, NAN);     // (exactly the launch's words: the address sanitizer sees one more)
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

static int ilog2(int v) { int l = 0; while ((1 << l) < v) l++; return l; }

// in.bin: i32 {nser, nprod, NT, nstack, nlevel, B, nband, SB, ncalls, has_mask}, i32 kedge[nband + 1], i32 calls[ncalls],
//         u8 keep[NT/2] if has_mask, f32 z[sum calls][nser][nprod]
// out.bin: i32 nstacks, f32 A[nser][NT/2], PlongRecord out[nser][nlevel][nband] (of the last completed stack)
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[10];
    if (!f || fread(h, 4, 10, f) != 10) return 2;
    const int nser = h[0], nprod = h[1], NT = h[2], nstack = h[3], nlevel = h[4], B = h[5], nband = h[6], SB = h[7], ncalls = h[8], has_mask = h[9];
    const int N = NT / 2, LN = ilog2(N), LN1 = pl_ln1(LN), LN2 = LN - LN1, lb = ilog2(B), N1 = 1 << LN1, N2 = 1 << LN2;
    std::vector<int> kedge(nband + 1), calls(ncalls);
    if (fread(kedge.data(), 4, nband + 1, f) != (size_t)nband + 1 || fread(calls.data(), 4, ncalls, f) != (size_t)ncalls) return 2;
    std::vector<uint8_t> keep(N, 1);
    if (has_mask && fread(keep.data(), 1, N, f) != (size_t)N) return 2;
    for (auto& k : keep) k = k ? 1 : 0;
    size_t total = 0;
    for (int c : calls) total += c;
    std::vector<float> z(total * nser * nprod);
    if (fread(z.data(), 4, z.size(), f) != z.size()) return 2;
    fclose(f);
    std::vector<float> cnt(N / B, 0.f);
    for (int k = 1; k < N; k++) cnt[k / B] += (float)keep[k];
    auto table = [](size_t len) {
        std::vector<float2> t(len / 2);
        const double step = -2.0 * 3.14159265358979323846 / (double)len;
        for (size_t k = 0; k < len / 2; k++) t[k] = make_float2((float)std::cos(step * (double)k), (float)std::sin(step * (double)k));
        return t;
    };
    const std::vector<float2> tw = table(NT), tws = table(N), tw1 = table(N1), tw2 = table(N2);
    std::vector<float> tbuf((size_t)nser * NT, -7.f), A((size_t)nser * N, -7.f), P((size_t)SB * N, -7.f);
    std::vector<float2> scr((size_t)SB * N, float2{-7.f, -7.f});
    std::vector<PlongRecord> part((size_t)SB * nlevel * nband * PL_NTILE, PlongRecord{-5.f, -5}), out((size_t)nser * nlevel * nband, PlongRecord{-5.f, -5});
    std::vector<PlongMean> mv(nser, PlongMean{-7.f, -5});
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    auto ingest = [&](const float* in, int pos, int nc) {
        std::vector<float> span(in, in + (size_t)nc * nser * nprod);     // a copy of exactly the call's words: a read past them is seen
        launch((nser + PL_TILE - 1) / PL_TILE, (nc + PL_TILE - 1) / PL_TILE, 0, [&] {
            if (nprod == 1) plong_ingest_kernel<1>(span.data(), tbuf.data(), nser, NT, pos, nc);
            else plong_ingest_kernel<4>(span.data(), tbuf.data(), nser, NT, pos, nc);
        });
    };
    const int lr = pl_lrows(LN2), lw = pl_lwhite(lb);
    long long nwindows = 0;
    int nseg = 0, nstacks = 0;
    const float* in = z.data();
    for (int nc : calls) {
        const int pos = (int)(nwindows % NT), head = nc < NT - pos ? nc : NT - pos;
        if (nc > NT) return 3;
        ingest(in, pos, head);
        if (pos + head == NT) {
            const bool first = nseg == 0, stack_done = nseg + 1 == nstack;
            launch(nser, 1, 0, [&] { plong_mean_kernel(tbuf.data(), mv.data(), LN); });
            for (int s0 = 0; s0 < nser; s0 += SB) {
                const int ns = nser - s0 < SB ? nser - s0 : SB;
                launch(N2 / PL_TC, ns, (size_t)N1 * PL_TC * 8, [&] { plong_cols_kernel(tbuf.data(), mv.data(), scr.data(), tw1.data(), LN1, LN2, s0); });
                launch(N1 >> lr, ns, ((size_t)N2 << lr) * 8, [&] { plong_rows_kernel(scr.data(), tws.data(), tw2.data(), LN1, LN2); });
                launch(N2 / PL_TC, ns, (size_t)PL_TC * (N1 + PL_PPAD) * 4, [&] { plong_power_kernel(scr.data(), tw.data(), P.data(), LN1, LN2); });
                launch(1 << (LN - lw), ns, (size_t)4 << lw,
                       [&] { plong_whiten_kernel(P.data(), A.data(), keep.data(), cnt.data(), mv.data(), LN, lb, (int)first, s0); });
            }
            if (stack_done)
                for (int s0 = 0; s0 < nser; s0 += SB) {
                    const int ns = nser - s0 < SB ? nser - s0 : SB;
                    const long long nrec = (long long)ns * nlevel * nband;
                    launch(PL_NTILE, ns, 0, [&] { plong_sums_kernel(A.data(), kedge.data(), part.data(), LN, nlevel, nband, s0); });
                    launch((int)((nrec + 255) / 256), 1, 0, [&] { plong_reduce_kernel(part.data(), out.data() + (size_t)s0 * nlevel * nband, nrec); });
                }
            nseg = stack_done ? 0 : nseg + 1;
            nstacks += stack_done;
            if (nc > head) ingest(in + (size_t)head * nser * nprod, 0, nc - head);
        }
        in += (size_t)nc * nser * nprod;
        nwindows += nc;
    }
    f = fopen(argv[2], "wb");
    fwrite(&nstacks, 4, 1, f);
    fwrite(A.data(), 4, A.size(), f);
    fwrite(out.data(), 8, out.size(), f);
    fclose(f);
    return 0;
}
