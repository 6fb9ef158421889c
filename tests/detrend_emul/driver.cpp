// Runs the kernels of csrc/detrend_kernels.h on host threads, one work-group after another, with the grids, the LDS bytes and the
// arguments detrend.hip launches them with for a run of calls from a fresh context: the ingest, the decision on a call that takes a
// block's last window, the apply.  The dynamic LDS starts as NaN before every work-group and has exactly the launch's words.
// detrend_kernels_host.h is the header with its `extern __shared__` lines turned into a pointer to g_lds (the test writes it).
// Every buffer has exactly the size detrend.hip gives it (the input is a copy of exactly the call's windows): the address sanitizer
// sees a word read or written outside.  The ring and the knot tables start as NaN (the valid bytes as 0xA5), and a Reset changes the
// host's counts only, as xengDetrendReset does: a value used from before window 0 shows.  After every call the output, and after a
// call that decided a block its M, A and valid bytes, must equal the expectation file (exit status 4 + what differed otherwise).
#include "detrend_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx, gridDim;
pthread_barrier_t g_bar, g_wbar[4];
float* g_lds;
uint32_t g_slot[256];
static std::vector<float> g_ldsbuf;
using namespace xeng;

// a launch: 256 threads walk the grid together; LDS is NaN before every work-group
static void launch(int gx, int gy, size_t lds_bytes, const std::function<void()>& kernel) {
    g_ldsbuf.assign(lds_bytes / 4, NAN);        // (exactly the launch's words: the address sanitizer sees one more)
    g_lds = g_ldsbuf.data();
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int b = 0; b < gx * gy; b++) {
            if (t == 0) for (auto& v : g_ldsbuf) v = NAN;
            pthread_barrier_wait(&g_bar);
            threadIdx.x = t; blockIdx.x = b % gx; blockIdx.y = b / gx; gridDim.x = gx; gridDim.y = gy;
            kernel();
            pthread_barrier_wait(&g_bar);
        }
    });
    for (auto& x : th) x.join();
}

// in.bin:  i32 {nser, nprod, nblk, nwin, normalise, ncalls, nresets}, f32 k_mad, i32 calls[ncalls], i32 resets[nresets] (a Reset
//          before that call), f32 x[sum calls][nser][nprod]
// exp.bin: per call f32 out[nc][nser] and, when the call decided a block, f32 M[nser], f32 A[nser], u8 valid[nser]
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[7];
    float k_mad;
    if (!f || fread(h, 4, 7, f) != 7 || fread(&k_mad, 4, 1, f) != 1) return 2;
    const int nser = h[0], nprod = h[1], nblk = h[2], nwin = h[3], normalise = h[4], ncalls = h[5], nresets = h[6];
    if ((nprod != 1 && nprod != 4) || nblk < 4 || nblk > 8192 || (nblk & 1) || nwin < 1 || nwin > nblk || nser < 1) return 3;
    std::vector<int> calls(ncalls), resets(nresets);
    if (fread(calls.data(), 4, ncalls, f) != (size_t)ncalls || fread(resets.data(), 4, nresets, f) != (size_t)nresets) return 2;
    size_t total = 0;
    for (int c : calls) total += c;
    std::vector<float> xin(total * nser * nprod);
    if (fread(xin.data(), 4, xin.size(), f) != xin.size()) return 2;
    fclose(f);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe) return 2;

    // the context's state as Initialize sizes it, each piece at its exact size
    const int D = 3 * (nblk / 2), L = D + nwin;
    const float r = 1.0f / (float)(2 * nblk);
    std::vector<float> ring((size_t)nser * L, NAN), M((size_t)DT_KNOTS * nser, NAN), A(M), G(M);
    std::vector<unsigned char> valid((size_t)DT_KNOTS * nser, 0xA5);
    DetrendKnots kn{M.data(), A.data(), G.data(), valid.data()};
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    auto differs = [&](const void* got, size_t bytes) {
        std::vector<uint8_t> e(bytes);
        return fread(e.data(), 1, bytes, fe) != bytes || memcmp(e.data(), got, bytes) != 0;
    };
    long long nwindows = 0, nblocks = 0;
    int ndecided = 0;
    const float* in = xin.data();
    for (int ic = 0; ic < ncalls; ic++) {
        for (int rs : resets)
            if (rs == ic) nwindows = nblocks = 0;
        const int nc = calls[ic];
        if (nc < 1 || nc > nwin) return 3;
        std::vector<float> span(in, in + (size_t)nc * nser * nprod);    // a copy of exactly the call's words: a read past them is seen
        std::vector<float> out((size_t)nc * nser, -5.f);
        const long long n0 = nwindows, kcur = n0 / nblk;
        const int e0 = (int)(n0 % nblk);
        const bool done = e0 + nc >= nblk;
        const int gx = (nser + DT_TILE - 1) / DT_TILE, gy = (nc + DT_TILE - 1) / DT_TILE;
        launch(gx, gy, DT_TILE_LDS_BYTES, [&] {
            if (nprod == 1) detrend_ingest_kernel<1>(span.data(), ring.data(), nser, L, (int)(n0 % L), nc);
            else detrend_ingest_kernel<4>(span.data(), ring.data(), nser, L, (int)(n0 % L), nc);
        });
        if (done)
            launch(nser, 1, detrend_decide_lds_bytes(nblk), [&] {
                detrend_decide_kernel(ring.data(), kn, nser, nblk, L, (int)((kcur * nblk) % L), (int)(kcur & (DT_KNOTS - 1)), normalise, k_mad);
            });
        const long long m0 = n0 - D;
        const int slotm0 = (int)(((m0 % L) + L) % L);
        launch(gx, gy, DT_TILE_LDS_BYTES, [&] { detrend_apply_kernel(ring.data(), kn, out.data(), nser, nblk, L, nc, kcur - 2, e0, slotm0, normalise, r); });
        int bad = 0;
        if (differs(out.data(), out.size() * 4)) bad |= 1;
        if (done) {
            const size_t at = (size_t)(kcur & (DT_KNOTS - 1)) * nser;
            if (differs(M.data() + at, (size_t)nser * 4)) bad |= 2;
            if (differs(A.data() + at, (size_t)nser * 4)) bad |= 4;
            if (differs(valid.data() + at, (size_t)nser)) bad |= 8;
            nblocks++;
            ndecided++;
        }
        if (bad) {
            fprintf(stderr, "call %d (windows %lld + %d): out / M / A / valid differ from the restatement (mask %d)\n", ic, n0, nc, bad);
            return 4 + bad;
        }
        in += (size_t)nc * nser * nprod;
        nwindows += nc;
    }
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) { fprintf(stderr, "the expectation holds more than the %d calls\n", ncalls); return 3; }
    fclose(fe);
    printf("%d\n", ndecided);
    return 0;
}
