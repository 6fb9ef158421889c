// Runs the kernels of csrc/rfi_kernels.h on host threads, one work-group after another, in the order and with the arguments rfi.hip
// launches them with for a run of calls from a fresh context: the ingest, the decision on a call that takes a block's last window,
// the apply.  The dynamic LDS starts as NaN before every work-group and has exactly the launch's words.  rfi_kernels_host.h is the
// header with its `extern __shared__` lines turned into a pointer to g_lds (the test writes it).  Every buffer has exactly the size
// rfi.hip gives it: the address sanitizer sees a word read or written outside.  After every call out and stats, and after a call
// that decided a block its tables, must equal the bytes of the expectation file (exit status 4 + what differed otherwise).
#include "rfi_kernels_host.h"
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
    g_ldsbuf.assign(lds_bytes ? lds_bytes / 4 : 1, NAN);    // (exactly the launch's words: the address sanitizer sees one more)
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

struct Event { int at; float k_chan; RfiControl c; std::vector<unsigned char> mask; };

struct Half {
    std::vector<float4> c, m, g;
    std::vector<float2> v;
    std::vector<float> mu, var, r;
    std::vector<int> notkept;
    std::vector<unsigned char> flag;
    Half(size_t NC, int npair) : c(NC), m(NC), g(NC), v(NC), mu(NC), var(NC), r(NC), notkept(npair), flag(NC) {}
    RfiTables tables() { return RfiTables{c.data(), m.data(), g.data(), v.data(), mu.data(), var.data(), r.data(), notkept.data(), flag.data()}; }
};

// in.bin:  i32 {npair, nfine, nstat, nwin, ncalls, nevents}, i32 calls[ncalls], per event (controls and mask given before call `at`)
//          i32 at, f32 {k_chan, t_clip, t_broad}, i32 {min_count, zerodm}, u8 mask[nfine rounded up to 4]; f32 x[sum calls][NC][4]
// exp.bin: per call f32 out[nc][NC][4], i32 stats[nc][npair][4] and, when the call decided a block, u8 flags[NC], f32 mu[NC],
//          var[NC], r[NC], gains[NC][4]
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[6];
    if (!f || fread(h, 4, 6, f) != 6) return 2;
    const int npair = h[0], nfine = h[1], nstat = h[2], nwin = h[3], ncalls = h[4], nevents = h[5];
    const size_t NC = (size_t)npair * nfine;
    const int L = nstat + nwin;
    std::vector<int> calls(ncalls);
    if (fread(calls.data(), 4, ncalls, f) != (size_t)ncalls) return 2;
    std::vector<Event> events(nevents);
    for (auto& e : events) {
        e.mask.resize((nfine + 3) & ~3);
        if (fread(&e.at, 4, 1, f) != 1 || fread(&e.k_chan, 4, 1, f) != 1 || fread(&e.c, sizeof(RfiControl), 1, f) != 1 ||
            fread(e.mask.data(), 1, e.mask.size(), f) != e.mask.size())
            return 2;
        e.mask.resize(nfine);
        e.mask.shrink_to_fit();
    }
    size_t total = 0;
    for (int c : calls) total += c;
    std::vector<float4> xin(total * NC);
    if (fread(xin.data(), 16, xin.size(), f) != xin.size()) return 2;
    fclose(f);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe) return 2;

    // the context's state, each piece at its exact size
    std::vector<float4> ring((size_t)L * NC, float4{0, 0, 0, 0}), run(3 * NC, float4{0, 0, 0, 0});
    Half half[2] = {Half(NC, npair), Half(NC, npair)};
    std::vector<unsigned char> mask(nfine, 0);
    RfiTables2 tab;
    tab.h[0] = half[0].tables();
    tab.h[1] = half[1].tables();
    RfiControl2 ctl = {};
    RfiControl cur = {0.f, 0.f, 0, 0};
    float k_chan = 0.f;
    bool have = false;
    const float r = 1.0f / (float)nstat;
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    auto differs = [&](const void* got, size_t bytes) {
        std::vector<uint8_t> e(bytes);
        return fread(e.data(), 1, bytes, fe) != bytes || memcmp(e.data(), got, bytes) != 0;
    };
    long long nwindows = 0;
    int nblocks = 0;
    const float4* in = xin.data();
    for (int ic = 0; ic < ncalls; ic++) {
        for (auto& e : events)
            if (e.at == ic) {
                k_chan = e.k_chan;
                cur = e.c;
                mask = e.mask;
                have = true;
            }
        const int nc = calls[ic];
        if (!have || nc < 1 || nc > nwin) return 3;
        std::vector<float4> span(in, in + (size_t)nc * NC);     // a copy of exactly the call's words: a read past them is seen
        std::vector<float4> out((size_t)nc * NC, float4{-5.f, -5.f, -5.f, -5.f});
        std::vector<int> stats((size_t)nc * npair * 4, -5);
        const long long n0 = nwindows, k0 = n0 / nstat;
        const int pos0 = (int)(n0 % nstat);
        const bool done = pos0 + nc >= nstat;
        launch((int)((NC + RF_THREADS - 1) / RF_THREADS), 1, 0, [&] {
            rfi_ingest_kernel(span.data(), ring.data(), run.data(), tab, NC, nc, nstat, L, pos0, (int)(n0 % L), (int)(k0 & 1), r);
        });
        if (done) {
            ctl.h[k0 & 1] = cur;
            launch(npair, 1, rfi_decide_lds_bytes(nfine), [&] { rfi_decide_kernel(tab.h[k0 & 1], mask.data(), nfine, k_chan); });
        }
        launch(nc, npair, RF_APPLY_LDS_BYTES, [&] { rfi_apply_kernel(ring.data(), tab, ctl, out.data(), stats.data(), nfine, npair, nstat, L, n0 - nstat); });
        int bad = 0;
        if (differs(out.data(), out.size() * 16)) bad |= 1;
        if (differs(stats.data(), stats.size() * 4)) bad |= 2;
        if (done) {
            Half& t = half[k0 & 1];
            if (differs(t.flag.data(), NC)) bad |= 4;
            if (differs(t.mu.data(), NC * 4)) bad |= 8;
            if (differs(t.var.data(), NC * 4)) bad |= 8;
            if (differs(t.r.data(), NC * 4)) bad |= 8;
            if (differs(t.g.data(), NC * 16)) bad |= 16;
            nblocks++;
        }
        if (bad) {
            fprintf(stderr, "call %d: out / stats / flags / mu, var, r / gains differ from the restatement (mask %d)\n", ic, bad);
            return 4 + bad;
        }
        in += (size_t)nc * NC;
        nwindows += nc;
    }
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) { fprintf(stderr, "the expectation holds more than the %d calls\n", ncalls); return 3; }
    fclose(fe);
    printf("%d\n", nblocks);
    return 0;
}
