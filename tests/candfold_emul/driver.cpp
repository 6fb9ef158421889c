// Runs the kernels of csrc/candfold_kernels.h on host threads, one work-group after another, in the order and with the arguments
// candfold.hip launches them with for a run of calls from a fresh context: the fold per call and, per completed segment, the refine
// and the clearing launch, with the two cubes and the two candidate tables changing places as they do there.  The dynamic LDS
// starts as NaN before every work-group and has exactly the launch's words.  candfold_kernels_host.h is the header with its
// `extern __shared__` lines turned into a pointer to g_lds (the test writes it).  Every buffer has exactly the size candfold.hip
// gives it: the address sanitizer sees a word read or written outside.  After every completed segment the cube, the hits, the
// records and the best profiles must equal the bytes of the expectation file (exit status 4 + what differed otherwise).
#include "candfold_kernels_host.h"
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
static void launch(int gx, size_t lds_bytes, const std::function<void()>& kernel) {
    g_ldsbuf.assign(lds_bytes ? lds_bytes / 4 : 1, NAN);     // (exactly the launch's words: the address sanitizer sees one more)
    g_lds = g_ldsbuf.data();
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int bx = 0; bx < gx; bx++) {
            if (t == 0) for (auto& v : g_ldsbuf) v = NAN;
            pthread_barrier_wait(&g_bar);
            threadIdx.x = t; blockIdx.x = bx; gridDim.x = gx;
            kernel();
            pthread_barrier_wait(&g_bar);
        }
    });
    for (auto& x : th) x.join();
}

struct Set { int at, ncand; std::vector<CfCand> tab; };

// in.bin:  i32 {nser, nprod, ncand_max, nbin, nsub, nsubwin, nwidth, ntrial, ncalls, nsets}, i32 d1[ntrial], i32 d2[ntrial],
//          f32 g[nwidth], i32 calls[ncalls], per set i32 {at, ncand} and CfCand[ncand] (given before call `at`),
//          f32 z[sum calls][nser][nprod]
// exp.bin: per completed segment f32 cube[ncand_max][W], u32 hits[ncand_max][W], CfRecord[ncand_max], f32 prof[ncand_max][nbin]
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[10];
    if (!f || fread(h, 4, 10, f) != 10) return 2;
    const int nser = h[0], nprod = h[1], ncand_max = h[2], nbin = h[3], nsub = h[4], nsubwin = h[5], nwidth = h[6], ntrial = h[7], ncalls = h[8], nsets = h[9];
    const int W = nsub * nbin;
    const long long NT = (long long)nsub * nsubwin;
    std::vector<int> d1(ntrial), d2(ntrial), calls(ncalls);
    std::vector<float> gain(nwidth);
    if (fread(d1.data(), 4, ntrial, f) != (size_t)ntrial || fread(d2.data(), 4, ntrial, f) != (size_t)ntrial ||
        fread(gain.data(), 4, nwidth, f) != (size_t)nwidth || fread(calls.data(), 4, ncalls, f) != (size_t)ncalls)
        return 2;
    std::vector<Set> sets(nsets);
    for (auto& s : sets) {
        int a[2];
        if (fread(a, 4, 2, f) != 2) return 2;
        s.at = a[0]; s.ncand = a[1];
        s.tab.assign(ncand_max, CfCand{0, 0, 0, 0, 0});
        if (s.ncand < 1 || s.ncand > ncand_max || fread(s.tab.data(), sizeof(CfCand), s.ncand, f) != (size_t)s.ncand) return 2;
    }
    size_t total = 0;
    for (int c : calls) total += c;
    std::vector<float> z(total * nser * nprod);
    if (fread(z.data(), 4, z.size(), f) != z.size()) return 2;
    fclose(f);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe) return 2;

    // the context's state, each piece at its exact size
    const size_t cw = (size_t)ncand_max * W;
    std::vector<uint32_t> half[2] = {std::vector<uint32_t>(2 * cw, 0u), std::vector<uint32_t>(2 * cw, 0u)};     // a cube and its hits
    std::vector<CfCand> cand[2] = {std::vector<CfCand>(ncand_max, CfCand{0, 0, 0, 0, 0}), std::vector<CfCand>(ncand_max, CfCand{0, 0, 0, 0, 0})};
    std::vector<int> rot((size_t)ntrial * nsub), zrot(nsub, 0);
    int izero = -1;
    for (int t = 0; t < ntrial; t++) {
        if (izero < 0 && d1[t] == 0 && d2[t] == 0) izero = t;
        for (int s = 0; s < nsub; s++) {
            const long long r = cf_shift(d1[t], d2[t], s, nsub) % nbin;
            rot[(size_t)t * nsub + s] = (int)(r < 0 ? r + nbin : r);
        }
    }
    std::vector<CfRecord> out((size_t)ncand_max + (size_t)ncand_max * nbin / 4, CfRecord{-5.f, -5.f, -5, -5, -5, -5});
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    int cur = 0, act = 0;
    bool have = false, pending = false;
    long long n_ref = 0, nwindows = 0;
    int nsegs = 0;
    auto cube = [&](int k) { return (float*)half[k].data(); };
    auto hits = [&](int k) { return half[k].data() + cw; };
    auto fold = [&](const float* in, int pos, long long m0, int nc) {
        std::vector<float> span(in, in + (size_t)nc * nser * nprod);     // a copy of exactly the call's words: a read past them is seen
        launch(ncand_max, 2 * CF_TILE * 4, [&] {
            if (nprod == 1) candfold_fold_kernel<1>(span.data(), cube(cur), hits(cur), cand[act].data(), nser, nbin, W, nsubwin, pos, (unsigned)m0, nc);
            else candfold_fold_kernel<4>(span.data(), cube(cur), hits(cur), cand[act].data(), nser, nbin, W, nsubwin, pos, (unsigned)m0, nc);
        });
    };
    auto differs = [&](const void* got, size_t bytes) {
        std::vector<uint8_t> e(bytes);
        return fread(e.data(), 1, bytes, fe) != bytes || memcmp(e.data(), got, bytes) != 0;
    };
    const float* in = z.data();
    for (int ic = 0; ic < ncalls; ic++) {
        for (auto& s : sets)
            if (s.at == ic) {
                cand[act ^ 1] = s.tab;
                if (nwindows % NT == 0) { act ^= 1; n_ref = nwindows; pending = false; }
                else pending = true;
                have = true;
            }
        const int nc = calls[ic];
        if (!have || nc < 1 || nc > NT) return 3;
        const int pos = (int)(nwindows % NT), head = nc < NT - pos ? nc : (int)(NT - pos);
        fold(in, pos, nwindows - n_ref, head);
        if (pos + head == NT) {
            launch(ncand_max, (2 * (size_t)W + CF_REFINE_EXTRA) * 4, [&] {
                candfold_refine_kernel(cube(cur), hits(cur), cand[act].data(), rot.data(), zrot.data(), gain.data(), out.data(), (float*)(out.data() + ncand_max),
                                       nsub, nbin, nwidth, ntrial, izero);
            });
            int bad = 0;
            if (differs(cube(cur), cw * 4)) bad |= 1;
            if (differs(hits(cur), cw * 4)) bad |= 2;
            if (differs(out.data(), (size_t)ncand_max * 16)) bad |= 4;
            if (differs(out.data() + ncand_max, (size_t)ncand_max * nbin * 4)) bad |= 8;
            if (bad) {
                fprintf(stderr, "segment %d: cube / hits / records / profiles differ from the restatement (mask %d)\n", nsegs, bad);
                return 4 + bad;
            }
            out.assign(out.size(), CfRecord{-5.f, -5.f, -5, -5, -5, -5});
            cur ^= 1;
            { const size_t n = 2 * cw; size_t blocks = (n + 255) / 256; if (blocks > 7) blocks = 7;     // (a grid smaller than the words: the stride loop runs)
              launch((int)blocks, 0, [&] { candfold_clear_kernel(half[cur].data(), n); }); }
            if (pending) { act ^= 1; n_ref = nwindows + head; pending = false; }
            nsegs++;
            if (nc > head) fold(in + (size_t)head * nser * nprod, 0, nwindows + head - n_ref, nc - head);
        }
        in += (size_t)nc * nser * nprod;
        nwindows += nc;
    }
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) { fprintf(stderr, "the expectation holds more segments than the %d completed\n", nsegs); return 3; }
    fclose(fe);
    printf("%d\n", nsegs);
    return 0;
}
