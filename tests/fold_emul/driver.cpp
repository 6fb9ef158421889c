// Runs the kernels of csrc/fold_kernels.h on host threads, one work-group after another, with the grids and the arguments fold.hip
// launches them with for a list of operations on a fresh context: Run (fold_kernel with m0 = the count since the reference; the
// hits counted on this side with fold_bin, as xengFoldRun does), Dump (fold_dump_kernel with gpw and the grid of xengFoldDump; the
// hits go to the device's copy only for a normalising dump, which otherwise holds a pattern) and Reset (the fold_clear_kernel
// launch, the counts and the hits back to 0).  Every buffer has exactly the size fold.hip gives it (the input is a copy of exactly
// the call's windows): the address sanitizer sees a word read or written outside.  After every Run the profile, and after every
// Dump the output, the hits and the profile, must equal the expectation file (two NaN count as equal whatever their payload;
// exit status 4 + what differed otherwise).
#include "fold_kernels.h"
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx, gridDim;
pthread_barrier_t g_bar, g_wbar[4];
float* g_lds;
uint32_t g_slot[256];
using namespace xeng;

// a launch: 256 threads walk the grid together
static void launch(int gx, int gy, const std::function<void()>& kernel) {
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int b = 0; b < gx * gy; b++) {
            pthread_barrier_wait(&g_bar);
            threadIdx.x = t; blockIdx.x = b % gx; blockIdx.y = b / gx; gridDim.x = gx; gridDim.y = gy;
            kernel();
            pthread_barrier_wait(&g_bar);
        }
    });
    for (auto& x : th) x.join();
}

// floats equal bit for bit, or both NaN
static bool same_floats(const float* a, const float* b, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (memcmp(a + i, b + i, 4) != 0 && !(a[i] != a[i] && b[i] != b[i])) return false;
    return true;
}

struct Op { int kind, a, b, c; };       // 0: Run(a windows); 1: Dump(nfscr a, normalise b, clear c); 2: Reset

// in.bin:  i32 {npair, nfine, nwin, nbin, nprod, nops}, FoldOsc osc[npair] (32 bytes each), i32 rot[npair][nfine], f32 w[nfine],
//          i32 ops[nops][4], f32 x[the windows of the Runs in order][npair][nfine][4]
// exp.bin: per Run f32 prof[npair][nbin][nfine][nprod]; per Dump f32 out[npair][nprod][nfine / nfscr][nbin], u32 hits[npair][nbin]
//          as Dump returns them, f32 prof
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[6];
    if (!f || fread(h, 4, 6, f) != 6) return 2;
    const int npair = h[0], nfine = h[1], nwin = h[2], nbin = h[3], nprod = h[4], nops = h[5];
    if (nprod != 1 && nprod != 4) return 3;
    static_assert(sizeof(FoldOsc) == 32, "the oscillator's layout");
    std::vector<FoldOsc> osc(npair);
    std::vector<int> rot((size_t)npair * nfine);
    std::vector<float> w(nfine);
    std::vector<Op> ops(nops);
    if (fread(osc.data(), 32, npair, f) != (size_t)npair || fread(rot.data(), 4, rot.size(), f) != rot.size() || fread(w.data(), 4, nfine, f) != (size_t)nfine ||
        fread(ops.data(), 16, nops, f) != (size_t)nops)
        return 2;
    for (int r : rot)
        if (r < 0 || r >= nbin) return 3;
    size_t total = 0;
    for (auto& o : ops)
        if (o.kind == 0) total += o.a;
    const size_t NC = (size_t)npair * nfine;
    std::vector<float> xin(total * NC * 4);
    if (fread(xin.data(), 4, xin.size(), f) != xin.size()) return 2;
    fclose(f);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe) return 2;

    // the context's state as Initialize and the setters leave it, each piece at its exact size
    const size_t nwords = NC * nbin * nprod;
    std::vector<float> prof(nwords, 0.f), expf;
    std::vector<uint32_t> hits((size_t)npair * nbin, 0u), hits_dev(hits.size(), 0xA5A5A5A5u), exph(hits.size());
    long long nwindows = 0;
    const long long n_ref = 0;
    pthread_barrier_init(&g_bar, nullptr, 256);
    auto prof_differs = [&] {
        expf.resize(nwords);
        return fread(expf.data(), 4, nwords, fe) != nwords || !same_floats(prof.data(), expf.data(), nwords);
    };
    const float* in = xin.data();
    int ndumps = 0;
    for (int io = 0; io < nops; io++) {
        const Op& o = ops[io];
        int bad = 0;
        if (o.kind == 0) {
            const int nc = o.a;
            if (nc < 1 || nc > nwin) return 3;
            std::vector<float> span(in, in + (size_t)nc * NC * 4);      // a copy of exactly the call's words: a read past them is seen
            const long long m0 = nwindows - n_ref;
            launch((int)(((size_t)nfine * nprod + 255) / 256), npair, [&] {
                if (nprod == 1) fold_kernel<1>(span.data(), prof.data(), osc.data(), npair, nfine, nbin, (unsigned)m0, nc);
                else fold_kernel<4>(span.data(), prof.data(), osc.data(), npair, nfine, nbin, (unsigned)m0, nc);
            });
            for (int p = 0; p < npair; p++) {
                if (!osc[p].active) continue;
                for (int i = 0; i < nc; i++) hits[(size_t)p * nbin + fold_bin(osc[p], (uint64_t)(m0 + i), (uint32_t)nbin)]++;
            }
            nwindows += nc;
            in += (size_t)nc * NC * 4;
            if (prof_differs()) bad |= 4;
        } else if (o.kind == 1) {
            const int nfscr = o.a, normalise = o.b, clear = o.c;
            if (nfscr < 1 || nfine % nfscr) return 3;
            if (normalise) hits_dev = hits;
            const int gpw = nfscr >= FOLD_QC ? 1 : FOLD_QC / nfscr;
            const long long ngroups = nfine / nfscr, ngb = (ngroups + gpw - 1) / gpw, nbt = (nbin + FOLD_BT - 1) / FOLD_BT;
            std::vector<float> out((size_t)npair * nprod * ngroups * nbin, -5.f), expo(out.size());
            launch((int)(ngb * nbt), npair, [&] {
                if (nprod == 1) fold_dump_kernel<1>(prof.data(), osc.data(), rot.data(), w.data(), hits_dev.data(), out.data(), nfine, nbin, nfscr, gpw, normalise ? 1 : 0, clear ? 1 : 0);
                else fold_dump_kernel<4>(prof.data(), osc.data(), rot.data(), w.data(), hits_dev.data(), out.data(), nfine, nbin, nfscr, gpw, normalise ? 1 : 0, clear ? 1 : 0);
            });
            if (fread(expo.data(), 4, expo.size(), fe) != expo.size() || !same_floats(out.data(), expo.data(), out.size())) bad |= 1;
            if (fread(exph.data(), 4, exph.size(), fe) != exph.size() || memcmp(exph.data(), hits.data(), hits.size() * 4) != 0) bad |= 2;
            if (clear) std::fill(hits.begin(), hits.end(), 0u);
            if (prof_differs()) bad |= 4;
            ndumps++;
        } else {
            const size_t blocks = (nwords + 255) / 256;
            launch((int)(blocks < 65536 ? blocks : 65536), 1, [&] { fold_clear_kernel(prof.data(), nwords); });
            std::fill(hits.begin(), hits.end(), 0u);
            nwindows = 0;
        }
        if (bad) {
            fprintf(stderr, "operation %d (kind %d): the dump's output (1) / the hits (2) / the profile (4) differ from the restatement (mask %d)\n", io, o.kind, bad);
            return 4 + bad;
        }
    }
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) { fprintf(stderr, "the expectation holds more than the %d operations\n", nops); return 3; }
    fclose(fe);
    printf("%d\n", ndumps);
    return 0;
}
