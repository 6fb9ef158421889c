// Runs the kernels of csrc/dedisp_kernels.h on host threads, one work-group after another, in the order and with the grids and
// arguments dedisp.hip launches them with for a run of calls from a fresh context with a delay table: the ingest, then the
// dedisperser with tshift, head and the clamped n0 as dedisp_launch forms them.  Every buffer has exactly the size dedisp.hip gives
// it (the input is a copy of exactly the call's windows, the output has exactly the call's words): the address sanitizer sees a
// word read or written outside.  The history ring starts as NaN, not as the zeros of SetDelays: a value used from before window 0
// shows in the output.  SetWeights replaces w; Reset changes the host's count only, as xengDedispReset does.  After every call the
// output must equal the bytes of the expectation file (exit status 4 otherwise).
#include "dedisp_kernels.h"
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar, g_wbar[4];
float* g_lds;
uint32_t g_slot[256];
using namespace xeng;

// a launch: 256 threads walk the grid together
static void launch(int gx, int gy, int gz, const std::function<void()>& kernel) {
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int b = 0; b < gx * gy * gz; b++) {
            pthread_barrier_wait(&g_bar);
            threadIdx.x = t; blockIdx.x = b % gx; blockIdx.y = b / gx % gy; blockIdx.z = b / gx / gy;
            kernel();
            pthread_barrier_wait(&g_bar);
        }
    });
    for (auto& x : th) x.join();
}

struct Event { int at, kind; std::vector<float> w; };       // kind 0: SetWeights(w), 1: Reset

template <int NPROD>
static void run_call(const float4* in, float* hist, const int* bt, const float* w, float* out, int npair, int nfine, int ndm, int L, int head,
                     long long nwindows, int nc) {
    launch((nfine + DD_TILE - 1) / DD_TILE, npair, (nc + DD_TILE - 1) / DD_TILE, [&] { dedisp_ingest_kernel<NPROD>(in, hist, npair, nfine, L, head, nc); });
    int tshift = 0;
    while (tshift < 6 && (1 << tshift) < nc) tshift++;
    const int TT = 1 << tshift, DD = 64 >> tshift;
    const long long tiles = (long long)((nc + TT - 1) / TT) * ((ndm + DD - 1) / DD);
    const int n0 = nwindows < (1LL << 30) ? (int)nwindows : (1 << 30);
    launch((int)tiles, npair, 1, [&] { dedisp_kernel<NPROD>(hist, bt, w, out, npair, nfine, ndm, L, head, n0, nc, tshift); });
}

// in.bin:  i32 {npair, nfine, nwin, ndm, max_delay, nprod, ncalls, nevents}, i32 calls[ncalls], i32 delays[ndm][nfine], per event
//          (given before call `at`) i32 {at, kind}, f32 w[nfine]; f32 x[sum calls][npair][nfine][4]
// exp.bin: per call f32 out[nc][npair][ndm][nprod]
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[8];
    if (!f || fread(h, 4, 8, f) != 8) return 2;
    const int npair = h[0], nfine = h[1], nwin = h[2], ndm = h[3], max_delay = h[4], nprod = h[5], ncalls = h[6], nevents = h[7];
    if (nprod != 1 && nprod != 4) return 3;
    std::vector<int> calls(ncalls), delays((size_t)ndm * nfine);
    if (fread(calls.data(), 4, ncalls, f) != (size_t)ncalls || fread(delays.data(), 4, delays.size(), f) != delays.size()) return 2;
    std::vector<Event> events(nevents);
    for (auto& e : events) {
        e.w.resize(nfine);
        if (fread(&e.at, 4, 1, f) != 1 || fread(&e.kind, 4, 1, f) != 1 || fread(e.w.data(), 4, nfine, f) != (size_t)nfine) return 2;
    }
    size_t total = 0;
    for (int c : calls) total += c;
    const size_t NC = (size_t)npair * nfine;
    std::vector<float4> xin(total * NC);
    if (fread(xin.data(), 16, xin.size(), f) != xin.size()) return 2;
    fclose(f);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe) return 2;

    // the context's state as Initialize and SetDelays leave it, each piece at its exact size
    const int L = max_delay + nwin;
    int S = 0;
    for (int s : delays) {
        if (s < 0 || s > max_delay) return 3;
        if (s > S) S = s;
    }
    std::vector<int> bt((size_t)nfine * ndm);
    for (int d = 0; d < ndm; d++)
        for (int q = 0; q < nfine; q++) bt[(size_t)q * ndm + d] = S - delays[(size_t)d * nfine + q];
    std::vector<float> hist(NC * nprod * L, NAN), w(nfine, 1.f);
    long long nwindows = 0;
    int head = 0;
    pthread_barrier_init(&g_bar, nullptr, 256);
    const float4* in = xin.data();
    for (int ic = 0; ic < ncalls; ic++) {
        for (auto& e : events)
            if (e.at == ic) {
                if (e.kind == 0) w = e.w;
                else nwindows = 0;
            }
        const int nc = calls[ic];
        if (nc < 1 || nc > nwin) return 3;
        std::vector<float4> span(in, in + (size_t)nc * NC);     // a copy of exactly the call's words: a read past them is seen
        std::vector<float> out((size_t)nc * npair * ndm * nprod, -5.f), exp(out.size());
        if (nprod == 1) run_call<1>(span.data(), hist.data(), bt.data(), w.data(), out.data(), npair, nfine, ndm, L, head, nwindows, nc);
        else run_call<4>(span.data(), hist.data(), bt.data(), w.data(), out.data(), npair, nfine, ndm, L, head, nwindows, nc);
        if (fread(exp.data(), 4, exp.size(), fe) != exp.size() || memcmp(exp.data(), out.data(), out.size() * 4) != 0) {
            size_t i = 0;
            while (i < out.size() && memcmp(&exp[i], &out[i], 4) == 0) i++;
            fprintf(stderr, "call %d: the output differs from the restatement (first at word %zu: %.9g, expected %.9g)\n", ic, i,
                    i < out.size() ? out[i] : 0.f, i < out.size() ? exp[i] : 0.f);
            return 4;
        }
        head = (head + nc) % L;
        nwindows += nc;
        in += (size_t)nc * NC;
    }
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) { fprintf(stderr, "the expectation holds more than the %d calls\n", ncalls); return 3; }
    fclose(fe);
    printf("%d\n", ncalls);
    return 0;
}
