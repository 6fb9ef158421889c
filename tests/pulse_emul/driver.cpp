// Runs the kernel of csrc/pulse_kernels.h on host threads, one work-group after another, with the grid, the LDS bytes and the
// arguments pulse.hip launches it with for a run of calls from a fresh context: rows = max(T + 2 nc, 16), the clamped n0, head and
// pos0 as pulse_launch forms them, rho and r_nstat as xengPulseInitialize does.  The dynamic LDS starts as NaN before every
// work-group and has exactly the launch's words.  pulse_kernels_host.h is the header with its `extern __shared__` line turned into
// a pointer to g_lds (the test writes it).  Every buffer has exactly the size pulse.hip gives it (the input is a copy of exactly the
// call's windows): the address sanitizer sees a word read or written outside.  The state and the y ring start as NaN, and a Reset
// changes the host's count only, as xengPulseReset does: a value used from before window 0 shows.  After every call the records,
// and after a call that completes a block the seven state rows, must equal the expectation file (two NaN count as equal whatever
// their payload; exit status 4 + what differed otherwise).
#include "pulse_kernels_host.h"
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
    g_ldsbuf.assign(lds_bytes / 4, NAN);        // (exactly the launch's words: the address sanitizer sees one more)
    g_lds = g_ldsbuf.data();
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int b = 0; b < gx; b++) {
            if (t == 0) for (auto& v : g_ldsbuf) v = NAN;
            pthread_barrier_wait(&g_bar);
            threadIdx.x = t; blockIdx.x = b; gridDim.x = gx;
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

// in.bin:  i32 {nser, nwin, nprod, nwidth, nstat, ncalls, nresets}, i32 calls[ncalls], i32 resets[nresets] (a Reset before that
//          call), f32 x[sum calls][nser][nprod]
// exp.bin: per call {f32 snr, i32 n, i32 iw, f32 B}[nser] and, when the call completed a block, f32 state[7][nser]
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[7];
    if (!f || fread(h, 4, 7, f) != 7) return 2;
    const int nser = h[0], nwin = h[1], nprod = h[2], nwidth = h[3], nstat = h[4], ncalls = h[5], nresets = h[6];
    if ((nprod != 1 && nprod != 4) || nwidth < 1 || nwidth > 8 || nstat < 2 || (1 << (nwidth - 1)) > nstat) return 3;
    std::vector<int> calls(ncalls), resets(nresets);
    if (fread(calls.data(), 4, ncalls, f) != (size_t)ncalls || fread(resets.data(), 4, nresets, f) != (size_t)nresets) return 2;
    size_t total = 0;
    for (int c : calls) total += c;
    std::vector<float> xin(total * nser * nprod);
    if (fread(xin.data(), 4, xin.size(), f) != xin.size()) return 2;
    fclose(f);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe) return 2;

    // the context's state as Initialize leaves it, each piece at its exact size
    const int T = (1 << (nwidth - 1)) - 1, L = T + nwin;
    if (T + 2 * nwin > 256) return 3;
    std::vector<float> state((size_t)PS_NSTATE * nser, NAN), tail((size_t)L * nser, NAN), rho(nwidth);
    for (int iw = 0; iw < nwidth; iw++) rho[iw] = (float)std::ldexp(iw & 1 ? 0.70710678118654752440 : 1.0, -(iw >> 1));
    const float r_nstat = 1.0f / (float)nstat;
    long long nwindows = 0;
    int nblocks = 0;
    pthread_barrier_init(&g_bar, nullptr, 256);
    const float* in = xin.data();
    for (int ic = 0; ic < ncalls; ic++) {
        for (int r : resets)
            if (r == ic) nwindows = 0;
        const int nc = calls[ic];
        if (nc < 1 || nc > nwin) return 3;
        std::vector<float> span(in, in + (size_t)nc * nser * nprod);    // a copy of exactly the call's words: a read past them is seen
        std::vector<float4> out(nser, float4{-5.f, -5.f, -5.f, -5.f}), exp(nser);
        const int rows = T + 2 * nc < 16 ? 16 : T + 2 * nc;
        const int n0 = nwindows < (1LL << 30) ? (int)nwindows : (1 << 30);
        const int head = (int)(nwindows % L), pos0 = (int)(nwindows % nstat);
        launch((nser + PS_SERIES - 1) / PS_SERIES, (size_t)rows * PS_SERIES * sizeof(float), [&] {
            if (nprod == 1) pulse_search_kernel<1>(span.data(), state.data(), tail.data(), rho.data(), out.data(), nser, nc, nwidth, nstat, r_nstat, L, head, n0, pos0);
            else pulse_search_kernel<4>(span.data(), state.data(), tail.data(), rho.data(), out.data(), nser, nc, nwidth, nstat, r_nstat, L, head, n0, pos0);
        });
        int bad = 0;
        if (fread(exp.data(), 16, nser, fe) != (size_t)nser) return 2;
        for (int s = 0; s < nser && !bad; s++) {
            if (!same_floats(&out[s].x, &exp[s].x, 1) || !same_floats(&out[s].w, &exp[s].w, 1)) bad |= 1;
            if (memcmp(&out[s].y, &exp[s].y, 8) != 0) bad |= 2;
            if (bad) fprintf(stderr, "call %d, series %d: {%.9g, %d, %d, %.9g}, expected {%.9g, %d, %d, %.9g}\n", ic, s, out[s].x, __float_as_int(out[s].y),
                             __float_as_int(out[s].z), out[s].w, exp[s].x, __float_as_int(exp[s].y), __float_as_int(exp[s].z), exp[s].w);
        }
        if (pos0 + nc >= nstat) {
            std::vector<float> es(state.size());
            if (fread(es.data(), 4, es.size(), fe) != es.size()) return 2;
            for (int k = 0; k < PS_NSTATE; k++)
                if (!same_floats(&state[(size_t)k * nser], &es[(size_t)k * nser], nser)) {
                    bad |= 4;
                    fprintf(stderr, "call %d: state row %d differs from the restatement\n", ic, k);
                }
            nblocks++;
        }
        if (bad) return 4 + bad;                // 1: snr or B, 2: (n, iw), 4: the state
        in += (size_t)nc * nser * nprod;
        nwindows += nc;
    }
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) { fprintf(stderr, "the expectation holds more than the %d calls\n", ncalls); return 3; }
    fclose(fe);
    printf("%d\n", nblocks);
    return 0;
}
