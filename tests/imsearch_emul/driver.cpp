// Runs the two kernels of csrc/imsearch_kernels.h on host threads, integration after integration, the way imsearch.hip launches
// them: the compact tables of the groups in use, the slots and the live counts are formed as xengImsearchRun forms them.  The ingest
// kernel has no barrier and runs lane after lane on one thread; a work-group of the search kernel is 256 threads that live for the
// whole run.  The LDS starts as NaN before every work-group: nothing may depend on what it held.  Every buffer is a heap block of its
// exact size -- each integration's image one of its own -- so the address sanitizer this is built with sees any access outside it;
// the planes start as a pattern no record has, so a word nobody wrote shows.  The rings start as a finite pattern: what lies before
// the live range must be left out by index.  imsearch_kernels_host.h is that header with its one `__shared__` line replaced (the
// test writes it).
#include "imsearch_kernels_host.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar;
uint8_t* g_lds;
using namespace xeng;
static void* alloc16(size_t bytes) {        // 16-byte aligned, exactly `bytes` long
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1)) abort();
    return p;
}
// args: npix ngroup ndm nwidth nstat nint n_w in.bin out.bin ; in: delays i32[ndm][ngroup], weights f32[ngroup] (in force from
// integration 0), weights f32[ngroup] (set when n_w integrations had been taken; n_w < 0: never), images f32[nint][ngroup][4][npix]
// out: records [nint][npix], then c, m, v f32[ngroup][npix] of the last complete block
int main(int argc, char** argv) {
    if (argc != 10) return 2;
    const int npix = atoi(argv[1]), ngroup = atoi(argv[2]), ndm = atoi(argv[3]), nwidth = atoi(argv[4]), nstat = atoi(argv[5]), nint = atoi(argv[6]),
              n_set = atoi(argv[7]);
    const int npitch = (npix + 3) & ~3, T = (1 << (nwidth - 1)) - 1;
    const size_t nimg = (size_t)ngroup * 4 * npix, plane = (size_t)ngroup * npix;
    std::vector<int> delays((size_t)ndm * ngroup);
    std::vector<float> w0(ngroup), w1(ngroup);
    FILE* f = fopen(argv[8], "rb");
    if (!f || fread(delays.data(), 4, delays.size(), f) != delays.size() || fread(w0.data(), 4, ngroup, f) != (size_t)ngroup ||
        fread(w1.data(), 4, ngroup, f) != (size_t)ngroup)
        return 2;
    std::vector<float*> img(nint);
    for (int n = 0; n < nint; n++) {
        img[n] = (float*)alloc16(nimg * 4);
        if (fread(img[n], 4, nimg, f) != nimg) return 2;
    }
    fclose(f);
    int S = 0;
    for (int s : delays) S = s > S ? s : S;
    const size_t nu = (size_t)(S + 1) * ngroup * npitch, nz = (size_t)(T + 1) * ndm * npitch;
    float* state = (float*)alloc16(IS_NSTATE * plane * 4);
    float* U = (float*)alloc16(nu * 4);
    float* Z = (float*)alloc16(nz * 4);
    float2* out = (float2*)alloc16((size_t)nint * npix * 8);
    for (size_t i = 0; i < IS_NSTATE * plane; i++) state[i] = 0.f;
    for (size_t i = 0; i < nu; i++) U[i] = 3.f;
    for (size_t i = 0; i < nz; i++) Z[i] = 5.f;
    for (size_t i = 0; i < (size_t)nint * npix; i++) out[i] = make_float2(-777.f, -777.f);
    int *bk = nullptr, *gk = nullptr;           // (allocated by tables(): exactly nusedp entries a row, so a read past the padding shows)
    float* wk = nullptr;
    int nused = 0;
    float kappa = 0.f;
    auto tables = [&](const std::vector<float>& w) {
        double sum2 = 0.0;
        nused = 0;
        for (int g = 0; g < ngroup; g++) nused += w[g] != 0.f;
        const int nusedp = (nused + IS_CHUNK - 1) / IS_CHUNK * IS_CHUNK;
        free(bk); free(gk); free(wk);
        bk = (int*)malloc((size_t)ndm * nusedp * 4);
        gk = (int*)malloc((size_t)nusedp * 4);
        wk = (float*)malloc((size_t)nusedp * 4);
        int k = 0;
        for (int g = 0; g < ngroup; g++)
            if (w[g] != 0.f) {
                gk[k] = g; wk[k] = w[g]; k++;
                sum2 += (double)w[g] * (double)w[g];
            }
        for (; k < nusedp; k++) {
            gk[k] = gk[0]; wk[k] = 0.f;
        }
        kappa = (float)(1.0 / std::sqrt(sum2));
        for (int d = 0; d < ndm; d++)
            for (k = 0; k < nusedp; k++) bk[(size_t)d * nusedp + k] = k < nused ? S - delays[(size_t)d * ngroup + gk[k]] : 0;
    };
    tables(w0);
    const int ntile = (npitch + IS_TILE - 1) / IS_TILE, NT = 64 * IS_WAVES;
    const size_t nlds = (IS_WAVES - 1) * 2 * 64 * sizeof(float4);
    int n_w = 0;
    pthread_barrier_init(&g_bar, nullptr, NT);
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back([&, t] {
        for (int n = 0; n < nint; n++)
            for (int tile = 0; tile < ntile; tile++) {
                pthread_barrier_wait(&g_bar);
                if (t == 0) {
                    if (tile == 0) {
                        if (n == n_set) {
                            tables(w1);
                            n_w = n;
                        }
                        for (int g = 0; g < ngroup; g++)
                            for (int bx = 0; bx < ntile; bx++)
                                for (int l = 0; l < 64; l++) {
                                    threadIdx.x = l; blockIdx.x = bx; blockIdx.y = g;
                                    imsearch_ingest_kernel(img[n], state, U, npix, npitch, ngroup, nstat, 1.0f / (float)nstat, n % nstat, n >= nstat,
                                                           n % (S + 1));
                                }
                    }
                    free(g_lds);
                    g_lds = (uint8_t*)alloc16(nlds);
                    memset(g_lds, 0xFF, nlds);      // NaN: whatever was there must not matter
                }
                pthread_barrier_wait(&g_bar);
                threadIdx.x = t; blockIdx.x = tile; blockIdx.y = 0;
                const int since = n - n_w;
                const int zl = since < T ? since : T;
                float2* o = out + (size_t)n * npix;
#define SEARCH(NW) imsearch_search_kernel<NW>(U, Z, bk, gk, wk, o, npix, npitch, ngroup, ndm, nused, nstat, S, n, n % (S + 1), n % (T + 1), zl, kappa)
                switch (nwidth) {
                    case 1: SEARCH(1); break;
                    case 2: SEARCH(2); break;
                    case 3: SEARCH(3); break;
                    case 4: SEARCH(4); break;
                    case 5: SEARCH(5); break;
                    default: SEARCH(6); break;
                }
            }
    });
    for (auto& t : th) t.join();
    free(g_lds);
    f = fopen(argv[9], "wb");
    fwrite(out, 8, (size_t)nint * npix, f);
    fwrite(state + IS_DC * plane, 4, plane, f);
    fwrite(state + IS_DM * plane, 4, plane, f);
    fwrite(state + IS_DV * plane, 4, plane, f);
    fclose(f);
    for (float* p : img) free(p);
    free(state); free(U); free(Z); free(out); free(bk); free(gk); free(wk);
    return 0;
}
