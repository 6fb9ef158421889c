// Runs the kernels of csrc/toa_kernels.h on host threads, one work-group after another, with the grids, the LDS bytes and the
// arguments toa.hip launches them with for one call: scrunch, band, base, DFT, correlate, pick.  The lists of used groups and the
// mask's counts are formed here as xengToaSetBands and xengToaSetMask form them.  The dynamic LDS starts as NaN before every
// work-group and has exactly the launch's words.  toa_kernels_host.h is the header with its `extern __shared__` lines turned into a
// pointer to g_lds (the test writes it).  Every buffer has exactly the size toa.hip gives it, the list of used groups exactly its
// words: the address sanitizer sees a word read or written outside.  base and var start as NaN, the output as bytes of 0xCD.  The
// call runs twice over the same state: every byte of the output (but for the sign and payload of a NaN) must equal the expectation
// file both times (exit status 4 otherwise), and the input must be unchanged.
#include "toa_kernels_host.h"
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
static void launch(int gx, int gy, int gz, size_t lds_bytes, const std::function<void()>& kernel) {
    g_ldsbuf.assign(lds_bytes / 4, NAN);        // (exactly the launch's words: the address sanitizer sees one more)
    g_lds = g_ldsbuf.data();
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int b = 0; b < gx * gy * gz; b++) {
            if (t == 0) for (auto& v : g_ldsbuf) v = NAN;
            pthread_barrier_wait(&g_bar);
            threadIdx.x = t; blockIdx.x = b % gx; blockIdx.y = b / gx % gy; blockIdx.z = b / gx / gy;
            gridDim.x = gx; gridDim.y = gy; gridDim.z = gz;
            kernel();
            pthread_barrier_wait(&g_bar);
        }
    });
    for (auto& x : th) x.join();
}

template <class V> static bool rd(FILE* f, V& v) { return v.empty() || fread(v.data(), sizeof(v[0]), v.size(), f) == v.size(); }

// in.bin:  i32 {npair, nprod, nchg, nbin, nsub, nharm, nlag}, i32 edges[nsub+1], f32 w[nchg], f32 D[nbin][nharm][2],
//          f32 L[nharm][nlag][2], f32 S[nrow][nharm][2], u8 off[npair][nbin], u8 active[npair], f32 X[npair][nprod][nchg][nbin]
// exp.bin: the output's bytes
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[7];
    if (!f || fread(h, 4, 7, f) != 7) return 2;
    const int npair = h[0], nprod = h[1], nchg = h[2], nbin = h[3], nsub = h[4], nharm = h[5], nlag = h[6];
    if (npair < 1 || (nprod != 1 && nprod != 4) || nchg < 1 || nbin < 1 || nbin > 16384 || nsub < 1 || nsub > 256 || nharm < 1 || nharm > (nbin - 1) / 2 ||
        nlag < 1 || nlag > 65536)
        return 3;
    const int nrow = npair * (nsub + 1);
    std::vector<int> edges(nsub + 1);
    std::vector<float> w(nchg), D((size_t)nbin * nharm * 2), L((size_t)nharm * nlag * 2), S((size_t)nrow * nharm * 2), X((size_t)npair * nprod * nchg * nbin);
    std::vector<unsigned char> off((size_t)npair * nbin), active(npair);
    if (!rd(f, edges) || !rd(f, w) || !rd(f, D) || !rd(f, L) || !rd(f, S) || !rd(f, off) || !rd(f, active) || !rd(f, X)) return 2;
    fclose(f);
    // the context's state as Initialize, SetBands and SetMask leave it, each piece at its exact size
    std::vector<int> gl, gs(nsub + 1, 0), cnt(npair, 0);
    for (int r = 0; r < nsub; r++) {
        if (edges[r] < 0 || edges[r] > edges[r + 1] || edges[r + 1] > nchg) return 3;
        gs[r] = (int)gl.size();
        for (int g = edges[r]; g < edges[r + 1]; g++)
            if (w[g] != 0.f) gl.push_back(g);
    }
    gs[nsub] = (int)gl.size();
    for (int p = 0; p < npair; p++)
        for (int b = 0; b < nbin; b++) cnt[p] += off[(size_t)p * nbin + b] != 0;
    std::vector<float> bv((size_t)nrow * 2, NAN);
    const size_t prof_off = (size_t)nrow * sizeof(ToaRecord), harm_off = prof_off + (size_t)nrow * nbin * 4, ccf_off = harm_off + (size_t)nrow * nharm * 8,
                 out_bytes = ccf_off + (size_t)nrow * nlag * 4;
    std::vector<uint8_t> e(out_bytes);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe || fread(e.data(), 1, out_bytes, fe) != out_bytes) return 2;
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) return 3;
    fclose(fe);
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    const std::vector<float> X0 = X;
    const int ntile = (nrow + TOA_ROWS - 1) / TOA_ROWS;
    for (int call = 0; call < 2; call++) {
        std::vector<uint8_t> out(out_bytes, 0xCD);
        ToaRecord* rec = (ToaRecord*)out.data();
        float* P = (float*)(out.data() + prof_off);
        float* PH = (float*)(out.data() + harm_off);
        float* ccf = (float*)(out.data() + ccf_off);
        launch((nbin + 4 * TOA_THREADS - 1) / (4 * TOA_THREADS), nsub, npair, 0, [&] {
            if (nprod == 4)
                toa_scrunch_kernel<4>(X.data(), w.data(), gl.data(), gs.data(), active.data(), P, nchg, nbin, nsub);
            else
                toa_scrunch_kernel<1>(X.data(), w.data(), gl.data(), gs.data(), active.data(), P, nchg, nbin, nsub);
        });
        launch((nbin + TOA_THREADS - 1) / TOA_THREADS, npair, 1, 0, [&] { toa_band_kernel(active.data(), P, nbin, nsub); });
        launch((nrow + 3) / 4, 1, 1, TOA_BASE_LDS_BYTES, [&] { toa_base_kernel(P, off.data(), active.data(), cnt.data(), bv.data(), nrow, nbin, nsub); });
        launch(ntile, (nharm + TOA_THREADS - 1) / TOA_THREADS, 1, TOA_DFT_LDS_BYTES,
               [&] { toa_dft_kernel(P, bv.data(), D.data(), active.data(), PH, nrow, nbin, nsub, nharm); });
        launch(ntile, (nlag + TOA_THREADS - 1) / TOA_THREADS, 1, TOA_CORR_LDS_BYTES,
               [&] { toa_corr_kernel(PH, S.data(), L.data(), active.data(), ccf, nrow, nsub, nharm, nlag); });
        launch(nrow, 1, 1, TOA_PICK_LDS_BYTES, [&] { toa_pick_kernel(ccf, bv.data(), gs.data(), active.data(), rec, nsub, nlag); });
        if (memcmp(X.data(), X0.data(), X.size() * 4) != 0) {
            fprintf(stderr, "call %d: the input was written\n", call);
            return 4;
        }
        // byte for byte, but for a NaN's sign and payload in the float words (the records' l is compared as it is), which the contract leaves open
        size_t i = 0;
        for (; i < out_bytes; i += 4) {
            if (i < prof_off && i % 16 == 0) {
                if (memcmp(&e[i], &out[i], 4) != 0) break;
                continue;
            }
            float a, b;
            memcpy(&a, &e[i], 4);
            memcpy(&b, &out[i], 4);
            if (memcmp(&a, &b, 4) != 0 && !(a != a && b != b)) break;
        }
        if (i < out_bytes) {
            fprintf(stderr, "call %d: the output differs from the restatement at byte %zu (P begins at %zu, PH at %zu, ccf at %zu)\n", call, i, prof_off, harm_off,
                    ccf_off);
            return 4;
        }
    }
    printf("%d\n", (int)gl.size());
    return 0;
}
