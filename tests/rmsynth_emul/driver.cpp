// Runs the kernels of csrc/rmsynth_kernels.h on host threads, one work-group after another, with the grids, the LDS bytes and the
// arguments rmsynth.hip launches them with for one call: base, contract, pick, profile.  The list of used channels and the masks'
// counts are formed here as xengRmsynthSetTable and xengRmsynthSetMasks form them.  The dynamic LDS starts as NaN before every
// work-group and has exactly the launch's words.  rmsynth_kernels_host.h is the header with its `extern __shared__` lines turned
// into a pointer to g_lds (the test writes it).  Every buffer has exactly the size rmsynth.hip gives it, the list of used channels
// exactly nused words: the address sanitizer sees a word read or written outside.  The baselines, the partials, spec and the picked
// depths start as NaN (an int of 0x7FC00000 in the depths), the output as bytes of 0xCD.  The call runs twice over the same state:
// every byte of the output (but for the sign and payload of a NaN) must equal the expectation file both times (exit status 4 otherwise), and the input must be unchanged.
#include "rmsynth_kernels_host.h"
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

// in.bin:  i32 {npair, nchg, nbin, nphi, feeds}, f32 T[nchg][nphi][2], f32 w[nchg], u8 use[nchg], u8 off[npair][nbin],
//          u8 on[npair][nbin], u8 active[npair], f32 X[npair][4][nchg][nbin]
// exp.bin: the output's bytes
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[5];
    if (!f || fread(h, 4, 5, f) != 5) return 2;
    const int npair = h[0], nchg = h[1], nbin = h[2], nphi = h[3], feeds = h[4];
    if (npair < 1 || nchg < 1 || nbin < 1 || nbin > 65536 || nphi < 1 || nphi > 4096 || (feeds != 0 && feeds != 1)) return 3;
    std::vector<float> T((size_t)nchg * nphi * 2), w(nchg), X((size_t)npair * 4 * nchg * nbin);
    std::vector<unsigned char> use(nchg), off((size_t)npair * nbin), on((size_t)npair * nbin), active(npair);
    if (!rd(f, T) || !rd(f, w) || !rd(f, use) || !rd(f, off) || !rd(f, on) || !rd(f, active) || !rd(f, X)) return 2;
    fclose(f);
    // the context's state as Initialize, SetTable and SetMasks leave it, each piece at its exact size
    const int nrun = (nbin + RM_TILE - 1) / RM_TILE;
    std::vector<int> gl, cnt((size_t)npair * 2, 0);
    for (int g = 0; g < nchg; g++)
        if (use[g]) gl.push_back(g);
    const int nused = (int)gl.size();
    for (int p = 0; p < npair; p++)
        for (int b = 0; b < nbin; b++) {
            cnt[2 * p] += on[(size_t)p * nbin + b] != 0;
            cnt[2 * p + 1] += off[(size_t)p * nbin + b] != 0;
        }
    std::vector<float> base((size_t)npair * 4 * nchg, NAN), part((size_t)npair * nrun * nphi, NAN), spec((size_t)npair * nphi, NAN);
    std::vector<int> kbest(npair, 0x7FC00000);
    const size_t spec_off = (size_t)npair * sizeof(RmRecord), prof_off = spec_off + (size_t)npair * nphi * 4, out_bytes = prof_off + (size_t)npair * 16 * nbin;
    std::vector<uint8_t> e(out_bytes);
    FILE* fe = fopen(argv[2], "rb");
    if (!fe || fread(e.data(), 1, out_bytes, fe) != out_bytes) return 2;
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) return 3;
    fclose(fe);
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    const std::vector<float> X0 = X;
    for (int call = 0; call < 2; call++) {
        std::vector<uint8_t> out(out_bytes, 0xCD);
        launch((int)(((long long)npair * nchg + 3) / 4), 1, 1, RM_BASE_LDS_BYTES,
               [&] { rmsynth_base_kernel(X.data(), off.data(), use.data(), active.data(), cnt.data(), base.data(), npair, nchg, nbin, feeds); });
        launch((nphi + RM_TILE - 1) / RM_TILE, nrun, npair, RM_CONTRACT_LDS_BYTES, [&] {
            rmsynth_contract_kernel(X.data(), T.data(), gl.data(), base.data(), on.data(), active.data(), part.data(), nused, nchg, nbin, nphi, feeds);
        });
        launch(npair, 1, 1, RM_PICK_LDS_BYTES, [&] {
            rmsynth_pick_kernel(part.data(), active.data(), cnt.data(), spec.data(), kbest.data(), (RmRecord*)out.data(), (float*)(out.data() + spec_off), nrun, nphi);
        });
        launch((nbin + RM_THREADS - 1) / RM_THREADS, npair, 1, 0, [&] {
            rmsynth_profile_kernel(X.data(), T.data(), w.data(), gl.data(), base.data(), active.data(), kbest.data(), (float*)(out.data() + prof_off), nused, nchg,
                                   nbin, nphi, feeds);
        });
        if (memcmp(X.data(), X0.data(), X.size() * 4) != 0) {
            fprintf(stderr, "call %d: the input was written\n", call);
            return 4;
        }
        // byte for byte, but for a NaN's sign and payload in the float words behind the records, which the contract leaves open
        size_t i = 0;
        for (; i < spec_off && e[i] == out[i]; i++) {}
        for (; i >= spec_off && i < out_bytes; i += 4) {
            float a, b;
            memcpy(&a, &e[i], 4);
            memcpy(&b, &out[i], 4);
            if (memcmp(&a, &b, 4) != 0 && !(a != a && b != b)) break;
        }
        if (i < out_bytes) {
            fprintf(stderr, "call %d: the output differs from the restatement at byte %zu (spec begins at %zu, the profile at %zu)\n", call, i, spec_off, prof_off);
            return 4;
        }
    }
    printf("%d\n", nused);
    return 0;
}
