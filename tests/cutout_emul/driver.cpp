// Runs the kernels of csrc/cutout_kernels.h (and dedisp_kernels.h's ingest) on host threads, one work-group after another, with the
// grids, the LDS bytes and the arguments cutout.hip launches them with for a run of calls from a fresh context with a delay table:
// the ingest, and on a call that serves the partials, the row scores and the pick.  What a call serves is decided here from the
// counts as xengCutoutRun decides it.  The dynamic LDS starts as NaN before every work-group and has exactly the launch's words.
// cutout_kernels_host.h is the header with its `extern __shared__` lines turned into a pointer to g_lds (the test writes it).
// Every buffer has exactly the size cutout.hip gives it (the input is a copy of exactly the call's windows): the address sanitizer
// sees a word read or written outside.  The ring and the row records start as NaN, the output as bytes of 0xCD before every call,
// and a Reset changes the host's counts only, as xengCutoutReset does: a value used from before window 0 shows.  After every call the
// ids served and expired and, on a serving call, every byte of the output must equal the expectation file (exit status 4 otherwise).
#include "cutout_kernels_host.h"
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

struct Req { int id, pair; long long n_c; int ic, dstep; };
struct Pending { Req q; long long first, last; };
struct Event { int at, kind; std::vector<float> w; };       // kind 0: SetWeights(w), 1: Reset

// in.bin:  i32 {npair, nfine, nwin, ndmf, nhist, nband, nt, tscr, ndmc, nwidth, nreq_max, ncalls, nreq, nevents}, f32 k_mad,
//          i32 calls[ncalls], i32 delays[ndmf][nfine], per request i32 at (given before call `at`) and the 24 bytes of xengCutoutReq,
//          per event i32 {at, kind}, f32 w[nfine]; f32 x[sum calls][npair][nfine][4]
// exp.bin: per call i32 nserved, ids, i32 nexpired, ids and, when nserved > 0, the output's bytes over 0xCD
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[14];
    float k_mad;
    if (!f || fread(h, 4, 14, f) != 14 || fread(&k_mad, 4, 1, f) != 1) return 2;
    const int npair = h[0], nfine = h[1], nwin = h[2], ndmf = h[3], nhist = h[4], nband = h[5], nt = h[6], tscr = h[7], ndmc = h[8], nwidth = h[9],
              nreq_max = h[10], ncalls = h[11], nreq = h[12], nevents = h[13];
    if (nband < 1 || nfine % nband || tscr < 1 || tscr > 64 || (tscr & (tscr - 1)) || nt < 16 || nt > 1024 || (nt & 1) || ndmc < 1 || ndmc > 256 ||
        nwidth < 1 || nwidth > CO_MAX_WIDTH || (1 << (nwidth - 1)) > nt / 2 || nreq_max < 1 || nreq_max > CO_MAX_REQ || nhist < nt * tscr)
        return 3;
    std::vector<int> calls(ncalls), delays((size_t)ndmf * nfine);
    if (fread(calls.data(), 4, ncalls, f) != (size_t)ncalls || fread(delays.data(), 4, delays.size(), f) != delays.size()) return 2;
    std::vector<int> req_at(nreq);
    std::vector<Req> reqs(nreq);
    static_assert(sizeof(Req) == 24, "xengCutoutReq");
    for (int k = 0; k < nreq; k++)
        if (fread(&req_at[k], 4, 1, f) != 1 || fread(&reqs[k], 24, 1, f) != 1) return 2;
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
    const int ntu = nt * tscr, L = nhist + nwin, c = ndmc / 2;
    int tshift = 0;
    while ((1 << tshift) < tscr) tshift++;
    std::vector<int> smax(ndmf, 0);
    for (int d = 0; d < ndmf; d++)
        for (int q = 0; q < nfine; q++) {
            const int s = delays[(size_t)d * nfine + q];
            if (s < 0 || s > nhist - ntu) return 3;
            if (s > smax[d]) smax[d] = s;
        }
    CutoutRho rho = {};
    for (int iw = 0; iw < nwidth; iw++) rho.rho[iw] = (float)std::pow(2.0, -0.5 * iw);
    std::vector<float> ring(NC * L, NAN), w(nfine, 1.f);
    std::vector<CutoutRow> rowrec((size_t)nreq_max * ndmc, CutoutRow{NAN, 0x5A5A5A5Au, NAN, NAN});
    const size_t rec_bytes = (size_t)nreq_max * sizeof(CutoutRecord), out_bytes = rec_bytes + (size_t)nreq_max * 4 * nt * ((size_t)nband + ndmc);
    std::vector<Pending> pending;
    long long nwindows = 0;
    int nserving = 0;
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    const float4* in = xin.data();
    for (int ic = 0; ic < ncalls; ic++) {
        for (auto& e : events)
            if (e.at == ic) {
                if (e.kind == 0) w = e.w;
                else { nwindows = 0; pending.clear(); }
            }
        for (int k = 0; k < nreq; k++)
            if (req_at[k] == ic) {
                const Req& q = reqs[k];
                if (q.pair < 0 || q.pair >= npair || q.ic < 0 || q.ic >= ndmf || q.n_c < 0 || q.dstep < 1) return 3;
                int S = 0;
                for (int i = 0; i < ndmc; i++) {
                    const long long d = (long long)q.ic + (long long)(i - c) * q.dstep;
                    if (d >= 0 && d < ndmf && smax[(size_t)d] > S) S = smax[(size_t)d];
                }
                Pending pe{q, q.n_c - ntu / 2, 0};
                pe.last = pe.first + ntu - 1 + S;
                pending.push_back(pe);
            }
        const int nc = calls[ic];
        if (nc < 1 || nc > nwin) return 3;
        std::vector<float4> span(in, in + (size_t)nc * NC);     // a copy of exactly the call's words: a read past them is seen
        std::vector<uint8_t> out(out_bytes, 0xCD);
        const long long n0 = nwindows, n = n0 + nc;
        CutoutSlots sl = {};
        std::vector<Pending> keep;
        std::vector<int> served, expired;
        int r = 0;
        for (const Pending& pe : pending) {
            if (pe.first < n - nhist) expired.push_back(pe.q.id);
            else if (pe.last < n && r < nreq_max) {
                sl.id[r] = pe.q.id; sl.pair[r] = pe.q.pair; sl.ic[r] = pe.q.ic; sl.dstep[r] = pe.q.dstep;
                sl.slot0[r] = (int)(((pe.first % L) + L) % L);
                sl.a0[r] = pe.first < (1LL << 30) ? (int)pe.first : (1 << 30);
                served.push_back(pe.q.id);
                r++;
            } else keep.push_back(pe);
        }
        pending.swap(keep);
        launch((nfine + DD_TILE - 1) / DD_TILE, npair, (nc + DD_TILE - 1) / DD_TILE, 0,
               [&] { dedisp_ingest_kernel<1>(span.data(), ring.data(), npair, nfine, L, (int)(n0 % L), nc); });
        if (r) {
            float* W = (float*)(out.data() + rec_bytes);
            float* P = W + (size_t)nreq_max * nband * nt;
            launch((ntu + CO_THREADS - 1) / CO_THREADS, ndmc, r, CO_PARTIALS_LDS_BYTES,
                   [&] { cutout_partials_kernel(ring.data(), delays.data(), w.data(), sl, W, P, nfine, L, ndmf, nband, nt, tshift, ndmc); });
            launch(ndmc, r, 1, cutout_score_lds_bytes(nt), [&] { cutout_score_kernel(P, sl, rowrec.data(), ndmf, ndmc, nt, nwidth, k_mad, rho); });
            launch(nreq_max, 1, 1, CO_PICK_LDS_BYTES, [&] { cutout_pick_kernel(rowrec.data(), sl, (CutoutRecord*)out.data(), ndmc, r); });
            nserving++;
        }
        auto ids_differ = [&](const std::vector<int>& got) {
            int ne = -1;
            if (fread(&ne, 4, 1, fe) != 1 || ne != (int)got.size()) return true;
            std::vector<int> e(ne);
            return (ne && fread(e.data(), 4, ne, fe) != (size_t)ne) || e != got;
        };
        int bad = 0;
        if (ids_differ(served)) bad |= 1;
        if (!bad && ids_differ(expired)) bad |= 2;
        if (!bad && r) {
            std::vector<uint8_t> e(out_bytes);
            if (fread(e.data(), 1, out_bytes, fe) != out_bytes) bad |= 4;
            else if (memcmp(e.data(), out.data(), out_bytes) != 0) {
                size_t i = 0;
                while (e[i] == out[i]) i++;
                fprintf(stderr, "call %d: the output differs from the restatement at byte %zu (records end at %zu, waterfalls at %zu)\n", ic, i, rec_bytes,
                        rec_bytes + (size_t)nreq_max * nband * nt * 4);
                bad |= 4;
            }
        }
        if (bad) {
            fprintf(stderr, "call %d (windows %lld + %d): served / expired / output differ from the restatement (mask %d)\n", ic, n0, nc, bad);
            return 4 + bad;
        }
        in += (size_t)nc * NC;
        nwindows = n;
    }
    uint8_t more;
    if (fread(&more, 1, 1, fe) == 1) { fprintf(stderr, "the expectation holds more than the %d calls\n", ncalls); return 3; }
    fclose(fe);
    printf("%d\n", nserving);
    return 0;
}
