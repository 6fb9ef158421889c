// Runs the kernels of csrc/accel_kernels.h on host threads, one work-group after another, in the order and with the arguments
// accel.hip launches them with for a run of calls from a reset: the ingest per call and, per completed segment, per batch of SB
// series and per trial the gathered mean and columns pass, plong's rows pass, untangle, whitening, sums and reduce on the batch's
// buffers, then the best over the trials.  Beside it, per completed segment and trial, the sequence of plong.hip (nstack = 1, one
// batch) on the segment resampled on the host: the two sets of trial records must be equal byte for byte (exit status 4 otherwise).
// The dynamic LDS starts as NaN before every work-group.  accel_kernels_host.h and plong_kernels_host.h are the two headers with
// their `extern __shared__` lines turned into a pointer to g_lds (the test writes them).  Every buffer has exactly the size
// accel.hip gives it: the address sanitizer sees a word read or written outside.
#include "accel_kernels_host.h"
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>
thread_local dim3e threadIdx, blockIdx;
pthread_barrier_t g_bar, g_wbar[4];
float* g_lds;
uint32_t g_slot[256];
static std::vector<float> g_ldsbuf;
using namespace xeng;

// a launch: 256 threads walk the grid together; LDS is NaN before every work-group
static void launch(int gx, int gy, size_t lds_bytes, const std::function<void()>& kernel) {
    g_ldsbuf.assign(lds_bytes ? lds_bytes / 4 : 1, NAN);     // (exactly the launch's words: the address sanitizer sees one more)
    g_lds = g_ldsbuf.data();
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++) th.emplace_back([&, t] {
        for (int by = 0; by < gy; by++)
            for (int bx = 0; bx < gx; bx++) {
                if (t == 0) for (auto& v : g_ldsbuf) v = NAN;
                pthread_barrier_wait(&g_bar);
                threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by;
                kernel();
                pthread_barrier_wait(&g_bar);
            }
    });
    for (auto& x : th) x.join();
}

static int ilog2(int v) { int l = 0; while ((1 << l) < v) l++; return l; }

// in.bin: i32 {nser, nprod, NT, nlevel, B, nband, SB, ncalls, has_mask, ntrial}, i32 kedge[nband + 1], i32 calls[ncalls],
//         f64 alpha[ntrial], u8 keep[NT/2] if has_mask, f32 z[sum calls][nser][nprod]
// out.bin: i32 nsegs, then of the last completed segment PlongRecord trec[ntrial][nser][nlevel][nband], the same from the plong
//          sequence on the host-resampled series, and AccelRecord out[nser][nlevel][nband]
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[10];
    if (!f || fread(h, 4, 10, f) != 10) return 2;
    const int nser = h[0], nprod = h[1], NT = h[2], nlevel = h[3], B = h[4], nband = h[5], SB = h[6], ncalls = h[7], has_mask = h[8], ntrial = h[9];
    const int N = NT / 2, LN = ilog2(N), LN1 = pl_ln1(LN), LN2 = LN - LN1, lb = ilog2(B), N1 = 1 << LN1, N2 = 1 << LN2;
    std::vector<int> kedge(nband + 1), calls(ncalls);
    std::vector<double> alpha(ntrial);
    if (fread(kedge.data(), 4, nband + 1, f) != (size_t)nband + 1 || fread(calls.data(), 4, ncalls, f) != (size_t)ncalls ||
        fread(alpha.data(), 8, ntrial, f) != (size_t)ntrial)
        return 2;
    std::vector<uint8_t> keep(N, 1);
    if (has_mask && fread(keep.data(), 1, N, f) != (size_t)N) return 2;
    for (auto& k : keep) k = k ? 1 : 0;
    size_t total = 0;
    for (int c : calls) total += c;
    std::vector<float> z(total * nser * nprod);
    if (fread(z.data(), 4, z.size(), f) != z.size()) return 2;
    fclose(f);
    int izero = -1;
    for (int a = ntrial - 1; a >= 0; a--)
        if (alpha[a] == 0.0) izero = a;
    std::vector<float> cnt(N / B, 0.f);
    for (int k = 1; k < N; k++) cnt[k / B] += (float)keep[k];
    auto table = [](size_t len) {
        std::vector<float2> t(len / 2);
        const double step = -2.0 * 3.14159265358979323846 / (double)len;
        for (size_t k = 0; k < len / 2; k++) t[k] = make_float2((float)std::cos(step * (double)k), (float)std::sin(step * (double)k));
        return t;
    };
    const std::vector<float2> tw = table(NT), tws = table(N), tw1 = table(N1), tw2 = table(N2);
    const size_t per = (size_t)nlevel * nband, nrec_all = (size_t)nser * per;
    // the accel engine's buffers
    std::vector<float> tbuf((size_t)nser * NT, -7.f), P((size_t)SB * N, -7.f), S((size_t)SB * N, -7.f);
    std::vector<float2> scr((size_t)SB * N, float2{-7.f, -7.f});
    std::vector<PlongRecord> part((size_t)SB * per * PL_NTILE, PlongRecord{-5.f, -5}), trec((size_t)ntrial * nrec_all, PlongRecord{-5.f, -5});
    std::vector<PlongMean> mv(SB, PlongMean{-7.f, -5});
    std::vector<AccelRecord> out(nrec_all, AccelRecord{-5.f, -5, -5, -5.f});
    // the plong engine's, one batch of nser series
    std::vector<float> zres((size_t)nser * NT), P2((size_t)nser * N), A2((size_t)nser * N);
    std::vector<float2> scr2((size_t)nser * N);
    std::vector<PlongRecord> part2(nrec_all * PL_NTILE), ref((size_t)ntrial * nrec_all, PlongRecord{-6.f, -6});
    std::vector<PlongMean> mv2(nser);
    pthread_barrier_init(&g_bar, nullptr, 256);
    for (auto& b : g_wbar) pthread_barrier_init(&b, nullptr, 64);
    auto ingest = [&](const float* in, int pos, int nc) {
        std::vector<float> span(in, in + (size_t)nc * nser * nprod);     // a copy of exactly the call's words: a read past them is seen
        launch((nser + PL_TILE - 1) / PL_TILE, (nc + PL_TILE - 1) / PL_TILE, 0, [&] {
            if (nprod == 1) plong_ingest_kernel<1>(span.data(), tbuf.data(), nser, NT, pos, nc);
            else plong_ingest_kernel<4>(span.data(), tbuf.data(), nser, NT, pos, nc);
        });
    };
    const int lr = pl_lrows(LN2), lw = pl_lwhite(lb);
    const size_t lds_cols = (size_t)N1 * PL_TC * 8, lds_rows = ((size_t)N2 << lr) * 8, lds_power = (size_t)PL_TC * (N1 + PL_PPAD) * 4, lds_white = (size_t)4 << lw;
    long long nwindows = 0;
    int nsegs = 0;
    const float* in = z.data();
    for (int nc : calls) {
        const int pos = (int)(nwindows % NT), head = nc < NT - pos ? nc : NT - pos;
        if (nc > NT) return 3;
        ingest(in, pos, head);
        if (pos + head == NT) {
            for (int s0 = 0; s0 < nser; s0 += SB) {
                const int ns = nser - s0 < SB ? nser - s0 : SB;
                const long long nrec = (long long)ns * (long long)per;
                for (int a = 0; a < ntrial; a++) {
                    const double al = alpha[a];
                    launch(ns, 1, 0, [&] { accel_mean_kernel(tbuf.data(), mv.data(), LN, s0, al); });
                    launch(N2 / PL_TC, ns, lds_cols, [&] { accel_cols_kernel(tbuf.data(), mv.data(), scr.data(), tw1.data(), LN1, LN2, s0, al); });
                    launch(N1 >> lr, ns, lds_rows, [&] { plong_rows_kernel(scr.data(), tws.data(), tw2.data(), LN1, LN2); });
                    launch(N2 / PL_TC, ns, lds_power, [&] { plong_power_kernel(scr.data(), tw.data(), P.data(), LN1, LN2); });
                    launch(1 << (LN - lw), ns, lds_white, [&] { plong_whiten_kernel(P.data(), S.data(), keep.data(), cnt.data(), mv.data(), LN, lb, 1, 0); });
                    launch(PL_NTILE, ns, 0, [&] { plong_sums_kernel(S.data(), kedge.data(), part.data(), LN, nlevel, nband, 0); });
                    launch((int)((nrec + 255) / 256), 1, 0,
                           [&] { plong_reduce_kernel(part.data(), trec.data() + (size_t)a * nrec_all + (size_t)s0 * per, nrec); });
                }
            }
            launch((int)((nrec_all + 255) / 256), 1, 0, [&] { accel_best_kernel(trec.data(), out.data(), (long long)nrec_all, ntrial, izero); });
            // xengPlong* (nstack = 1) on z_a, resampled on the host with the contract's rule
            for (int a = 0; a < ntrial; a++) {
                for (int s = 0; s < nser; s++)
                    for (int n = 0; n < NT; n++) {
                        const long long q = (long long)n * (long long)(n - NT);
                        const long long at = n + std::llrint(alpha[a] * (double)q);
                        if (at < 0 || at >= NT) return 5;
                        zres[(size_t)s * NT + n] = tbuf[(size_t)s * NT + at];
                    }
                launch(nser, 1, 0, [&] { plong_mean_kernel(zres.data(), mv2.data(), LN); });
                launch(N2 / PL_TC, nser, lds_cols, [&] { plong_cols_kernel(zres.data(), mv2.data(), scr2.data(), tw1.data(), LN1, LN2, 0); });
                launch(N1 >> lr, nser, lds_rows, [&] { plong_rows_kernel(scr2.data(), tws.data(), tw2.data(), LN1, LN2); });
                launch(N2 / PL_TC, nser, lds_power, [&] { plong_power_kernel(scr2.data(), tw.data(), P2.data(), LN1, LN2); });
                launch(1 << (LN - lw), nser, lds_white, [&] { plong_whiten_kernel(P2.data(), A2.data(), keep.data(), cnt.data(), mv2.data(), LN, lb, 1, 0); });
                launch(PL_NTILE, nser, 0, [&] { plong_sums_kernel(A2.data(), kedge.data(), part2.data(), LN, nlevel, nband, 0); });
                launch((int)((nrec_all + 255) / 256), 1, 0, [&] { plong_reduce_kernel(part2.data(), ref.data() + (size_t)a * nrec_all, (long long)nrec_all); });
            }
            if (memcmp(ref.data(), trec.data(), trec.size() * sizeof(PlongRecord))) {
                fprintf(stderr, "segment %d: the trial records differ from the plong sequence on the resampled series\n", nsegs);
                return 4;
            }
            nsegs++;
            if (nc > head) ingest(in + (size_t)head * nser * nprod, 0, nc - head);
        }
        in += (size_t)nc * nser * nprod;
        nwindows += nc;
    }
    f = fopen(argv[2], "wb");
    fwrite(&nsegs, 4, 1, f);
    fwrite(trec.data(), 8, trec.size(), f);
    fwrite(ref.data(), 8, ref.size(), f);
    fwrite(out.data(), 16, out.size(), f);
    fclose(f);
    return 0;
}
