// Per-stand gains from the fine-channel visibilities (xengGaincal*, gaincal.hip): StEFCal (Salvini & Wijnholds 2014) against a
// point-source sky model of nsrc <= 32 sources, one solution per (fine channel, polarisation), the whole iteration in one launch.
//
// Contract (include/xeng.h, "Per-stand gains from the fine-channel visibilities"); ninput = 2 nstand, X[s][t] = conj(vis[c][t p][s p]):
//   vis    cf32[nfine][nstand][2][nstand][2], UpchanCorr's span; only the pp blocks are read, never written
//   freq   f64[nfine] Hz, tau f64[nsrc][nstand] s, flux f32[nfine][nsrc] >= 0, w f32[nstand] >= 0 (the context's state)
//   a_ks = exp(-2 pi i frac(freq[c] tau[k][s])): the product and its fraction of a turn in fp64, sincospif and everything after fp32
//   per iteration  N_s = sum_k F_k conj(a_ks) sum_{t != s} X[s][t] (w_t g_t a_kt)
//                  D_s = sum_{k,k'} (F_k a_ks) conj(F_k' a_k's) G[k][k'] - w_s |g_s|^2 (sum_k F_k)^2,   G[k][k'] = sum_t w_t |g_t|^2 conj(a_kt) a_k't
//                  g_s <- N_s / D_s, or 0 where D_s is not > 0; on even iterations delta, the early exit or the average
//   gains  cf32[nfine][2][nstand] after the phase reference, stats f32[nfine][2][4] = {iterations, last delta (-1: none), stands solved, converged}
//
// One kernel, one work-group of 256 threads (four waves) per (channel, polarisation): the two polarisations are two independent
// problems with early exits of their own, so a group per pair keeps the exit uniform per work-group, halves the registers and gives
// twice the work-groups (192 at 96 channels for 256 compute units).  The price: the 8-byte pp words of a row of V lie 16 bytes
// apart, so half of every cache line fetched is the pq words nobody uses -- as in image_kernel, which fetches 24 of 32 bytes.
// LDS: the steering tile a[s][k] (float2 at pitch GC_PITCH = 33, built once), w, g, the new g (first N), F, the Gram matrix, the
// waves' sums.  What differs from the issue's sketch: the tile in LDS is a, not h = w g a -- both tiles at 512 stands would take
// 270 KB -- and h is formed at the operand read by one complex multiply with w_t g_t.  Per iteration:
//   1. U[k][s] = sum_t h_kt X[s][t] on v_mfma_f32_32x32x2_f32, rows = the sources, columns = a tile of 32 stands s, k = the stands t
//      two at a time in ascending order.  Wave w takes the column tiles w, w + 4, ...  V is re-read, ALONG its rows: lane (r, h)
//      loads vis[t0 + h, p][s0 + r, p], consecutive pp words across r, and conjugates by the operand signs: four MFMAs per k pair
//          Ure += hr Vr,  Ure += hi Vi,  Uim += hi Vr,  Uim += (-hr) Vi         (the minus is an exact operand negation)
//      A block with w_s = 0 or w_t = 0, and s = t, is not loaded: its operand is a zero.  Then per lane (its column s, its 16 rows
//      k, ascending): n += (F_k conj(a_ks)) U[k][s] by fmaf; the two halves added (one shuffle); N_s into LDS.
//   2. the Gram matrix: thread e takes (k, k') = (e / nsrc, e % nsrc), e += 256; the stands t in ascending order, one fmaf chain.
//   3. thread s (and s + 256) forms D_s: for k ascending, c_k = sum_k' G[k][k'] conj(z_k') with k' ascending, D += Re(z_k c_k), then
//      the t = s term is subtracted by one fmaf; g_s = N_s / D_s.
//   4. on even iterations delta = sqrt(sum |g_new - g|^2 / sum |g_new|^2) over the stands of weight > 0: a thread's (at most two)
//      stands in ascending order, a butterfly over the wave's 64 lanes (xor 1 .. 32), the four waves through LDS added in wave order.
//      Every thread of the work-group holds the same bits, so the exit is uniform.
// After the loop the gains are multiplied by conj(g_ref) / |g_ref| (left alone where |g_ref| is not > 0), stands of weight 0 written
// as 0 + 0i.  The unreferenced solution and whether it was converged and finite go to the context's keep for a warm start (not with
// niter = 0).  A solution depends on its own channel's block, the model and the weights only.  No atomics, no scalar memory writes,
// no printf; one owner per word.
//
// LDS banks (ds_read_b64, the lanes 0..31 and 32..63 in one cycle each, bank = (address / 4) mod 64): the argument of
// image_kernels.h holds unchanged.  Step 1's operand read takes 32 consecutive float2 of row t: 64 distinct banks at any pitch; its
// epilogue and step 3 read a[s0 + (lane & 31)][k]: a stride of the pitch, 66 dwords = 2 banks at pitch 33, 64 distinct banks (at
// pitch 32 all 32 lanes of a half would meet on one pair).  Step 2 reads one row per trip: a broadcast and consecutive words.
//
// gaincal.hip is compiled with -fno-slp-vectorize (Makefile): complex fp32 arithmetic beside MFMA kernels, as image_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int GC_K = 32;            // sources at the most (the rows of the 32x32 MFMA)
constexpr int GC_T = 32;            // stands per column tile
constexpr int GC_PITCH = 33;        // float2 per stand of the steering tile
constexpr int GC_PAIRS = 8;         // k pairs per trip of the contraction: their loads are all in flight before the first MFMA
constexpr int GC_WAVES = 4;
constexpr int GC_THREADS = 64 * GC_WAVES;
constexpr int GC_MAX_NSTAND = 2 * GC_THREADS;   // a thread owns the stands tid and tid + 256
static_assert(GC_T % (2 * GC_PAIRS) == 0, "a trip of the contraction stays within the padded tile");

typedef float gc_f32x16 __attribute__((ext_vector_type(16)));

// dynamic LDS of gaincal_kernel: the steering tile, w, g, the new g, F, the Gram matrix, the waves' sums
__host__ __device__ constexpr size_t gaincal_lds_bytes(int nstand) {
    const size_t nsp = (size_t)(nstand + GC_T - 1) / GC_T * GC_T;
    return nsp * GC_PITCH * sizeof(float2) + nsp * sizeof(float) + 2 * nsp * sizeof(float2) + GC_K * sizeof(float) + (size_t)GC_K * GC_K * sizeof(float2) +
           (size_t)2 * GC_WAVES * sizeof(float);
}

// row of accumulator register v in lane half h (C/D map of the 32x32 MFMA: col = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 h)
__device__ __forceinline__ int gc_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// The sums of a and of b over the work-group, the same bits in every thread: the wave's 64 lanes by a butterfly, the waves in order.
// Reached by every thread of the work-group.
__device__ __forceinline__ void gc_block_sum2(float& a, float& b, float* red, int tid) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        a += __shfl_xor(a, m);
        b += __shfl_xor(b, m);
    }
    __syncthreads();                                             // (the last sums have been read)
    if ((tid & 63) == 0) {
        red[tid >> 6] = a;
        red[GC_WAVES + (tid >> 6)] = b;
    }
    __syncthreads();
    a = ((red[0] + red[1]) + red[2]) + red[3];
    b = ((red[GC_WAVES] + red[GC_WAVES + 1]) + red[GC_WAVES + 2]) + red[GC_WAVES + 3];
}

// grid (nfine, 2), GC_THREADS threads, gaincal_lds_bytes(nstand) of dynamic LDS; nstand <= GC_MAX_NSTAND, nsrc <= GC_K, refant < nstand
__global__ __launch_bounds__(GC_THREADS) void gaincal_kernel(const float2* __restrict__ vis, const double* __restrict__ freq, const double* __restrict__ tau,
                                                             const float* __restrict__ flux, const float* __restrict__ w, float2* __restrict__ gains,
                                                             float* __restrict__ stats, float2* __restrict__ keep_g, int* __restrict__ keep_ok, int nstand,
                                                             int nsrc, int niter, float tol, int refant, int warm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t gc_lds[];
    const int nsp = (nstand + GC_T - 1) / GC_T * GC_T, ntile = nsp / GC_T;
    float2* at = (float2*)gc_lds;                                // [nsp][GC_PITCH]
    float* wl = (float*)(at + (size_t)nsp * GC_PITCH);           // [nsp]
    float2* g = (float2*)(wl + nsp);                             // [nsp]
    float2* gn = g + nsp;                                        // [nsp]: N, then the new g
    float* fl = (float*)(gn + nsp);                              // [GC_K]
    float2* gram = (float2*)(fl + GC_K);                         // [GC_K][GC_K]
    float* red = (float*)(gram + GC_K * GC_K);                   // [2][GC_WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int c = blockIdx.x, p = blockIdx.y;
    const size_t ninput = 2 * (size_t)nstand, cp = (size_t)c * 2 + p;

    const bool from_keep = warm && keep_ok[cp] != 0;             // (uniform)
    for (int s = tid; s < nsp; s += GC_THREADS) {
        const float ws = s < nstand ? w[s] : 0.f;
        wl[s] = ws;
        float2 g0 = make_float2(0.f, 0.f);
        if (ws != 0.f) g0 = from_keep ? keep_g[cp * nstand + s] : make_float2(1.f, 0.f);
        g[s] = g0;
    }
    if (tid < GC_K) fl[tid] = tid < nsrc ? flux[(size_t)c * nsrc + tid] : 0.f;
    __syncthreads();
    // the steering tile: thread e takes (k, s) = (e / nsp, e % nsp), so the reads of tau run along s
    const double f = freq[c];
    for (int e = tid; e < GC_K * nsp; e += GC_THREADS) {
        const int k = e / nsp, s = e - k * nsp;
        float2 a = make_float2(0.f, 0.f);
        if (k < nsrc && wl[s] != 0.f) {
            const double turns = __dmul_rn(f, tau[(size_t)k * nstand + s]);
            const float fr = (float)(turns - rint(turns));       // in [-1/2, 1/2]
            float sn, cs;
            sincospif(2.0f * fr, &sn, &cs);
            a = make_float2(cs, -sn);
        }
        at[s * GC_PITCH + k] = a;
    }
    float fsum = 0.f;
    for (int k = 0; k < GC_K; k++) fsum += fl[k];

    const float2* vc = vis + (size_t)c * ninput * ninput;
    int it = 0, conv = 0;
    float delta = -1.f;
    while (it < niter && !conv) {
        __syncthreads();                                         // (g is whole; the first time, the tile too)
        // 1. N_s
        for (int sj = wave; sj < ntile; sj += GC_WAVES) {
            const int s = sj * GC_T + r;
            const bool slive = s < nstand && wl[s] != 0.f;
            gc_f32x16 ure = {}, uim = {};
            // GC_PAIRS k pairs per trip: the loads first, then 4 GC_PAIRS MFMAs (one wave per SIMD: nothing else hides the loads).
            // t0 + 2 GC_PAIRS - 1 <= nsp - 1, and w and the rows of the tile are zeros from nstand on: the pairs past the last stand
            // add fma(0, 0, C) = C
            for (int t0 = 0; t0 < nstand; t0 += 2 * GC_PAIRS) {
                float2 hh[GC_PAIRS], v[GC_PAIRS];
#pragma unroll
                for (int q = 0; q < GC_PAIRS; q++) {
                    const int t = t0 + 2 * q + h;
                    const float wt = wl[t];
                    const float2 gt = g[t], a = at[t * GC_PITCH + r];
                    const float hr = wt * gt.x, hi = wt * gt.y;
                    hh[q] = make_float2(__builtin_fmaf(hr, a.x, -(hi * a.y)), __builtin_fmaf(hr, a.y, hi * a.x));
                    v[q] = make_float2(0.f, 0.f);
                    if (slive && wt != 0.f && t != s) v[q] = vc[(size_t)(2 * t + p) * ninput + 2 * s + p];      // (wt = 0 for t >= nstand)
                }
#pragma unroll
                for (int q = 0; q < GC_PAIRS; q++) {
                    const float hr = hh[q].x, hi = hh[q].y, nhr = -hh[q].x;
                    ure = __builtin_amdgcn_mfma_f32_32x32x2f32(hr, v[q].x, ure, 0, 0, 0);
                    uim = __builtin_amdgcn_mfma_f32_32x32x2f32(hi, v[q].x, uim, 0, 0, 0);
                    ure = __builtin_amdgcn_mfma_f32_32x32x2f32(hi, v[q].y, ure, 0, 0, 0);
                    uim = __builtin_amdgcn_mfma_f32_32x32x2f32(nhr, v[q].y, uim, 0, 0, 0);
                }
            }
            float nr = 0.f, ni = 0.f;
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int k = gc_row(v, h);
                const float2 a = at[s * GC_PITCH + k];
                const float zr = fl[k] * a.x, zi = -(fl[k] * a.y);                  // F_k conj(a_ks)
                nr = __builtin_fmaf(zr, ure[v], __builtin_fmaf(-zi, uim[v], nr));
                ni = __builtin_fmaf(zr, uim[v], __builtin_fmaf(zi, ure[v], ni));
            }
            nr += __shfl_xor(nr, 32);
            ni += __shfl_xor(ni, 32);
            if (h == 0) gn[s] = make_float2(nr, ni);
        }
        // 2. the Gram matrix
        for (int e = tid; e < nsrc * nsrc; e += GC_THREADS) {
            const int k = e / nsrc, k2 = e - k * nsrc;
            float gr = 0.f, gi = 0.f;
            for (int t = 0; t < nstand; t++) {
                const float2 gt = g[t], a = at[t * GC_PITCH + k], b = at[t * GC_PITCH + k2];
                const float qt = wl[t] * __builtin_fmaf(gt.x, gt.x, gt.y * gt.y);
                gr = __builtin_fmaf(qt, __builtin_fmaf(a.x, b.x, a.y * b.y), gr);   // conj(a) b
                gi = __builtin_fmaf(qt, __builtin_fmaf(a.x, b.y, -(a.y * b.x)), gi);
            }
            gram[k * GC_K + k2] = make_float2(gr, gi);
        }
        __syncthreads();
        // 3. D_s and the new gains of this thread's stands
        float2 gnew[2], gold[2];
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int s = tid + j * GC_THREADS;
            gnew[j] = gold[j] = make_float2(0.f, 0.f);
            if (s < nstand && wl[s] != 0.f) {
                const float2 o = g[s], n = gn[s];
                float d = 0.f;
                for (int k = 0; k < nsrc; k++) {
                    float cr = 0.f, ci = 0.f;
                    for (int k2 = 0; k2 < nsrc; k2++) {
                        const float2 G = gram[k * GC_K + k2], a2 = at[s * GC_PITCH + k2];
                        const float yr = fl[k2] * a2.x, yi = fl[k2] * a2.y;         // z_k' ; G conj(z_k')
                        cr = __builtin_fmaf(G.x, yr, __builtin_fmaf(G.y, yi, cr));
                        ci = __builtin_fmaf(G.y, yr, __builtin_fmaf(-G.x, yi, ci));
                    }
                    const float2 a = at[s * GC_PITCH + k];
                    const float zr = fl[k] * a.x, zi = fl[k] * a.y;
                    d = __builtin_fmaf(zr, cr, __builtin_fmaf(-zi, ci, d));
                }
                d = __builtin_fmaf(-(wl[s] * __builtin_fmaf(o.x, o.x, o.y * o.y)), fsum * fsum, d);
                float2 nv = make_float2(0.f, 0.f);
                if (d > 0.f) nv = make_float2(n.x / d, n.y / d);
                gnew[j] = nv;
                gold[j] = o;
                const float dx = nv.x - o.x, dy = nv.y - o.y;
                num += __builtin_fmaf(dx, dx, dy * dy);
                den += __builtin_fmaf(nv.x, nv.x, nv.y * nv.y);
            }
        }
        it++;
        if ((it & 1) == 0) {
            gc_block_sum2(num, den, red, tid);
            delta = sqrtf(num / den);
            if (tol > 0.f && delta <= tol) {
                conv = 1;
            } else {
#pragma unroll
                for (int j = 0; j < 2; j++) gnew[j] = make_float2((gnew[j].x + gold[j].x) * 0.5f, (gnew[j].y + gold[j].y) * 0.5f);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int s = tid + j * GC_THREADS;
            if (s < nstand) g[s] = gnew[j];
        }
    }
    __syncthreads();
    // the phase reference, the outputs, the keep
    const float2 gr = g[refant];
    const float mag = sqrtf(__builtin_fmaf(gr.x, gr.x, gr.y * gr.y));
    float2 ph = make_float2(1.f, 0.f);
    if (mag > 0.f) ph = make_float2(gr.x / mag, -(gr.y / mag));
    float solved = 0.f, bad = 0.f;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int s = tid + j * GC_THREADS;
        if (s < nstand) {
            const float2 x = g[s];
            float2 y = make_float2(0.f, 0.f);
            if (wl[s] != 0.f) {
                y = make_float2(__builtin_fmaf(x.x, ph.x, -(x.y * ph.y)), __builtin_fmaf(x.x, ph.y, x.y * ph.x));
                if (x.x != 0.f || x.y != 0.f) solved += 1.f;
                if (!(fabsf(x.x) <= 3.4028234664e38f) || !(fabsf(x.y) <= 3.4028234664e38f)) bad += 1.f;
            }
            gains[cp * nstand + s] = y;
            if (niter > 0) keep_g[cp * nstand + s] = x;
        }
    }
    gc_block_sum2(solved, bad, red, tid);
    if (tid == 0) {
        float* st = stats + cp * 4;
        st[0] = (float)it;
        st[1] = delta;
        st[2] = solved;
        st[3] = (float)conv;
        if (niter > 0) keep_ok[cp] = conv && bad == 0.f;
    }
}

}  // namespace xeng
