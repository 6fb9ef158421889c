// Direction-dependent gains and peeling of bright sources (xengPeel*, peel.hip): one complex gain per (fine channel, polarisation,
// direction, stand) for ndir <= 8 point sources, solved per integration, and each source taken out with its own gains.
//
// Contract (include/xeng.h, "Direction-dependent gains and peeling"); ninput = 2 nstand, X[s][t] = conj(vis[c][t p][s p]):
//   vis    cf32[nfine][nstand][2][nstand][2], UpchanCorr's span (normally UpchanCalApply's output); never written
//   a      cf32[nfine][ndir][nstand], a_ds = exp(-2 pi i frac(freq[c] tau[d][s])): built by peel_steer_kernel at SetModel from the fp64
//          product and its fp64 fraction of a turn, sincospif and everything after fp32 (the context's state); both kernels read it
//   flux   f32[nfine][ndir] >= 0 (0: the direction is off), w f32[nstand] >= 0 (0: the stand is not loaded)
//   model  V[s][t] ~ sum_d F_d u_ds conj(u_dt), u_ds = g_ds a_ds.  Per sweep, from the gains g at its start:
//            Y[d][s] = sum_{t != s} X[s][t] w_t u_dt                                   for all directions: the one pass over V
//            for d ascending, with u~_e the new u_e for e < d and the old for e > d:
//              G_e = sum_t w_t conj(u~_et) u_dt  (G_d = P = sum_t w_t |u_dt|^2)
//              N_s = Y[d][s] - sum_{e != d} F_e u~_es (G_e - w_s conj(u~_es) u_ds)       e ascending
//              g'_ds = conj(a_ds) N_s / (F_d (P - w_s |u_ds|^2)), 0 where the denominator is not > 0
//          on even sweeps delta over the live (direction, stand), the early exit or the average
//   gains  cf32[nfine][2][ndir][nstand] after the phase reference per direction, stats f32[nfine][2][4] = {sweeps, last delta (-1:
//          none), stands solved, converged}
//   out    cf32 in vis's layout: on the parallel hands V - sum_d (F_d u_ds) conj(u_dt) from the gains just written, the cross hands
//          copied; the words i >= j are read, i > j computed, the diagonal's imaginary part +0, i < j the conjugate of out[j][i]
//
// peel_solve_kernel: one work-group of 256 threads (four waves) per (channel, polarisation), the whole iteration in one launch, as
// gaincal_kernel and for its reasons (the exit is uniform per work-group).  LDS: four tables [stand][PL_PITCH = 9] of float2 -- the
// steering a, the gains g at the sweep's start, u~ (u = g a, direction by direction replaced by the new one), and Y (then g') --
// with w, F, the partial sums and the sums: 152 KB at 512 stands, one work-group per compute unit.  Per sweep:
//   1. Y on v_mfma_f32_16x16x4_f32: rows = the directions (8 of the 16 rows used; the rest take zero operands), columns = a tile of
//      16 stands s, k = the stands t four at a time in ascending order.  Wave w takes the column tiles w, w + 4, ...  Lane (r, q) =
//      (lane & 15, lane >> 4) supplies A[row r][k q] = w_t u_rt of t = t0 + q (from LDS, one float2 read and two multiplies) and
//      B[k q][column r] = vis[t, p][s0 + r, p], consecutive pp words across r, conjugated by the operand signs:
//          Yre += hr Vr,  Yre += hi Vi,  Yim += hi Vr,  Yim += (-hr) Vi         (the minus is an exact operand negation)
//      PL_QUADS quads of t per trip, their loads in flight together.  A word with w_s = 0 or w_t = 0, and s = t, is not loaded: its
//      operand is a zero.  The 32x32x2 form would spend 64 cycles on two stands t for 32 columns with 8 of 32 rows used; this one
//      spends 32 cycles on four stands for 16 columns with 8 of 16 used: half the MFMA time per word of V, which at 512 stands is the
//      difference between an MFMA time equal to the HBM time of re-reading V and half of it.  Accumulator v of lane (r, q) is row 4 q
//      + v, column r: the lanes q < 2 hold the eight directions and write Y[s0 + r][4 q + v].
//   2. for d ascending with F_d > 0: (a) thread (j, e) = (tid >> 3, tid & 7) sums w_t conj(u~_et) u_dt over t = j, j + 32, ...
//      ascending (e = d gives P); (b) thread e < 8 adds the 32 partial sums of G_e in ascending j; (c) thread s (and s + 256) forms
//      N_s, g'_ds (into Y's place) and the new u~_ds.  Three barriers per direction.
//   3. delta as in gaincal_kernel (a thread's words in ascending (stand, direction) order, a butterfly over the wave, the waves in
//      order through LDS: the same bits in every thread, so the exit is uniform), the average, g and u = g a for the next sweep.
// After the loop every direction is multiplied by conj(g_d,ref) / |g_d,ref|; the unreferenced solution goes to the keep.
//
// peel_subtract_kernel: calapply_kernel's decomposition -- one wave per (fine channel, pair of 32-stand tiles S >= T), the chunks of
// 16 rows, the 16-byte loads and stores, the mirrored image through LDS -- with one model tile per polarisation on
// v_mfma_f32_32x32x2_f32 (k = the directions two per instruction; z = F u, b = u, u = g a formed at the operand load) and no factors:
// a word of a cross hand is stored as it was loaded.
//
// LDS banks.  Solve, step 1 (ds_read_b64, the lanes 0..31 and 32..63 in one cycle each, bank = (address / 4) mod 64): the lanes r < 8
// of the quads q, q + 1 read the dwords 18 (t0 + q) + 2 r .. + 1 and 18 more: 32 distinct banks.  Step 2 (c) and 3 read row s = tid:
// a stride of 18 dwords, 32 distinct bank pairs over 32 lanes (at pitch 8 the stride of 16 dwords would put 8 lanes on one pair).
// Step 2 (a) reads the rows j, j + 1, j + 2, j + 3 at e = 0 .. 7 per 32 lanes: the same 32 bank pairs as step 1.  Subtract: the
// image's argument is calapply_kernels.h's, unchanged.
//
// No atomics, no scalar memory writes, no printf, no scratch; one owner per word.  peel.hip is compiled with -fno-slp-vectorize
// (Makefile): complex fp32 arithmetic beside MFMA kernels, as image_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int PL_D = 8;             // directions at the most
constexpr int PL_T = 16;            // stands per column tile of the solve (the columns of the 16x16 MFMA)
constexpr int PL_PITCH = 9;         // float2 per stand of the LDS tables
constexpr int PL_QUADS = 8;         // k quads per trip of the contraction: their loads are all in flight before the first MFMA
constexpr int PL_PAD = 4 * PL_QUADS;    // the stands are padded to whole trips
constexpr int PL_PART = 32;         // partial sums per reduction of step 2
constexpr int PL_WAVES = 4;
constexpr int PL_THREADS = 64 * PL_WAVES;
constexpr int PL_MAX_NSTAND = 2 * PL_THREADS;   // a thread owns the stands tid and tid + 256
constexpr int PL_STEER_THREADS = 256;
constexpr int PS_T = 32;            // stands per tile of the subtraction (the rows and the columns of the 32x32 MFMA)
constexpr int PS_THREADS = 64;      // one wave
constexpr int PS_ROWS = 16;         // rows of a chunk
constexpr int PS_PITCH = 17;        // float2 per row of the mirrored image
static_assert(PL_PAD % PL_T == 0 && PL_THREADS == PL_D * PL_PART, "whole column tiles; one thread per (partial sum, direction)");

typedef float pl_f32x4 __attribute__((ext_vector_type(4)));
typedef float pl_f32x16 __attribute__((ext_vector_type(16)));

// dynamic LDS of peel_solve_kernel: a, g, u, y; w; F; the partial sums; the sums; the waves' sums
__host__ __device__ constexpr size_t peel_lds_bytes(int nstand) {
    const size_t nsp = (size_t)(nstand + PL_PAD - 1) / PL_PAD * PL_PAD;
    return 4 * nsp * PL_PITCH * sizeof(float2) + nsp * sizeof(float) + PL_D * sizeof(float) + (size_t)PL_D * PL_PART * sizeof(float2) + PL_D * sizeof(float2) +
           (size_t)2 * PL_WAVES * sizeof(float);
}
__host__ __device__ constexpr size_t peel_subtract_lds_bytes() { return (size_t)2 * PS_T * PS_PITCH * sizeof(float2); }

// g a
__device__ __forceinline__ float2 pl_cmul(float2 g, float2 a) {
    return make_float2(__builtin_fmaf(g.x, a.x, -(g.y * a.y)), __builtin_fmaf(g.x, a.y, g.y * a.x));
}

// The sums of a and of b over the work-group, the same bits in every thread: the wave's 64 lanes by a butterfly, the waves in order.
// Reached by every thread of the work-group.
__device__ __forceinline__ void pl_block_sum2(float& a, float& b, float* red, int tid) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        a += __shfl_xor(a, m);
        b += __shfl_xor(b, m);
    }
    __syncthreads();                                             // (the last sums have been read)
    if ((tid & 63) == 0) {
        red[tid >> 6] = a;
        red[PL_WAVES + (tid >> 6)] = b;
    }
    __syncthreads();
    a = ((red[0] + red[1]) + red[2]) + red[3];
    b = ((red[PL_WAVES] + red[PL_WAVES + 1]) + red[PL_WAVES + 2]) + red[PL_WAVES + 3];
}

// grid (ceil(ndir nstand / PL_STEER_THREADS), nfine): a[c][d][s] from freq[c] and tau[d][s]
__global__ __launch_bounds__(PL_STEER_THREADS) void peel_steer_kernel(const double* __restrict__ freq, const double* __restrict__ tau, float2* __restrict__ a,
                                                                      int nstand, int ndir) {
    const size_t n = (size_t)ndir * nstand, e = (size_t)blockIdx.x * PL_STEER_THREADS + threadIdx.x;
    if (e >= n) return;
    const double turns = __dmul_rn(freq[blockIdx.y], tau[e]);
    const float fr = (float)(turns - rint(turns));               // in [-1/2, 1/2]
    float sn, cs;
    sincospif(2.0f * fr, &sn, &cs);
    a[(size_t)blockIdx.y * n + e] = make_float2(cs, -sn);
}

// grid (nfine, 2), PL_THREADS threads, peel_lds_bytes(nstand) of dynamic LDS; nstand <= PL_MAX_NSTAND, 1 <= ndir <= PL_D, refant < nstand
__global__ __launch_bounds__(PL_THREADS) void peel_solve_kernel(const float2* __restrict__ vis, const float2* __restrict__ a, const float* __restrict__ flux,
                                                                const float* __restrict__ w, float2* __restrict__ gains, float* __restrict__ stats,
                                                                float2* __restrict__ keep_g, int* __restrict__ keep_ok, int nstand, int ndir, int niter, float tol,
                                                                int refant, int warm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pl_lds[];
    const int nsp = (nstand + PL_PAD - 1) / PL_PAD * PL_PAD, ntile = nsp / PL_T;
    float2* at = (float2*)pl_lds;                                // [nsp][PL_PITCH]
    float2* g = at + (size_t)nsp * PL_PITCH;                     // [nsp][PL_PITCH]: the gains at the sweep's start
    float2* u = g + (size_t)nsp * PL_PITCH;                      // [nsp][PL_PITCH]: u~
    float2* y = u + (size_t)nsp * PL_PITCH;                      // [nsp][PL_PITCH]: Y, then g'
    float* wl = (float*)(y + (size_t)nsp * PL_PITCH);            // [nsp]
    float* fl = wl + nsp;                                        // [PL_D]
    float2* part = (float2*)(fl + PL_D);                         // [PL_D][PL_PART]
    float2* fin = part + PL_D * PL_PART;                         // [PL_D]
    float* red = (float*)(fin + PL_D);                           // [2][PL_WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int c = blockIdx.x, p = blockIdx.y;
    const size_t ninput = 2 * (size_t)nstand, cp = (size_t)c * 2 + p;

    const bool from_keep = warm && keep_ok[cp] != 0;             // (uniform)
    if (tid < PL_D) fl[tid] = tid < ndir ? flux[(size_t)c * ndir + tid] : 0.f;
    for (int s = tid; s < nsp; s += PL_THREADS) {
        const float ws = s < nstand ? w[s] : 0.f;
        wl[s] = ws;
        for (int d = 0; d < PL_PITCH; d++) {
            float2 av = make_float2(0.f, 0.f), g0 = make_float2(0.f, 0.f);
            if (d < ndir && ws != 0.f) {
                av = a[((size_t)c * ndir + d) * nstand + s];
                if (flux[(size_t)c * ndir + d] > 0.f) g0 = from_keep ? keep_g[(cp * ndir + d) * nstand + s] : make_float2(1.f, 0.f);
            }
            at[s * PL_PITCH + d] = av;
            g[s * PL_PITCH + d] = g0;
            u[s * PL_PITCH + d] = pl_cmul(g0, av);
            y[s * PL_PITCH + d] = make_float2(0.f, 0.f);
        }
    }

    const float2* vc = vis + (size_t)c * ninput * ninput;
    int it = 0, conv = 0;
    float delta = -1.f;
    while (it < niter && !conv) {
        __syncthreads();                                         // (g and u are whole; the first time, the other tables too)
        // 1. Y[d][s]
        for (int sj = wave; sj < ntile; sj += PL_WAVES) {
            const int s = sj * PL_T + r;
            const bool slive = s < nstand && wl[s] != 0.f;
            pl_f32x4 yre = {}, yim = {};
            // PL_QUADS k quads per trip: the loads first, then 4 PL_QUADS MFMAs.  t0 + 4 PL_QUADS - 1 <= nsp - 1, and w and the rows
            // of u are zeros from nstand on: the quads past the last stand add fma(0, 0, C) = C
            for (int t0 = 0; t0 < nstand; t0 += 4 * PL_QUADS) {
                float2 hh[PL_QUADS], v[PL_QUADS];
#pragma unroll
                for (int q = 0; q < PL_QUADS; q++) {
                    const int t = t0 + 4 * q + kq;
                    const float wt = wl[t];
                    hh[q] = make_float2(0.f, 0.f);
                    if (r < PL_D) {
                        const float2 ut = u[t * PL_PITCH + r];
                        hh[q] = make_float2(wt * ut.x, wt * ut.y);
                    }
                    v[q] = make_float2(0.f, 0.f);
                    if (slive && wt != 0.f && t != s) v[q] = vc[(size_t)(2 * t + p) * ninput + 2 * s + p];      // (wt = 0 for t >= nstand)
                }
#pragma unroll
                for (int q = 0; q < PL_QUADS; q++) {
                    const float hr = hh[q].x, hi = hh[q].y, nhr = -hh[q].x;
                    yre = __builtin_amdgcn_mfma_f32_16x16x4f32(hr, v[q].x, yre, 0, 0, 0);
                    yim = __builtin_amdgcn_mfma_f32_16x16x4f32(hi, v[q].x, yim, 0, 0, 0);
                    yre = __builtin_amdgcn_mfma_f32_16x16x4f32(hi, v[q].y, yre, 0, 0, 0);
                    yim = __builtin_amdgcn_mfma_f32_16x16x4f32(nhr, v[q].y, yim, 0, 0, 0);
                }
            }
            if (kq < 2) {
#pragma unroll
                for (int v = 0; v < 4; v++) y[s * PL_PITCH + 4 * kq + v] = make_float2(yre[v], yim[v]);
            }
        }
        __syncthreads();
        // 2. the directions in ascending order
        for (int d = 0; d < ndir; d++) {
            const float fd = fl[d];
            if (!(fd > 0.f)) continue;                           // (uniform)
            {
                const int e = tid & (PL_D - 1), j = tid >> 3;
                float sr = 0.f, si = 0.f;
                for (int t = j; t < nstand; t += PL_PART) {
                    const float wt = wl[t];
                    const float2 ud = u[t * PL_PITCH + d], ue = u[t * PL_PITCH + e];
                    sr = __builtin_fmaf(wt, __builtin_fmaf(ue.x, ud.x, ue.y * ud.y), sr);       // conj(u~_e) u_d
                    si = __builtin_fmaf(wt, __builtin_fmaf(ue.x, ud.y, -(ue.y * ud.x)), si);
                }
                part[e * PL_PART + j] = make_float2(sr, si);
            }
            __syncthreads();
            if (tid < PL_D) {
                float sr = 0.f, si = 0.f;
                for (int j = 0; j < PL_PART; j++) {
                    sr += part[tid * PL_PART + j].x;
                    si += part[tid * PL_PART + j].y;
                }
                fin[tid] = make_float2(sr, si);
            }
            __syncthreads();
            const float pw = fin[d].x;
#pragma unroll
            for (int jj = 0; jj < 2; jj++) {
                const int s = tid + jj * PL_THREADS;
                if (s < nstand && wl[s] != 0.f) {
                    const float ws = wl[s];
                    const float2 ud = u[s * PL_PITCH + d], av = at[s * PL_PITCH + d];
                    float2 n = y[s * PL_PITCH + d];
                    for (int e = 0; e < ndir; e++) {
                        if (e == d) continue;
                        const float2 ue = u[s * PL_PITCH + e], ge = fin[e];
                        const float cr = ge.x - ws * __builtin_fmaf(ue.x, ud.x, ue.y * ud.y);
                        const float ci = ge.y - ws * __builtin_fmaf(ue.x, ud.y, -(ue.y * ud.x));
                        const float zr = fl[e] * ue.x, zi = fl[e] * ue.y;
                        n.x -= __builtin_fmaf(zr, cr, -(zi * ci));
                        n.y -= __builtin_fmaf(zr, ci, zi * cr);
                    }
                    const float den = fd * (pw - ws * __builtin_fmaf(ud.x, ud.x, ud.y * ud.y));
                    float2 gn = make_float2(0.f, 0.f);
                    if (den > 0.f) gn = make_float2(__builtin_fmaf(av.x, n.x, av.y * n.y) / den, __builtin_fmaf(av.x, n.y, -(av.y * n.x)) / den);
                    y[s * PL_PITCH + d] = gn;
                    u[s * PL_PITCH + d] = pl_cmul(gn, av);
                }
            }
            __syncthreads();                                     // (u~_d is whole before the next direction's sums; fin has been read)
        }
        // 3. delta, the exit or the average, the tables of the next sweep
        it++;
        const bool even = (it & 1) == 0;
        if (even) {
            float num = 0.f, den = 0.f;
#pragma unroll
            for (int jj = 0; jj < 2; jj++) {
                const int s = tid + jj * PL_THREADS;
                if (s < nstand && wl[s] != 0.f) {
                    for (int d = 0; d < ndir; d++) {
                        if (!(fl[d] > 0.f)) continue;
                        const float2 nv = y[s * PL_PITCH + d], o = g[s * PL_PITCH + d];
                        const float dx = nv.x - o.x, dy = nv.y - o.y;
                        num += __builtin_fmaf(dx, dx, dy * dy);
                        den += __builtin_fmaf(nv.x, nv.x, nv.y * nv.y);
                    }
                }
            }
            pl_block_sum2(num, den, red, tid);
            delta = sqrtf(num / den);
            if (tol > 0.f && delta <= tol) conv = 1;
        }
        const bool avg = even && !conv;
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            const int s = tid + jj * PL_THREADS;
            if (s < nstand && wl[s] != 0.f) {
                for (int d = 0; d < ndir; d++) {
                    float2 nv = make_float2(0.f, 0.f);
                    if (fl[d] > 0.f) {
                        nv = y[s * PL_PITCH + d];
                        const float2 o = g[s * PL_PITCH + d];
                        if (avg) nv = make_float2((nv.x + o.x) * 0.5f, (nv.y + o.y) * 0.5f);
                    }
                    g[s * PL_PITCH + d] = nv;
                    u[s * PL_PITCH + d] = pl_cmul(nv, at[s * PL_PITCH + d]);
                }
            }
        }
    }
    __syncthreads();
    // the phase reference per direction, the outputs, the keep
    float solved = 0.f, bad = 0.f;
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
        const int s = tid + jj * PL_THREADS;
        if (s < nstand) {
            const bool slive = wl[s] != 0.f;
            bool all = slive, any = false;
            for (int d = 0; d < ndir; d++) {
                const float2 gr = g[refant * PL_PITCH + d], x = g[s * PL_PITCH + d];
                const float mag = sqrtf(__builtin_fmaf(gr.x, gr.x, gr.y * gr.y));
                float2 ph = make_float2(1.f, 0.f);
                if (mag > 0.f) ph = make_float2(gr.x / mag, -(gr.y / mag));
                float2 o = make_float2(0.f, 0.f);
                if (slive) {
                    o = pl_cmul(x, ph);
                    if (fl[d] > 0.f) {
                        any = true;
                        if (x.x == 0.f && x.y == 0.f) all = false;
                    }
                    if (!(fabsf(x.x) <= 3.4028234664e38f) || !(fabsf(x.y) <= 3.4028234664e38f)) bad += 1.f;
                }
                gains[(cp * ndir + d) * nstand + s] = o;
                if (niter > 0) keep_g[(cp * ndir + d) * nstand + s] = x;
            }
            if (all && any) solved += 1.f;
        }
    }
    pl_block_sum2(solved, bad, red, tid);
    if (tid == 0) {
        float* st = stats + cp * 4;
        st[0] = (float)it;
        st[1] = delta;
        st[2] = solved;
        st[3] = (float)conv;
        if (niter > 0) keep_ok[cp] = conv && bad == 0.f;
    }
}

// two words at p, p + 1 (p 16-byte aligned): both as one 16-byte store, one as an 8-byte store
__device__ __forceinline__ void ps_store2(float2* p, float2 w0, float2 w1, bool m0, bool m1) {
    if (m0 && m1)
        *(float4*)p = make_float4(w0.x, w0.y, w1.x, w1.y);
    else if (m0)
        p[0] = w0;
    else if (m1)
        p[1] = w1;
}

// grid (ntile (ntile + 1) / 2, nfine) with ntile = ceil(nstand / PS_T), PS_THREADS threads; vis and out 16-byte aligned, 1 <= ndir <= PL_D
__global__ __launch_bounds__(PS_THREADS, 2) void peel_subtract_kernel(const float2* __restrict__ vis, const float2* __restrict__ a, const float* __restrict__ flux,
                                                                      const float2* __restrict__ gains, float2* __restrict__ out, int nstand, int ndir) {
    __shared__ __attribute__((aligned(16))) float2 ps_lds[2 * PS_T * PS_PITCH];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int c = blockIdx.y;
    int S = 0, T = blockIdx.x;                                   // blockIdx.x = S (S + 1) / 2 + T, T <= S
    while (T > S) {
        T -= S + 1;
        S++;
    }
    const int s0 = S * PS_T, t0 = T * PS_T;
    const bool diag = S == T;
    const size_t ninput = 2 * (size_t)nstand;

    // 1. the model's tiles, one per polarisation: rows = the stands of S, columns = the stands of T, k = the directions two per
    //    instruction in ascending order; a direction past ndir and a stand past nstand are zero operands
    pl_f32x16 mre0 = {}, mim0 = {}, mre1 = {}, mim1 = {};
    {
        float2 z[2][PL_D / 2], b[2][PL_D / 2];
#pragma unroll
        for (int p = 0; p < 2; p++) {
#pragma unroll
            for (int m = 0; m < PL_D / 2; m++) {
                const int d = 2 * m + h;
                z[p][m] = b[p][m] = make_float2(0.f, 0.f);
                if (d < ndir) {
                    const float f = flux[(size_t)c * ndir + d];
                    const size_t ia = ((size_t)c * ndir + d) * nstand, ig = (((size_t)c * 2 + p) * ndir + d) * nstand;
                    if (s0 + r < nstand) {
                        const float2 us = pl_cmul(gains[ig + s0 + r], a[ia + s0 + r]);
                        z[p][m] = make_float2(f * us.x, f * us.y);
                    }
                    if (t0 + r < nstand) b[p][m] = pl_cmul(gains[ig + t0 + r], a[ia + t0 + r]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < PL_D / 2; m++) {
            if (2 * m < ndir) {                                  // (uniform)
                const float nzr0 = -z[0][m].x, nzr1 = -z[1][m].x;
                mre0 = __builtin_amdgcn_mfma_f32_32x32x2f32(z[0][m].x, b[0][m].x, mre0, 0, 0, 0);
                mre0 = __builtin_amdgcn_mfma_f32_32x32x2f32(z[0][m].y, b[0][m].y, mre0, 0, 0, 0);
                mim0 = __builtin_amdgcn_mfma_f32_32x32x2f32(z[0][m].y, b[0][m].x, mim0, 0, 0, 0);
                mim0 = __builtin_amdgcn_mfma_f32_32x32x2f32(nzr0, b[0][m].y, mim0, 0, 0, 0);
                mre1 = __builtin_amdgcn_mfma_f32_32x32x2f32(z[1][m].x, b[1][m].x, mre1, 0, 0, 0);
                mre1 = __builtin_amdgcn_mfma_f32_32x32x2f32(z[1][m].y, b[1][m].y, mre1, 0, 0, 0);
                mim1 = __builtin_amdgcn_mfma_f32_32x32x2f32(z[1][m].y, b[1][m].x, mim1, 0, 0, 0);
                mim1 = __builtin_amdgcn_mfma_f32_32x32x2f32(nzr1, b[1][m].y, mim1, 0, 0, 0);
            }
        }
    }

    const int t = t0 + r;
    const bool tin = t < nstand;
    const float2* vc = vis + (size_t)c * ninput * ninput;
    float2* oc = out + (size_t)c * ninput * ninput;

    // 2. the chunks (calapply_kernels.h: the rows a lane takes are the rows of its accumulators)
#pragma unroll
    for (int g = 0; g < 4; g++) {
        float4 v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int uu = e >> 1, p = e & 1;
            const int s = s0 + 8 * g + 4 * h + uu, i = 2 * s + p;
            const bool in = s < nstand && tin;
            const bool n0 = in && (!diag || 2 * t <= i), n1 = in && (!diag || 2 * t + 1 <= i);
            const float2* src = vc + (size_t)i * ninput + 2 * t;
            v[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 && n1) {
                v[e] = *(const float4*)src;
            } else if (n0) {
                const float2 x = src[0];
                v[e].x = x.x;
                v[e].y = x.y;
            } else if (n1) {
                const float2 x = src[1];
                v[e].z = x.x;
                v[e].w = x.y;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int uu = e >> 1, p = e & 1;
            const int s = s0 + 8 * g + 4 * h + uu, i = 2 * s + p;
            float2 o[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int j = 2 * t + q;
                float yr = q ? v[e].z : v[e].x, yi = q ? v[e].w : v[e].y;
                if (q == p) {
                    yr -= p ? mre1[4 * g + uu] : mre0[4 * g + uu];
                    yi -= p ? mim1[4 * g + uu] : mim0[4 * g + uu];
                }
                if (i == j) yi = 0.f;
                o[q] = make_float2(yr, yi);
                ps_lds[(2 * r + q) * PS_PITCH + 2 * (4 * h + uu) + p] = make_float2(yr, -yi);      // the mirrored word: the conjugate
            }
            const bool in = s < nstand && tin;
            ps_store2(oc + (size_t)i * ninput + 2 * t, o[0], o[1], in && (!diag || 2 * t <= i), in && (!diag || 2 * t + 1 <= i));
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int jl = 8 * e + (lane >> 3), il = 2 * (lane & 7);
            const int j = 2 * t0 + jl, i = 2 * s0 + PS_ROWS * g + il;                   // out[j][i], out[j][i + 1]; i is even
            const float2 w0 = ps_lds[jl * PS_PITCH + il], w1 = ps_lds[jl * PS_PITCH + il + 1];
            const bool in = (size_t)j < ninput && (size_t)i < ninput;
            ps_store2(oc + (size_t)j * ninput + i, w0, w1, in && (!diag || i > j), in && (!diag || i + 1 > j));
        }
        __syncthreads();                                         // (the image has been read before the next chunk overwrites it)
    }
}

}  // namespace xeng
