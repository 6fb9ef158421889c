// Calibrated, source-subtracted visibilities (xengCalapply*, calapply.hip): UpchanCorr's matrix times the apply factors of its two
// inputs, minus a point-source model of nsrc <= 32 sources on the parallel hands, written as a matrix of the same format.
//
// Contract (include/xeng.h, "Calibrated, source-subtracted visibilities"); ninput = 2 nstand, row i = 2 s + p, column j = 2 t + q:
//   vis    cf32[nfine][nstand][2][nstand][2], UpchanCorr's span V[c][s p][t q]; only the words i >= j are read, never written
//   a      cf32[nfine][nsrc][nstand], a_ks = exp(-2 pi i frac(freq[c] tau[k][s])): built by calapply_steer_kernel at SetModel from
//          the fp64 product and its fp64 fraction of a turn, sincospif and everything after fp32 -- the words of image_kernel and
//          gaincal_kernel, formed once per model instead of once per work-group (the context's state)
//   flux   f32[nfine][nsrc] >= 0, hf cf32[nfine][2][nstand] (the context's state); hf = 0 marks a (stand, pol) that is left out
//   out    cf32 in vis's layout.  i > j: (h_i conj(h_j)) V[c][i][j] - delta_pq M_c[s][t];  i = j: its real part and +0;  i < j: the
//          conjugate of out[c][j][i], the same words with the sign of the imaginary part turned, not computed again.
//          M_c[s][t] = sum_k (F_k a_ks) conj(a_kt).  A word whose h_i or h_j is 0 is not loaded and is written +0 + 0i, both copies.
//
// calapply_kernel: one work-group of ONE wave per (fine channel, pair of 32-stand tiles S >= T), grid (ntile (ntile + 1) / 2, nfine).
// The bound is HBM (64 x 64 words read, twice that written: 96 KiB per work-group); one wave per work-group keeps the model tile
// in one wave's registers with no copy between waves and no barrier that waits for anybody, and the occupancy comes from the
// work-groups: 8.5 KiB of LDS and 139 registers each, three waves per SIMD (__launch_bounds__(64, 3): without the bound the
// compiler keeps the model's tile in 32 AGPRs beside 139 VGPRs, two waves per SIMD, and a run takes 9 % longer; a bound of four
// spills).  The compiler issues the loads of all four chunks ahead of the first chunk's arithmetic (vis and out are __restrict__).
//   1. M's tile on v_mfma_f32_32x32x2_f32: rows = the stands s of S, columns = the stands t of T, k = the sources two per
//      instruction in ascending order, CA_PAIRS pairs per trip with their loads in flight together.  Lane (r, h) loads a[k = 2 m +
//      h][s0 + r] and a[k][t0 + r] (consecutive words across r) and F_k; four MFMAs per pair, z = F a:
//          Mre += zr br,  Mre += zi bi,  Mim += zi br,  Mim += (-zr) bi        (the minus is an exact operand negation)
//      so per word and part one chain over k ascending: (k even, k odd) of the first product, then (k even, k odd) of the second.
//      A source past nsrc and a stand past nstand are zero operands: fma(0, 0, C) = C.  Lane (r, h) then holds M[s][t0 + r] of the
//      16 stands s = s0 + (v & 3) + 8 (v >> 2) + 4 h, v = 0 .. 15 -- so those are the rows it takes:
//   2. four chunks g of 16 rows (the stands s0 + 8 g .. s0 + 8 g + 7, both p).  Lane (r, h) reads, of the rows of the stands 8 g + 4
//      h + u (u = 0 .. 3) and both p, the 16-byte word at column stand t0 + r: one wave instruction reads two rows of 512
//      consecutive bytes.  A word that is not needed -- above the diagonal, flagged, past the matrix -- is not loaded: the 16-byte
//      load becomes an 8-byte load of the other word, or none.  The products are written with explicit fmaf, so the compiler's
//      contraction has nothing to choose:
//          w = h_i conj(h_j):  wr = fma(hir, hjr, hii hji), wi = fma(hii, hjr, -(hir hji))
//          o = w V          :  or = fma(wr, Vr, -(wi Vi)),  oi = fma(wr, Vi, wi Vr);      then o -= M where p = q
//      The words go to out[row i] as 16-byte stores, and their conjugates into the LDS image [column j of the tile][row of the chunk]
//      (64 x 16 words at pitch CA_PITCH = 17); after a barrier (of one wave) the image is read along its rows, lane l taking the words
//      2 (l & 7), 2 (l & 7) + 1 of the row 8 e + (l >> 3), e = 0 .. 7, and stored to out[row j] as 16-byte words: 8 rows of 128
//      consecutive bytes per wave instruction.  In a diagonal tile the row store keeps i >= j and the mirrored store i > j (8-byte
//      stores where a 16-byte word straddles the diagonal), so every word has one owner there too.
// Every word is a fixed function of its own input word, the two factors and the model: it does not depend on nstand, on the other
// channels or on anything else that runs.  No atomics, no scalar memory writes, no printf.
//
// LDS banks.  The image is written by ds_write2_b64 (the words q = 0, 1 of a lane in one instruction; banks (a / 4) mod 32, groups of 16
// lanes): lane (r, h) writes word [2 r + q][2 (4 h + u) + p], 68 dwords apart across r = 4 banks, so the 16 lanes of a group fall on 8
// bank pairs two deep: 2-way.  It is read by ds_read2_b64 (two accesses, each in groups of 16 lanes, banks mod 32): the 8 lanes of a
// row take the dwords 4 k, 4 k + 1 (k = 0 .. 7) of that row, the second row of the group starts 34 dwords on and takes the banks 4 k +
// 2, 4 k + 3: no conflict.  At pitch 16 the two rows of a group would meet on the same banks.  The LDS carries 32 KiB each way per
// work-group beside 96 KiB of HBM traffic, at more than ten times HBM's rate per CU: the 2-way write is not on the critical path.
//
// calapply.hip is compiled with -fno-slp-vectorize (Makefile): complex fp32 arithmetic beside MFMA kernels, as image_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int CA_K = 32;            // sources at the most
constexpr int CA_T = 32;            // stands per tile (the rows and the columns of the 32x32 MFMA)
constexpr int CA_PAIRS = 8;         // k pairs per trip of the model's contraction: their loads are all in flight before the first MFMA
constexpr int CA_THREADS = 64;      // one wave
constexpr int CA_ROWS = 16;         // rows of a chunk
constexpr int CA_PITCH = 17;        // float2 per row of the mirrored image
constexpr int CA_MAX_NSTAND = 512;
constexpr int CA_STEER_THREADS = 256;

typedef float ca_f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr size_t calapply_lds_bytes() { return (size_t)2 * CA_T * CA_PITCH * sizeof(float2); }

// grid (ceil(nsrc nstand / CA_STEER_THREADS), nfine): a[c][k][s] from freq[c] and tau[k][s]
__global__ __launch_bounds__(CA_STEER_THREADS) void calapply_steer_kernel(const double* __restrict__ freq, const double* __restrict__ tau, float2* __restrict__ a,
                                                                          int nstand, int nsrc) {
    const size_t n = (size_t)nsrc * nstand, e = (size_t)blockIdx.x * CA_STEER_THREADS + threadIdx.x;
    if (e >= n) return;
    const double turns = __dmul_rn(freq[blockIdx.y], tau[e]);
    const float fr = (float)(turns - rint(turns));               // in [-1/2, 1/2]
    float sn, cs;
    sincospif(2.0f * fr, &sn, &cs);
    a[(size_t)blockIdx.y * n + e] = make_float2(cs, -sn);
}

// two words at p, p + 1 (p 16-byte aligned): both as one 16-byte store, one as an 8-byte store
__device__ __forceinline__ void ca_store2(float2* p, float2 w0, float2 w1, bool m0, bool m1) {
    if (m0 && m1)
        *(float4*)p = make_float4(w0.x, w0.y, w1.x, w1.y);
    else if (m0)
        p[0] = w0;
    else if (m1)
        p[1] = w1;
}

// grid (ntile (ntile + 1) / 2, nfine) with ntile = ceil(nstand / CA_T), CA_THREADS threads; vis and out 16-byte aligned
__global__ __launch_bounds__(CA_THREADS, 3) void calapply_kernel(const float2* __restrict__ vis, const float2* __restrict__ a, const float* __restrict__ flux,
                                                              const float2* __restrict__ hf, float2* __restrict__ out, int nstand, int nsrc) {
    __shared__ __attribute__((aligned(16))) float2 ca_lds[2 * CA_T * CA_PITCH];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int c = blockIdx.y;
    int S = 0, T = blockIdx.x;                                   // blockIdx.x = S (S + 1) / 2 + T, T <= S
    while (T > S) {
        T -= S + 1;
        S++;
    }
    const int s0 = S * CA_T, t0 = T * CA_T;
    const bool diag = S == T;
    const size_t ninput = 2 * (size_t)nstand;

    // 1. the model's tile
    ca_f32x16 mre = {}, mim = {};
    if (nsrc > 0) {
        const float2* ac = a + (size_t)c * nsrc * nstand;
        const float* fc = flux + (size_t)c * nsrc;
        for (int k0 = 0; k0 < nsrc; k0 += 2 * CA_PAIRS) {
            float2 z[CA_PAIRS], b[CA_PAIRS];
#pragma unroll
            for (int m = 0; m < CA_PAIRS; m++) {
                const int k = k0 + 2 * m + h;
                z[m] = b[m] = make_float2(0.f, 0.f);
                if (k < nsrc) {
                    const float f = fc[k];
                    if (s0 + r < nstand) {
                        const float2 as = ac[(size_t)k * nstand + s0 + r];
                        z[m] = make_float2(f * as.x, f * as.y);
                    }
                    if (t0 + r < nstand) b[m] = ac[(size_t)k * nstand + t0 + r];
                }
            }
#pragma unroll
            for (int m = 0; m < CA_PAIRS; m++) {
                if (k0 + 2 * m < nsrc) {                         // (uniform)
                    const float nzr = -z[m].x;
                    mre = __builtin_amdgcn_mfma_f32_32x32x2f32(z[m].x, b[m].x, mre, 0, 0, 0);
                    mre = __builtin_amdgcn_mfma_f32_32x32x2f32(z[m].y, b[m].y, mre, 0, 0, 0);
                    mim = __builtin_amdgcn_mfma_f32_32x32x2f32(z[m].y, b[m].x, mim, 0, 0, 0);
                    mim = __builtin_amdgcn_mfma_f32_32x32x2f32(nzr, b[m].y, mim, 0, 0, 0);
                }
            }
        }
    }

    // the factors of this lane's column stand
    const int t = t0 + r;
    const bool tin = t < nstand;
    float2 hj[2];
    bool lj[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        hj[q] = tin ? hf[((size_t)c * 2 + q) * nstand + t] : make_float2(0.f, 0.f);
        lj[q] = hj[q].x != 0.f || hj[q].y != 0.f;
    }
    const float2* vc = vis + (size_t)c * ninput * ninput;
    float2* oc = out + (size_t)c * ninput * ninput;

    // 2. the chunks
#pragma unroll
    for (int g = 0; g < 4; g++) {
        float4 v[8];
        float2 hi[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int u = e >> 1, p = e & 1;
            const int s = s0 + 8 * g + 4 * h + u, i = 2 * s + p;
            const bool s_in = s < nstand;
            hi[e] = s_in ? hf[((size_t)c * 2 + p) * nstand + s] : make_float2(0.f, 0.f);
            const bool li = hi[e].x != 0.f || hi[e].y != 0.f;
            const bool n0 = li && lj[0] && (!diag || 2 * t <= i), n1 = li && lj[1] && (!diag || 2 * t + 1 <= i);
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
            const int u = e >> 1, p = e & 1;
            const int s = s0 + 8 * g + 4 * h + u, i = 2 * s + p;
            const bool s_in = s < nstand;
            const bool li = hi[e].x != 0.f || hi[e].y != 0.f;
            float2 o[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int j = 2 * t + q;
                const float vr = q ? v[e].z : v[e].x, vi = q ? v[e].w : v[e].y;
                const float wr = __builtin_fmaf(hi[e].x, hj[q].x, hi[e].y * hj[q].y), wi = __builtin_fmaf(hi[e].y, hj[q].x, -(hi[e].x * hj[q].y));
                float yr = __builtin_fmaf(wr, vr, -(wi * vi)), yi = __builtin_fmaf(wr, vi, wi * vr);
                if (q == p && nsrc > 0) {
                    yr -= mre[4 * g + u];
                    yi -= mim[4 * g + u];
                }
                if (i == j) yi = 0.f;
                const bool live = li && lj[q];
                o[q] = live ? make_float2(yr, yi) : make_float2(0.f, 0.f);
                // the mirrored word: the conjugate, and +0 + 0i where the word is left out
                ca_lds[(2 * r + q) * CA_PITCH + 2 * (4 * h + u) + p] = live ? make_float2(yr, -yi) : make_float2(0.f, 0.f);
            }
            const bool in = s_in && tin;
            ca_store2(oc + (size_t)i * ninput + 2 * t, o[0], o[1], in && (!diag || 2 * t <= i), in && (!diag || 2 * t + 1 <= i));
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int jl = 8 * e + (lane >> 3), il = 2 * (lane & 7);
            const int j = 2 * t0 + jl, i = 2 * s0 + CA_ROWS * g + il;                   // out[j][i], out[j][i + 1]; i is even
            const float2 w0 = ca_lds[jl * CA_PITCH + il], w1 = ca_lds[jl * CA_PITCH + il + 1];
            const bool in = (size_t)j < ninput && (size_t)i < ninput;
            ca_store2(oc + (size_t)j * ninput + i, w0, w1, in && (!diag || i > j), in && (!diag || i + 1 > j));
        }
        __syncthreads();                                         // (the image has been read before the next chunk overwrites it)
    }
}

}  // namespace xeng
