// Component lists taken out of the visibilities (xengPredict*, predict.hip): UpchanCorr's matrix minus the visibility model of up to
// 4096 point components per channel group -- UpchanClean's own records, or any catalogue -- on all four polarisation products,
// written as a matrix of the same format: the major cycle of a Cotton-Schwab CLEAN.
//
// Contract (include/xeng.h, "Component lists subtracted from the visibilities"); ninput = 2 nstand, row i = 2 s + p, column j = 2 t + q:
//   vis    cf32[nfine][nstand][2][nstand][2], V[c][s p][t q]; only the words i >= j are read, never written
//   tau    f64[ndir][nstand], freq f64[nfine] (the context's state, SetGeometry)
//   rec    pr_record[ngroup][ncomp_max], nrec i32[ngroup] = one past the last filled record of a group (the context's state,
//          SetComponents); a record whose pixel is -1 is empty: zero operands
//   a_ks = exp(-2 pi i frac(freq[c] tau[pixel_k][s])): the fp64 product and its fp64 fraction of a turn, sincospif and everything
//          after fp32 -- the words of image_kernel, gaincal_kernel and calapply_steer_kernel, formed HERE, in registers, by the lane
//          that feeds them to the MFMA: cf32[nfine][ncomp][nstand] would be 1.1 GB at 96 x 4096 x 352, and every word of it is used by
//          one row of tiles only.  The state beyond the geometry is the records (32 bytes each) and nrec.
//   M_c[s p][t p] = sum_k C_k^pp a_ks conj(a_kt);  with CROSS  M_c[s 0][t 1] = sum_k (C_Re + i C_Im)_k a_ks conj(a_kt),
//                                                              M_c[s 1][t 0] = sum_k (C_Re - i C_Im)_k a_ks conj(a_kt)
//   out    cf32 in vis's layout.  i > j: V - M (model: M), one fp32 subtraction per part;  i = j: its real part and +0;  i < j: the
//          conjugate of out[c][j][i], not computed again.  Without CROSS the cross-hand words are V's (model: +0).
//
// predict_kernel<CROSS>: calapply_kernel's grid and output pass -- one work-group of ONE wave per (fine channel, pair of 32-stand tiles
// S >= T), grid (ntile (ntile + 1) / 2, nfine) -- around a record loop that forms its own operands:
//   1. the records two per v_mfma_f32_32x32x2_f32 in ascending order, PR_PAIRS pairs per trip.  Lane (r, h) takes the record k = 2 m +
//      h: a uniform load per half-wave (32 bytes; 16 without CROSS), then tau[pixel][s0 + r] and tau[pixel][t0 + r], 256 consecutive
//      bytes per half-wave each (one of them in a diagonal tile: a_t is a_s there).  All loads of a trip are issued before its first
//      phase factor.  Per pair and lane two phase factors, then per product four MFMAs with z = C a_s, b = a_t:
//          Mre += zr br,  Mre += zi bi,  Mim += zi br,  Mim += (-zr) bi        (the minus is an exact operand negation)
//      so per word and part one chain over k ascending: (k even, k odd) of the first product, then (k even, k odd) of the second --
//      CalApply's sequence.  z on the parallel hands is one multiply per part: (C ar, C ai).  On the cross hands, with C = C_Re, D = C_Im:
//          XY: zr = fma(C, ar, -(D ai)),  zi = fma(C, ai, D ar);        YX: zr = fma(C, ar, D ai),  zi = fma(C, ai, -(D ar))
//      An empty record, a record past nrec and a stand past nstand are zero operands (C = 0 and a = 0): fma(0, 0, M) = M.  The loop
//      ends at nrec rounded up to a pair: the cost follows the list, not ncomp_max.  Eight accumulator tiles with CROSS (128
//      registers), four without.  Lane (r, h) then holds M[s][t0 + r] of the 16 stands s = s0 + (v & 3) + 8 (v >> 2) + 4 h:
//   2. calapply_kernel's four chunks of 16 rows without its factors: lane (r, h) reads the 16-byte words (q = 0, 1) at column stand t0
//      + r of the rows of the stands 8 g + 4 h + u, both p (nothing in model mode; 8 bytes or nothing where a word lies above the
//      diagonal or past the matrix), subtracts, stores 16-byte words to out[row i] and the conjugates into the LDS image [column j of
//      the tile][row of the chunk] (64 x 16 words at pitch PR_PITCH = 17), which is read along its rows after a barrier (of one
//      wave) and stored to out[row j]: 8 rows of 128 consecutive bytes per wave instruction.  In a diagonal tile the row store keeps
//      i >= j and the mirrored store i > j, so every word has one owner.  The banks are calapply_kernel's: 2-way on the write, none
//      on the read.
// A word is a fixed function of its own input word, freq[c], the delays of its two stands and its group's records: no atomics, no
// scalar memory writes, no printf.  predict.hip is compiled with -fno-slp-vectorize (Makefile), as calapply.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int PR_T = 32;            // stands per tile (the rows and the columns of the 32x32 MFMA)
constexpr int PR_PAIRS = 8;         // record pairs per trip of the loop: their loads are all in flight before the first phase factor
constexpr int PR_THREADS = 64;      // one wave
constexpr int PR_ROWS = 16;         // rows of a chunk
constexpr int PR_PITCH = 17;        // float2 per row of the mirrored image
constexpr int PR_MAX_NSTAND = 512;
constexpr int PR_MAX_NCOMP = 4096;

typedef float pr_f32x16 __attribute__((ext_vector_type(16)));

// blocks/imaging.py CLEAN_COMPONENT, the record of clean_kernels.h
struct alignas(16) pr_record {
    int pixel;                      // an index into tau; -1: empty
    float I;                        // (ignored)
    float cxx, cyy, cre, cim;
    unsigned pad[2];
};
static_assert(sizeof(pr_record) == 32, "UpchanClean's record");

__host__ __device__ constexpr size_t predict_lds_bytes() { return (size_t)2 * PR_T * PR_PITCH * sizeof(float2); }

// exp(-2 pi i frac(f tau)) where live, else 0
__device__ __forceinline__ float2 pr_steer(double f, double tau, bool live) {
    const double turns = __dmul_rn(f, tau);
    const float fr = (float)(turns - rint(turns));               // in [-1/2, 1/2]
    float sn, cs;
    sincospif(2.0f * fr, &sn, &cs);
    return live ? make_float2(cs, -sn) : make_float2(0.f, 0.f);
}

// one product's four MFMAs of a record pair
__device__ __forceinline__ void pr_mac(pr_f32x16& mre, pr_f32x16& mim, float zr, float zi, float2 b) {
    const float nzr = -zr;
    mre = __builtin_amdgcn_mfma_f32_32x32x2f32(zr, b.x, mre, 0, 0, 0);
    mre = __builtin_amdgcn_mfma_f32_32x32x2f32(zi, b.y, mre, 0, 0, 0);
    mim = __builtin_amdgcn_mfma_f32_32x32x2f32(zi, b.x, mim, 0, 0, 0);
    mim = __builtin_amdgcn_mfma_f32_32x32x2f32(nzr, b.y, mim, 0, 0, 0);
}

// two words at p, p + 1 (p 16-byte aligned): both as one 16-byte store, one as an 8-byte store
__device__ __forceinline__ void pr_store2(float2* p, float2 w0, float2 w1, bool m0, bool m1) {
    if (m0 && m1)
        *(float4*)p = make_float4(w0.x, w0.y, w1.x, w1.y);
    else if (m0)
        p[0] = w0;
    else if (m1)
        p[1] = w1;
}

// grid (ntile (ntile + 1) / 2, nfine) with ntile = ceil(nstand / PR_T), PR_THREADS threads; vis and out 16-byte aligned; vis is not
// read where model != 0
template <bool CROSS>
__global__ __launch_bounds__(PR_THREADS, 2) void predict_kernel(const float2* __restrict__ vis, const double* __restrict__ freq, const double* __restrict__ tau,
                                                              const pr_record* __restrict__ rec, const int* __restrict__ nrec, float2* __restrict__ out,
                                                              int nstand, int nfavg, int ncomp_max, int model) {
    __shared__ __attribute__((aligned(16))) float2 pr_lds[2 * PR_T * PR_PITCH];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int c = blockIdx.y;
    int S = 0, T = blockIdx.x;                                   // blockIdx.x = S (S + 1) / 2 + T, T <= S
    while (T > S) {
        T -= S + 1;
        S++;
    }
    const int s0 = S * PR_T, t0 = T * PR_T;
    const bool diag = S == T;
    const size_t ninput = 2 * (size_t)nstand;
    const int t = t0 + r;
    const bool sin_ = s0 + r < nstand, tin = t < nstand;

    // 1. the model's tiles: XX, YY and with CROSS XY (s 0, t 1), YX (s 1, t 0)
    pr_f32x16 xxr = {}, xxi = {}, yyr = {}, yyi = {}, xyr = {}, xyi = {}, yxr = {}, yxi = {};
    {
        const int grp = c / nfavg;
        const int nr = nrec[grp];                                // one past the last filled record: <= ncomp_max
        const pr_record* rc = rec + (size_t)grp * ncomp_max;
        const double f = freq[c];
        for (int k0 = 0; k0 < nr; k0 += 2 * PR_PAIRS) {
            int px[PR_PAIRS];
            float cxx[PR_PAIRS], cyy[PR_PAIRS], cre[PR_PAIRS], cim[PR_PAIRS];
            double ts[PR_PAIRS], tt[PR_PAIRS];
#pragma unroll
            for (int m = 0; m < PR_PAIRS; m++) {
                const int k = k0 + 2 * m + h;
                px[m] = -1;
                cxx[m] = cyy[m] = cre[m] = cim[m] = 0.f;
                ts[m] = tt[m] = 0.0;
                if (k < nr) {
                    px[m] = rc[k].pixel;
                    if (px[m] >= 0) {
                        cxx[m] = rc[k].cxx;
                        cyy[m] = rc[k].cyy;
                        if (CROSS) {
                            cre[m] = rc[k].cre;
                            cim[m] = rc[k].cim;
                        }
                        const double* tp = tau + (size_t)px[m] * nstand;
                        if (sin_) ts[m] = tp[s0 + r];
                        if (!diag && tin) tt[m] = tp[t];
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < PR_PAIRS; m++) {
                if (k0 + 2 * m < nr) {                           // (uniform)
                    const bool live = px[m] >= 0;
                    const float2 as = pr_steer(f, ts[m], live && sin_);
                    float2 at = as;
                    if (!diag) at = pr_steer(f, tt[m], live && tin);
                    pr_mac(xxr, xxi, cxx[m] * as.x, cxx[m] * as.y, at);
                    pr_mac(yyr, yyi, cyy[m] * as.x, cyy[m] * as.y, at);
                    if (CROSS) {
                        pr_mac(xyr, xyi, __builtin_fmaf(cre[m], as.x, -(cim[m] * as.y)), __builtin_fmaf(cre[m], as.y, cim[m] * as.x), at);
                        pr_mac(yxr, yxi, __builtin_fmaf(cre[m], as.x, cim[m] * as.y), __builtin_fmaf(cre[m], as.y, -(cim[m] * as.x)), at);
                    }
                }
            }
        }
    }

    const float2* vc = vis + (size_t)c * ninput * ninput;
    float2* oc = out + (size_t)c * ninput * ninput;

    // 2. the chunks
#pragma unroll
    for (int g = 0; g < 4; g++) {
        float4 v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int u = e >> 1, p = e & 1;
            const int s = s0 + 8 * g + 4 * h + u, i = 2 * s + p;
            const bool in = s < nstand && tin && !model;
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
            const int u = e >> 1, p = e & 1;
            const int s = s0 + 8 * g + 4 * h + u, i = 2 * s + p;
            float2 o[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int j = 2 * t + q;
                float yr = q ? v[e].z : v[e].x, yi = q ? v[e].w : v[e].y;
                if (q == p || CROSS) {
                    const float mr = q == p ? (p ? yyr[4 * g + u] : xxr[4 * g + u]) : (p ? yxr[4 * g + u] : xyr[4 * g + u]);
                    const float mi = q == p ? (p ? yyi[4 * g + u] : xxi[4 * g + u]) : (p ? yxi[4 * g + u] : xyi[4 * g + u]);
                    if (model) {
                        yr = mr;
                        yi = mi;
                    } else {
                        yr -= mr;
                        yi -= mi;
                    }
                }
                if (i == j) yi = 0.f;
                o[q] = make_float2(yr, yi);
                pr_lds[(2 * r + q) * PR_PITCH + 2 * (4 * h + u) + p] = make_float2(yr, -yi);        // the mirrored word: the conjugate
            }
            const bool in = s < nstand && tin;
            pr_store2(oc + (size_t)i * ninput + 2 * t, o[0], o[1], in && (!diag || 2 * t <= i), in && (!diag || 2 * t + 1 <= i));
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int jl = 8 * e + (lane >> 3), il = 2 * (lane & 7);
            const int j = 2 * t0 + jl, i = 2 * s0 + PR_ROWS * g + il;                   // out[j][i], out[j][i + 1]; i is even
            const float2 w0 = pr_lds[jl * PR_PITCH + il], w1 = pr_lds[jl * PR_PITCH + il + 1];
            const bool in = (size_t)j < ninput && (size_t)i < ninput;
            pr_store2(oc + (size_t)j * ninput + i, w0, w1, in && (!diag || i > j), in && (!diag || i + 1 > j));
        }
        __syncthreads();                                         // (the image has been read before the next chunk overwrites it)
    }
}

}  // namespace xeng
