// Running-median baseline removal of the dedispersed beams (xengDetrend*, detrend.hip): per (pair, DM trial) series and per block
// of nblk windows a knot {median, median absolute deviation}, and then, 3 nblk / 2 windows late, every window minus the line between
// the two knots around it, with `normalise` times the line between their reciprocal scales.
//
// Contract (include/xeng.h, "Baseline removal of the dedispersed beams"); nser = npair*ndm, h = nblk/2, D = 3h, L = D + nwin:
//   in     f32[nc][nser][nprod], xengDedispRun's output; z = in[..][0] at nprod 1, fl(XX + YY) at nprod 4; never written
//   ring   f32[nser][L]: window n of series s at ring[s L + n mod L], time the fastest axis
//   knots  DT_KNOTS = 4 slots of {M, A, G} f32[nser] and a valid byte u8[nser]: block k in slot k & 3 (a call reads the knots of at
//          most three blocks, and the newest of them is decided inside that call)
//   out    f32[nc][nser]
//
// Ingest, every call: a work-group moves a tile of 32 series x 32 windows: loads consecutive across lanes along the series (4 or
// 16 bytes a lane), through LDS (rows padded by one word), 4-byte stores consecutive across lanes along time (dedisp_ingest_kernel's
// scheme).
//
// Decide, on the call that takes a block's last window, one work-group per series: the block's nblk values go into LDS as sortable
// keys of fl(z + 0) (consecutive lanes read consecutive ring words).  The keys of ranks nblk/2 - 1 and nblk/2 are found together by
// a search on the key, bit by bit from the top: K grows by a bit whenever the count of keys below K | bit does not exceed the rank;
// the largest such K is the key of that rank.  A pass is one LDS read per key (lane-consecutive words), two compares, a sum over
// the work-group in an integer counter in LDS (one add per thread with a count, one barrier): 32 passes of nblk / 256 reads per
// thread, whatever the data, ties included.  The values come back from the keys (the key is a bijection of fl(z + 0)).
// The deviations |fl(z - M)| take the keys' place -- formed from fl(z + 0): the same number, since a zero of either sign minus M differs from the other only where M = +0, and there only
// in the sign that the absolute value drops -- and the same search gives A.  Thread 0 writes the knot.
//
// Apply, every call: a tile of 32 series x 32 output windows.  Lanes along time read the ring into LDS, then lanes along the series
// read the knots (consecutive words), form y and store it (consecutive words).  The knots of an output window depend on the window
// alone: k = k0 + carry, t = e - carry nblk with e = e0 + i, where the host gives k0 = n0 div nblk - 2 and e0 = n0 mod nblk.
// A lane outside the series or the call's windows reads nothing.
//
// No float atomics: the one atomic is the integer add to the count word in LDS; every other word has one owner; no work-group
// waits for another; size_t index arithmetic.  Nothing is contracted into an fma: the arithmetic is written in dt_add / dt_sub /
// dt_mul / dt_div, plain operators under `fp contract(off)` (rfi_kernels.h says why not __f*_rn).  Division is correctly rounded in hipcc's default build.
//
// detrend.hip is compiled with -fno-slp-vectorize (Makefile), with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

#pragma clang fp contract(off)

constexpr int DT_THREADS = 256;
constexpr int DT_TILE = 32;             // ingest and apply tile: series x windows
constexpr int DT_KNOTS = 4;             // slots of the knot ring
constexpr float DT_FLT_MAX = 3.402823466e+38f;
constexpr size_t DT_TILE_LDS_BYTES = (size_t)DT_TILE * (DT_TILE + 1) * sizeof(float);
// the keys and three count words that the passes take in turn
inline size_t detrend_decide_lds_bytes(int nblk) { return ((size_t)nblk + 3) * sizeof(float); }

struct DetrendKnots {
    float* M;               // [DT_KNOTS][nser]
    float* A;               // [DT_KNOTS][nser]
    float* G;               // [DT_KNOTS][nser], +0 where the knot is not valid or nothing is normalised
    unsigned char* valid;   // [DT_KNOTS][nser]
};

// one rounding each: this file's operators are not contracted (the pragma above)
__device__ __forceinline__ float dt_add(float a, float b) { return a + b; }
__device__ __forceinline__ float dt_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float dt_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float dt_div(float a, float b) { return a / b; }

__device__ __forceinline__ bool dt_finite(float x) { return __builtin_fabsf(x) <= DT_FLT_MAX; }     // false for NaN and Inf

// monotonic over the floats that are not NaN, -0 taken as +0 (rfi_kernels.h rf_key), and its inverse
__device__ __forceinline__ unsigned dt_key(float v) {
    const unsigned u = __float_as_uint(dt_add(v, 0.f));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dt_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// The sum of c over the work-group's 256 threads in an integer counter in LDS: cnt[set] takes the adds of this call, and thread 0
// clears cnt[set + 1 mod 3] for the next one (its last readers passed the barrier of the call before this one; its next adders
// start behind this call's barrier).  Every thread calls it, with set = 0, 1, 2, 0, .. from call to call, cnt[0] cleared and
// published before the first; its barrier also publishes what the threads wrote to LDS before the call.
__device__ __forceinline__ unsigned dt_block_sum(unsigned c, unsigned* cnt, int set) {
    if (c) atomicAdd(&cnt[set], c);
    if (threadIdx.x == 0) cnt[set == 2 ? 0 : set + 1] = 0;
    __syncthreads();
    return cnt[set];
}

// The median of the values whose keys are k[0 .. nblk), nblk even: fl(0.5f fl(lo + hi)) of the values of ranks nblk/2 - 1 and
// nblk/2.  The low half of a count word counts the keys below the lower rank's trial key, the high half those below the upper
// one's (nblk <= 8192: neither half carries).  The passes take the count sets set, set + 1, .. mod 3, and the next call set + 2
// mod 3 (32 passes).
__device__ __forceinline__ float dt_median(const unsigned* k, unsigned* cnt, int nblk, int set) {
    const unsigned rlo = (unsigned)(nblk / 2 - 1), rhi = (unsigned)(nblk / 2);
    unsigned klo = 0, khi = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const unsigned tlo = klo | (1u << bit), thi = khi | (1u << bit);
        unsigned c = 0;
        for (int q = threadIdx.x; q < nblk; q += DT_THREADS) {
            const unsigned x = k[q];
            c += (x < tlo ? 1u : 0u) + (x < thi ? 0x10000u : 0u);
        }
        c = dt_block_sum(c, cnt, set);
        set = set == 2 ? 0 : set + 1;
        if ((c & 0xFFFFu) <= rlo) klo = tlo;
        if ((c >> 16) <= rhi) khi = thi;
    }
    return dt_mul(0.5f, dt_add(dt_unkey(klo), dt_unkey(khi)));
}

// grid (ceil(nser / 32), ceil(nc / 32)), 256 threads, DT_TILE_LDS_BYTES of dynamic LDS; slot0 = n0 mod L, the slot of the call's
// first window
template <int NPROD>
__global__ __launch_bounds__(256) void detrend_ingest_kernel(const float* __restrict__ in, float* __restrict__ ring, int nser, int L, int slot0, int nc) {
    extern __shared__ float dt_lds[];
    float* tile = dt_lds;                           // [32 series][33]
    const int s0 = blockIdx.x * DT_TILE, t0 = blockIdx.y * DT_TILE;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    for (int i = 0; i < DT_TILE / 8; i++) {
        const int tt = hi + 8 * i, t = t0 + tt, s = s0 + lo;
        if (t < nc && s < nser) {
            float z;
            if constexpr (NPROD == 1) {
                z = in[(size_t)t * nser + s];
            } else {
                const float4 v = ((const float4*)in)[(size_t)t * nser + s];
                z = dt_add(v.x, v.y);
            }
            tile[lo * (DT_TILE + 1) + tt] = z;
        }
    }
    __syncthreads();
    const int t = t0 + lo;
    if (t >= nc) return;
    int slot = slot0 + t;                           // (slot0 < L and t < nwin <= L)
    slot -= slot >= L ? L : 0;
    for (int i = 0; i < DT_TILE / 8; i++) {
        const int ss = hi + 8 * i, s = s0 + ss;
        if (s >= nser) break;
        ring[(size_t)s * L + slot] = tile[ss * (DT_TILE + 1) + lo];
    }
}

// grid nser, 256 threads, detrend_decide_lds_bytes(nblk) of dynamic LDS; after the ingest that took the block's last window, on the
// same stream.  slotb = the slot of the block's first window, kslot = block & 3.
__global__ __launch_bounds__(256) void detrend_decide_kernel(const float* __restrict__ ring, DetrendKnots kn, int nser, int nblk, int L, int slotb, int kslot,
                                                             int normalise, float k_mad) {
    extern __shared__ float dt_lds[];
    unsigned* dt_k = (unsigned*)dt_lds;             // [nblk]: the keys of z, then of |z - M|
    unsigned* dt_cnt = dt_k + nblk;                 // [3]
    const int tid = threadIdx.x;
    const size_t s = blockIdx.x;
    const float* row = ring + s * L;
    if (tid == 0) dt_cnt[0] = 0;
    __syncthreads();
    unsigned bad = 0;
    for (int q = tid; q < nblk; q += DT_THREADS) {
        int slot = slotb + q;                       // (slotb < L and q < nblk < L)
        slot -= slot >= L ? L : 0;
        const float z = row[slot];
        bad += dt_finite(z) ? 0u : 1u;
        dt_k[q] = dt_key(z);
    }
    bad = dt_block_sum(bad, dt_cnt, 0);
    const size_t at = (size_t)kslot * nser + s;
    if (bad) {                                      // (the same in every thread)
        if (tid == 0) {
            kn.M[at] = 0.f;
            kn.A[at] = 0.f;
            kn.G[at] = 0.f;
            kn.valid[at] = 0;
        }
        return;
    }
    const float M = dt_median(dt_k, dt_cnt, nblk, 1);           // (sets 1, 2, 0, .. 2: 32 passes end on set 2)
    // (every thread has read the keys for the last time before the last pass's barrier: the keys of the deviations take their place)
    for (int q = tid; q < nblk; q += DT_THREADS) dt_k[q] = dt_key(__builtin_fabsf(dt_sub(dt_unkey(dt_k[q]), M)));
    __syncthreads();
    const float A = dt_median(dt_k, dt_cnt, nblk, 0);
    if (tid == 0) {
        float G = 0.f;
        bool ok = true;
        if (normalise) {
            const float sc = dt_mul(k_mad, A);
            ok = sc > 0.f && sc <= DT_FLT_MAX;
            if (ok) G = dt_div(1.0f, sc);
        }
        kn.M[at] = M;
        kn.A[at] = A;
        kn.G[at] = G;
        kn.valid[at] = ok ? 1 : 0;
    }
}

// grid (ceil(nser / 32), ceil(nc / 32)), 256 threads, DT_TILE_LDS_BYTES of dynamic LDS.  Output window i is the detrended window
// m = n0 + i - D: with e = e0 + i (e0 = n0 mod nblk) and carry = e >= nblk, k = k0 + carry (k0 = n0 div nblk - 2) and
// t = e - carry nblk; m < 0 iff k < -1 or k = -1 and t < h.  slotm0 = (n0 - D) mod L (floored), the slot of output window 0.
// r = 1.0f / (float)(2 nblk).
__global__ __launch_bounds__(256) void detrend_apply_kernel(const float* __restrict__ ring, DetrendKnots kn, float* __restrict__ out, int nser, int nblk, int L,
                                                            int nc, long long k0, int e0, int slotm0, int normalise, float r) {
    extern __shared__ float dt_lds[];
    float* tile = dt_lds;                           // [32 series][33]
    const int s0 = blockIdx.x * DT_TILE, t0 = blockIdx.y * DT_TILE;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const int h = nblk >> 1;
    {
        const int i = t0 + lo;
        const int e = e0 + i;
        const int carry = e >= nblk ? 1 : 0;
        const long long k = k0 + carry;
        const int t = e - carry * nblk;
        if (i < nc && (k > -1 || (k == -1 && t >= h))) {        // (a window before the reset is not in the ring)
            int slot = slotm0 + i;                  // (slotm0 < L and i < nwin <= L)
            slot -= slot >= L ? L : 0;
            for (int j = 0; j < DT_TILE / 8; j++) {
                const int ss = hi + 8 * j, s = s0 + ss;
                if (s >= nser) break;
                tile[ss * (DT_TILE + 1) + lo] = ring[(size_t)s * L + slot];
            }
        }
    }
    __syncthreads();
    const int s = s0 + lo;
    if (s >= nser) return;
    for (int j = 0; j < DT_TILE / 8; j++) {
        const int tt = hi + 8 * j, i = t0 + tt;
        if (i >= nc) break;
        const int e = e0 + i;
        const int carry = e >= nblk ? 1 : 0;
        const long long k = k0 + carry;
        const int t = e - carry * nblk;
        float y = 0.f;
        if (k > -1 || (k == -1 && t >= h)) {
            const size_t a = (size_t)((k < 0 ? 0 : k) & (DT_KNOTS - 1)) * nser + s, b = (size_t)((k + 1) & (DT_KNOTS - 1)) * nser + s;
            const bool va = kn.valid[a] != 0, vb = kn.valid[b] != 0;
            if (va || vb) {
                const size_t ia = va ? a : b, ib = vb ? b : a;
                const float z = tile[lo * (DT_TILE + 1) + tt];
                const float u = dt_mul((float)(2 * t + 1), r);
                const float Ma = kn.M[ia], Mb = kn.M[ib];
                y = dt_sub(z, dt_add(Ma, dt_mul(u, dt_sub(Mb, Ma))));
                if (normalise) {
                    const float Ga = kn.G[ia], Gb = kn.G[ib];
                    y = dt_mul(y, dt_add(Ga, dt_mul(u, dt_sub(Gb, Ga))));
                }
                if (!dt_finite(y)) y = 0.f;
            }
        }
        out[(size_t)i * nser + s] = y;
    }
}

}  // namespace xeng
