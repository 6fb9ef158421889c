// Cleaning of the fine-channel power beams (xengRfi*, rfi.hip): per block of nstat windows a bandpass (mean and variance per pair,
// channel and word), a robust test of the channels on the variance of the total power over its squared mean, and then, nstat
// windows late, every window normalised, clipped, tested for a broadband excess and freed of its mean over the channels.
//
// Contract (include/xeng.h, "Cleaning of the fine-channel power beams"); NC = npair*nfine, L = nstat + nwin:
//   in     f32[nc][npair][nfine][4] = [XX, YY, Re XY*, Im XY*], one float4 per (window, pair, channel); never written
//   ring   float4[L][NC]: window n sits in slot n mod L
//   run    float4[3][NC]: the running {c}, {a}, {s_0, s_1, 0, 0} of the block in progress
//   tab    two halves of block tables, block k in half k & 1 (RfiTables): {c, m, g} float4[NC], v float2[NC], {mu, V, R} f32[NC],
//          the flag byte per channel, the count of channels not kept per pair
//   out    as in; stats i32[nc][npair][4]
//
// Ingest, every call: lane = channel, adjacent lanes load adjacent 16-byte words.  A thread walks the call's windows in ascending n,
// copies each into its ring slot and carries the four chains in registers; at a block's last window it writes {c, m, v} to the
// half k & 1 and the next window starts the chains again.  The running state is read once (unless the call begins a block) and
// written once.
//
// Decide, on the call that completes a block, one work-group per pair: mu, V, R and the live test per channel, the sortable keys
// of R in LDS (RF_DEAD where a channel is not live), the median by exact rank selection (the key's rank is the count of keys below
// it, ties by index: nfine compares per key, four keys per 16-byte LDS read, the same address in every lane: a broadcast), the keys
// of |R - med|, their median, then flags and gains.  A thread keeps no per-channel array: R comes back from the table it wrote.
//
// Apply, one work-group of 256 per (output window, pair): thread t owns channels t, t + 256, ... -- the chain order of the
// contract --, forms y and the clip, adds its chains, then the tree through LDS (8 barriers; the six 4-byte rows are 256 words
// each: consecutive lanes read consecutive words, and t + h for h >= 32 is the same bank pattern shifted by whole rows of 32: no
// conflict).  A second sweep forms y again from the ring and the tables (they sit in L2) and writes out; thread 0 writes the
// 16-byte stats record.
//
// No atomics; every word has one owner; no work-group waits for another; size_t index arithmetic.  Nothing is contracted into an
// fma: the arithmetic is written in rf_add / rf_sub / rf_mul / rf_div, plain operators under `fp contract(off)`.  (__fmul_rn and
// __fadd_rn are plain operators too in this ROCm's headers, but compiled under the headers' own contraction rule: a product in one
// and a sum in the other may fuse once both are inlined, and s + d*d and s*r - m*m here are such pairs.)  Division and square root are correctly
// rounded in hipcc's default build (-fhip-fp32-correctly-rounded-divide-sqrt), which the Makefile does not turn off.
//
// rfi.hip is compiled with -fno-slp-vectorize (Makefile), with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

#pragma clang fp contract(off)

constexpr int RF_THREADS = 256;
constexpr int RF_MAX_NFINE = 8192;
constexpr unsigned RF_DEAD = 0xFFFFFFFFu;
constexpr float RF_FLT_MAX = 3.402823466e+38f;
constexpr size_t RF_APPLY_LDS_BYTES = 6 * RF_THREADS * sizeof(float);
inline size_t rfi_decide_lds_bytes(int nfine) { return ((size_t)((nfine + 3) & ~3) + 2 + RF_THREADS) * sizeof(float); }

struct RfiTables {
    float4* c;              // [NC]
    float4* m;              // [NC]
    float4* g;              // [NC], +0 where the channel is not kept
    float2* v;              // [NC]
    float* mu;              // [NC]
    float* var;             // [NC]
    float* r;               // [NC]
    int* notkept;           // [npair]
    unsigned char* flag;    // [NC]: bit 0 mask, bit 1 not live for another reason, bit 2 outlier
};

struct RfiControl {
    float t_clip, t_broad;
    int min_count, zerodm;
};

struct RfiControl2 {
    RfiControl h[2];
};

struct RfiTables2 {
    RfiTables h[2];
};

// one rounding each: this file's operators are not contracted (the pragma above)
__device__ __forceinline__ float rf_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rf_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float rf_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rf_div(float a, float b) { return a / b; }

// the tables of one half, picked without indexing the kernel's arguments by a variable
__device__ __forceinline__ RfiTables rf_pick(const RfiTables2& t, int half) {
    RfiTables o;
    o.c = half ? t.h[1].c : t.h[0].c;
    o.m = half ? t.h[1].m : t.h[0].m;
    o.g = half ? t.h[1].g : t.h[0].g;
    o.v = half ? t.h[1].v : t.h[0].v;
    o.mu = half ? t.h[1].mu : t.h[0].mu;
    o.var = half ? t.h[1].var : t.h[0].var;
    o.r = half ? t.h[1].r : t.h[0].r;
    o.notkept = half ? t.h[1].notkept : t.h[0].notkept;
    o.flag = half ? t.h[1].flag : t.h[0].flag;
    return o;
}

__device__ __forceinline__ bool rf_finite(float x) { return __builtin_fabsf(x) <= RF_FLT_MAX; }     // false for NaN and Inf

// monotonic over the finite floats, -0 taken as +0 (flag_kernels.h fl_key)
__device__ __forceinline__ unsigned rf_key(float v) {
    const unsigned u = __float_as_uint(rf_add(v, 0.f));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The rank of key kv at index `at` among k[0 .. 4 n4): the count of keys below it, ties by index (flag_kernels.h fl_rank).
// rf_rank(k, n4, RF_DEAD, 0) counts the live keys.
__device__ __forceinline__ int rf_rank(const unsigned* k, int n4, unsigned kv, int at) {
    const int qs = at >> 2, j = at & 3;
    int rank = 0;
    for (int q = 0; q < n4; q++) {
        const uint4 x = ((const uint4*)k)[q];
        const unsigned thr = q < qs ? kv + 1u : kv;
        rank += (x.x < thr ? 1 : 0) + (x.y < thr ? 1 : 0) + (x.z < thr ? 1 : 0) + (x.w < thr ? 1 : 0);
    }
    const uint4 x = ((const uint4*)k)[qs];
    rank += (j > 0 && x.x == kv ? 1 : 0) + (j > 1 && x.y == kv ? 1 : 0) + (j > 2 && x.z == kv ? 1 : 0);
    return rank;
}

// The median of val[q] over the channels whose keys in rf_k[0 .. 4 n4) are not RF_DEAD (rf_k[q] = rf_key(val[q]) there): the
// values of rank (n - 1) / 2 and n / 2, 0.5f (lo + hi) for even n, +0 for n = 0.  val(q) gives the value again.  Every thread
// of the work-group calls it; the keys were written before a barrier.
template <class F>
__device__ __forceinline__ float rf_median(const unsigned* rf_k, float* rf_cs, F val, int nfine) {
    const int n4 = (nfine + 3) >> 2;
    const int n = rf_rank(rf_k, n4, RF_DEAD, 0);
    for (int q = threadIdx.x; q < nfine; q += RF_THREADS) {
        if (rf_k[q] == RF_DEAD) continue;
        const int rank = rf_rank(rf_k, n4, rf_k[q], q);
        if (rank == (n - 1) / 2) rf_cs[0] = val(q);
        if (rank == n / 2) rf_cs[1] = val(q);
    }
    __syncthreads();
    const float lo = rf_cs[0], hi = rf_cs[1];
    __syncthreads();
    return n == 0 ? 0.f : (n & 1) ? hi : rf_mul(0.5f, rf_add(lo, hi));
}

// grid ceil(NC / 256), 256 threads.  The call's windows are n0 .. n0 + nc - 1: pos0 = n0 mod nstat, slot0 = n0 mod L, half0 =
// (n0 / nstat) & 1.  r = 1.0f / (float)nstat.
__global__ __launch_bounds__(256) void rfi_ingest_kernel(const float4* __restrict__ in, float4* __restrict__ ring, float4* __restrict__ run, RfiTables2 tab,
                                                         size_t NC, int nc, int nstat, int L, int pos0, int slot0, int half0, float r) {
    const size_t e = (size_t)blockIdx.x * RF_THREADS + threadIdx.x;
    if (e >= NC) return;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f), a = c;
    float s0 = 0.f, s1 = 0.f;
    if (pos0 != 0) {
        c = run[e];
        a = run[NC + e];
        const float4 s = run[2 * NC + e];
        s0 = s.x;
        s1 = s.y;
    }
    int pos = pos0, slot = slot0, half = half0;
    for (int i = 0; i < nc; i++) {
        const float4 x = in[(size_t)i * NC + e];
        ring[(size_t)slot * NC + e] = x;
        if (pos == 0) {
            c = x;
            a = make_float4(0.f, 0.f, 0.f, 0.f);
            s0 = s1 = 0.f;
        }
        const float d0 = rf_sub(x.x, c.x), d1 = rf_sub(x.y, c.y), d2 = rf_sub(x.z, c.z), d3 = rf_sub(x.w, c.w);
        a.x = rf_add(a.x, d0);
        a.y = rf_add(a.y, d1);
        a.z = rf_add(a.z, d2);
        a.w = rf_add(a.w, d3);
        s0 = rf_add(s0, rf_mul(d0, d0));
        s1 = rf_add(s1, rf_mul(d1, d1));
        if (pos == nstat - 1) {
            const RfiTables t = rf_pick(tab, half);
            const float4 m = make_float4(rf_mul(a.x, r), rf_mul(a.y, r), rf_mul(a.z, r), rf_mul(a.w, r));
            t.c[e] = c;
            t.m[e] = m;
            t.v[e] = make_float2(rf_sub(rf_mul(s0, r), rf_mul(m.x, m.x)), rf_sub(rf_mul(s1, r), rf_mul(m.y, m.y)));
            pos = 0;
            half ^= 1;
        } else {
            pos++;
        }
        slot = slot + 1 == L ? 0 : slot + 1;
    }
    run[e] = c;
    run[NC + e] = a;
    run[2 * NC + e] = make_float4(s0, s1, 0.f, 0.f);
}

// grid npair, 256 threads, rfi_decide_lds_bytes(nfine) of dynamic LDS; after the ingest that completed the block, on the same
// stream.  mask: u8[nfine].
__global__ __launch_bounds__(256) void rfi_decide_kernel(RfiTables t, const unsigned char* __restrict__ mask, int nfine, float k_chan) {
    extern __shared__ float rf_lds[];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * nfine;
    const int n4 = (nfine + 3) >> 2;
    unsigned* rf_k = (unsigned*)rf_lds;             // [4 n4]: the keys of R, then of |R - med|
    float* rf_cs = rf_lds + 4 * n4;                 // [2]
    int* rf_cnt = (int*)(rf_cs + 2);                // [256]
    for (int q = tid; q < 4 * n4; q += RF_THREADS) {
        unsigned key = RF_DEAD;
        if (q < nfine) {
            const float4 c = t.c[base + q], m = t.m[base + q];
            const float2 v = t.v[base + q];
            const float mu = rf_add(rf_add(c.x, m.x), rf_add(c.y, m.y));
            const float V = rf_add(v.x, v.y);
            const float R = rf_div(V, rf_mul(mu, mu));
            t.mu[base + q] = mu;
            t.var[base + q] = V;
            t.r[base + q] = R;
            const bool ok = rf_finite(m.x) && rf_finite(m.y) && rf_finite(m.z) && rf_finite(m.w) && v.x > 0.f && v.x <= RF_FLT_MAX && v.y > 0.f &&
                            v.y <= RF_FLT_MAX && mu > 0.f && rf_finite(R);
            const unsigned char f = (unsigned char)((mask[q] ? 1 : 0) | (ok ? 0 : 2));
            t.flag[base + q] = f;
            if (f == 0) key = rf_key(R);
        }
        rf_k[q] = key;
    }
    __syncthreads();
    const float med = rf_median(rf_k, rf_cs, [&](int q) { return t.r[base + q]; }, nfine);
    // (every thread has read its keys for the last time before the median's barriers: the keys of the deviations take their place)
    for (int q = tid; q < nfine; q += RF_THREADS)
        if (rf_k[q] != RF_DEAD) rf_k[q] = rf_key(__builtin_fabsf(rf_sub(t.r[base + q], med)));
    __syncthreads();
    const float mad = rf_median(rf_k, rf_cs, [&](int q) { return __builtin_fabsf(rf_sub(t.r[base + q], med)); }, nfine);
    const float thr = rf_mul(k_chan, mad);
    int notkept = 0;
    for (int q = tid; q < nfine; q += RF_THREADS) {
        unsigned char f = t.flag[base + q];
        if (f == 0 && __builtin_fabsf(rf_sub(t.r[base + q], med)) > thr) f = 4;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f == 0) {
            const float2 v = t.v[base + q];
            g.x = rf_div(1.f, __builtin_sqrtf(v.x));
            g.y = rf_div(1.f, __builtin_sqrtf(v.y));
            g.z = g.w = __builtin_sqrtf(rf_mul(g.x, g.y));
        } else {
            notkept++;
        }
        t.flag[base + q] = f;
        t.g[base + q] = g;
    }
    rf_cnt[tid] = notkept;
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < RF_THREADS; i++) n += rf_cnt[i];
        t.notkept[blockIdx.x] = n;
    }
}

// y of one sample of a kept channel; false when it is clipped
__device__ __forceinline__ bool rf_sample(const float4 x, const float4 c, const float4 m, const float4 g, float t_clip, float4& y) {
    y.x = rf_mul(rf_sub(rf_sub(x.x, c.x), m.x), g.x);
    y.y = rf_mul(rf_sub(rf_sub(x.y, c.y), m.y), g.y);
    y.z = rf_mul(rf_sub(rf_sub(x.z, c.z), m.z), g.z);
    y.w = rf_mul(rf_sub(rf_sub(x.w, c.w), m.w), g.w);
    const float z = rf_add(y.x, y.y);
    return rf_finite(y.x) && rf_finite(y.y) && rf_finite(y.z) && rf_finite(y.w) && __builtin_fabsf(z) <= t_clip;
}

// grid (nc, npair), 256 threads, RF_APPLY_LDS_BYTES of dynamic LDS.  Output window i is the cleaned window nsrc0 + i (nsrc0 = n0 - nstat, negative before the first
// block): its block is k = (nsrc0 + i) / nstat, its tables and controls those of half k & 1, its ring slot (nsrc0 + i) mod L.
__global__ __launch_bounds__(256) void rfi_apply_kernel(const float4* __restrict__ ring, RfiTables2 tab, RfiControl2 ctl, float4* __restrict__ out,
                                                        int* __restrict__ stats, int nfine, int npair, int nstat, int L, long long nsrc0) {
    extern __shared__ float rf_lds[];
    float* rf_p = rf_lds;                           // [4][256]
    int* rf_n = (int*)(rf_lds + 4 * RF_THREADS);    // [2][256]
    const int tid = threadIdx.x;
    const size_t p = blockIdx.y;
    const size_t NC = (size_t)npair * nfine;
    float4* o = out + ((size_t)blockIdx.x * npair + p) * nfine;
    int* st = stats + ((size_t)blockIdx.x * npair + p) * 4;
    const long long n = nsrc0 + (long long)blockIdx.x;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n < 0) {
        for (int q = tid; q < nfine; q += RF_THREADS) o[q] = zero;
        if (tid == 0) *(int4*)st = make_int4(0, 0, 4, 0);
        return;
    }
    const int half = (int)((n / nstat) & 1);
    const RfiTables t = rf_pick(tab, half);
    RfiControl k;
    k.t_clip = half ? ctl.h[1].t_clip : ctl.h[0].t_clip;
    k.t_broad = half ? ctl.h[1].t_broad : ctl.h[0].t_broad;
    k.min_count = half ? ctl.h[1].min_count : ctl.h[0].min_count;
    k.zerodm = half ? ctl.h[1].zerodm : ctl.h[0].zerodm;
    const float4* x = ring + (size_t)(n % L) * NC + p * nfine;
    const size_t base = p * nfine;
    float4 acc = zero;
    int count = 0, clipped = 0;
    for (int q = tid; q < nfine; q += RF_THREADS) {
        float4 y = zero;
        if (t.flag[base + q] == 0) {
            if (rf_sample(x[q], t.c[base + q], t.m[base + q], t.g[base + q], k.t_clip, y)) {
                count++;
            } else {
                clipped++;
                y = zero;
            }
        }
        acc.x = rf_add(acc.x, y.x);
        acc.y = rf_add(acc.y, y.y);
        acc.z = rf_add(acc.z, y.z);
        acc.w = rf_add(acc.w, y.w);
    }
    rf_p[tid] = acc.x;
    rf_p[1 * RF_THREADS + tid] = acc.y;
    rf_p[2 * RF_THREADS + tid] = acc.z;
    rf_p[3 * RF_THREADS + tid] = acc.w;
    rf_n[tid] = count;
    rf_n[RF_THREADS + tid] = clipped;
    __syncthreads();
    for (int h = RF_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            rf_p[tid] = rf_add(rf_p[tid], rf_p[tid + h]);
            rf_p[1 * RF_THREADS + tid] = rf_add(rf_p[1 * RF_THREADS + tid], rf_p[1 * RF_THREADS + tid + h]);
            rf_p[2 * RF_THREADS + tid] = rf_add(rf_p[2 * RF_THREADS + tid], rf_p[2 * RF_THREADS + tid + h]);
            rf_p[3 * RF_THREADS + tid] = rf_add(rf_p[3 * RF_THREADS + tid], rf_p[3 * RF_THREADS + tid + h]);
            rf_n[tid] += rf_n[tid + h];
            rf_n[RF_THREADS + tid] += rf_n[RF_THREADS + tid + h];
        }
        __syncthreads();
    }
    const float4 Z = make_float4(rf_p[0], rf_p[1 * RF_THREADS + 0], rf_p[2 * RF_THREADS + 0], rf_p[3 * RF_THREADS + 0]);
    count = rf_n[0];
    clipped = rf_n[RF_THREADS + 0];
    float4 zm = zero;
    if (count > 0) {
        const float fc = (float)count;
        zm = make_float4(rf_div(Z.x, fc), rf_div(Z.y, fc), rf_div(Z.z, fc), rf_div(Z.w, fc));
    }
    int code = 0;
    if (count < k.min_count)
        code = 1;
    else if (__builtin_fabsf(rf_add(Z.x, Z.y)) > rf_mul(k.t_broad, __builtin_sqrtf((float)count)))
        code = 2;
    if (tid == 0) *(int4*)st = make_int4(count, clipped, code, t.notkept[p]);
    for (int q = tid; q < nfine; q += RF_THREADS) {
        float4 w = zero;
        if (code == 0 && t.flag[base + q] == 0) {
            float4 y;
            if (rf_sample(x[q], t.c[base + q], t.m[base + q], t.g[base + q], k.t_clip, y))
                w = k.zerodm ? make_float4(rf_sub(y.x, zm.x), rf_sub(y.y, zm.y), rf_sub(y.z, zm.z), rf_sub(y.w, zm.w)) : y;
        }
        o[q] = w;
    }
}

}  // namespace xeng
