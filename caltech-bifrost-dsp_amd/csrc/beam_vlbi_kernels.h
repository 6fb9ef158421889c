// Device side of xengBeamformPacketizeVoltages: the voltage beams of one Beamform gulp -> "ibeam" packets
// (beamform_vlbi_output_block.py:258-276, which does the same selection and transposition with numpy on the host).
//
//   in   cf32[nchan][nbeam][ntime]                       rows r = (c, b), b in [beam0, beam0+nbeam_pkt): R = nchan*nbeam_pkt rows
//   out  slot t at out + t*pkt_stride:  byte 0 untouched, [1,16) header, [16, 16+8R) payload cf32[nchan][nbeam_pkt] at sample t
//
// A corner turn, bits copied as they are (integer loads and stores only: NaN payloads, -0.0 and denormals arrive unchanged).
// One 256-thread workgroup per tile of 32 rows x 32 samples, through 8 KiB of LDS:
//   read   16 lanes per row, 16 B (two samples) each: 256 contiguous bytes of one input row;
//   write  16 B (two rows) per lane, 8 lanes per 128 contiguous bytes of one packet's payload (one sample: 16 lanes, 256 B).
// LDS tile [32 rows][16 slots of 16 B], slot s of row j stored at s ^ ((j >> 1) & 15) (unswizzled, the 256-B rows put the
// rows of one sample on one bank: 16-way):
//   ds_write_b128 of a row (8 contiguous lanes = 8 slots of one row, banks mod 32): 8 distinct slots mod 8 -> conflict-free;
//   rows 2p and 2p+1 at sample t, which the compiler reads with one ds_read2_b64 (16 contiguous lanes, banks mod 32; as two
//   ds_read_b64, 32 lanes, banks mod 64): a 16-lane group holds 8 row pairs x 2 samples (the lane order of the write loop),
//   row pair p lands in slot (t/2) ^ p, 8 distinct slots mod 8 x 2 halves = 32 banks -> conflict-free either way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

constexpr int VLBI_ROWS = 32, VLBI_TIMES = 32, VLBI_HDR = 16;

// header bytes [1,16) of a slot: u8 server, gbe, nchan, nbeam, nserver; u16 chan0 big-endian; u64 seq big-endian
struct VlbiHeader {
    uint8_t server, gbe, nchan, nbeam, nserver;
    uint16_t chan0;
    uint64_t seq0;
};

__device__ __forceinline__ int vlbi_lds_index(int j, int t) {     // uint2 index of (row j, sample t) in the swizzled tile
    return j * VLBI_TIMES + ((((t >> 1) ^ (j >> 1)) & 15) << 1) + (t & 1);
}

// VEC_IN: every input row 16-B aligned (in 16-B aligned, ntime even) -> dwordx4 reads; otherwise dwordx2 reads
template <bool VEC_IN>
__global__ __launch_bounds__(256) void beam_vlbi_packetize_kernel(const uint2* __restrict__ in, uint8_t* __restrict__ out,
                                                                  int nbeam, int ntime, int beam0, int nbeam_pkt, int nrow,
                                                                  size_t pkt_stride, VlbiHeader h) {
    __shared__ __attribute__((aligned(16))) uint2 tile[VLBI_ROWS * VLBI_TIMES];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * VLBI_ROWS, t0 = blockIdx.y * VLBI_TIMES;
    if (VEC_IN) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int q = tid + 256 * k, j = q >> 4, s = q & 15;
            const int r = r0 + j, t = t0 + 2 * s;
            if (r < nrow && t < ntime) {                    // (ntime even: t + 1 < ntime as well)
                const int c = r / nbeam_pkt, b = beam0 + r % nbeam_pkt;
                const uint4 v = *reinterpret_cast<const uint4*>(in + ((size_t)c * nbeam + b) * ntime + t);
                *reinterpret_cast<uint4*>(&tile[vlbi_lds_index(j, 2 * s)]) = v;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = tid + 256 * k, j = q >> 5, tl = q & 31;
            const int r = r0 + j, t = t0 + tl;
            if (r < nrow && t < ntime) {
                const int c = r / nbeam_pkt, b = beam0 + r % nbeam_pkt;
                tile[vlbi_lds_index(j, tl)] = in[((size_t)c * nbeam + b) * ntime + t];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; k++) {
        // lane bits: [0,3) row pair p low, 3 sample t low, 4 row pair p high, [5,..) sample t high
        const int q = tid + 256 * k, p = (q & 7) | ((q >> 1) & 8), tl = ((q >> 3) & 1) | ((q >> 5) << 1);
        const int t = t0 + tl, r = r0 + 2 * p;
        if (r + 1 < nrow && t < ntime) {
            // (16-B aligned: out and pkt_stride are, and r is even -- told to the compiler, which would split the store otherwise)
            uint4* dst = static_cast<uint4*>(__builtin_assume_aligned(out + (size_t)t * pkt_stride + VLBI_HDR + (size_t)r * 8, 16));
            const uint2 a = tile[vlbi_lds_index(2 * p, tl)], b = tile[vlbi_lds_index(2 * p + 1, tl)];
            *dst = make_uint4(a.x, a.y, b.x, b.y);
        }
    }
    // an odd row count: the payload's last 8 bytes, one lane per sample (kept apart from the loop above: an 8-byte store in a
    // branch of it lets the compiler merge the two branches' tails into dwordx3 + dword for every pair)
    if ((nrow & 1) && r0 + VLBI_ROWS >= nrow && tid < VLBI_TIMES && t0 + tid < ntime) {
        const int j = nrow - 1 - r0;
        *reinterpret_cast<uint2*>(out + (size_t)(t0 + tid) * pkt_stride + VLBI_HDR + (size_t)(nrow - 1) * 8) = tile[vlbi_lds_index(j, tid)];
    }
    if (blockIdx.x == 0 && tid < VLBI_TIMES && t0 + tid < ntime) {       // the headers of this tile's samples
        const int t = t0 + tid;
        uint8_t* p = out + (size_t)t * pkt_stride;
        p[1] = h.server;
        *reinterpret_cast<uint16_t*>(p + 2) = (uint16_t)(h.gbe | (h.nchan << 8));
        *reinterpret_cast<uint32_t*>(p + 4) =
            (uint32_t)h.nbeam | ((uint32_t)h.nserver << 8) | ((uint32_t)(h.chan0 >> 8) << 16) | ((uint32_t)(h.chan0 & 0xFF) << 24);
        *reinterpret_cast<uint64_t*>(p + 8) = __builtin_bswap64(h.seq0 + (uint64_t)t);
    }
}

}  // namespace xeng
