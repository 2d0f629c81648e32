// Workgroup-level scan, reductions and the ranked scatter of the marching translation units (march_train.hip: the offsets
// of the training marcher; render_loop.hip: live lists, frame minimum, survivor counts, stable compaction).  Device helpers only, no
// kernel; internal to the including unit.
#pragma once
#include "sdn_common.h"

namespace {

constexpr uint32_t kScanBlock = 1024;

// Block-level inclusive scan of one uint32 per thread (1024 threads = 16 waves): DPP-free,
// __shfl_up based wave scan + LDS carry.
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t *lds /*[16]*/, uint32_t &block_total) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v += u;
    }
    if (lane == 63) lds[wid] = v;
    __syncthreads();
    uint32_t carry = 0, total = 0;
    const uint32_t nw = blockDim.x >> 6;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t s = lds[w];
        if (w < wid) carry += s;
        total += s;
    }
    block_total = total;
    __syncthreads();
    return v + carry;
}

// The 256-thread reductions below hand their result to every thread and contain barriers; lds4 must not be in use.
__device__ __forceinline__ uint32_t block_min_256(uint32_t v, uint32_t *lds4) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(lds4[0], lds4[1]), min(lds4[2], lds4[3]));
}
// Number of threads of the 256-thread workgroup whose flag is set, in every thread.  Contains a barrier; lds4 must not be in use.
__device__ __forceinline__ uint32_t block_count_256(bool flag, uint32_t *lds4) {
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63u) == 0) lds4[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}
__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t *lds4) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // protects lds4 against the previous use
    if ((threadIdx.x & 63u) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

// Stable scatter of the entries v >= 0 of a workgroup of WAVES waves (one entry per thread, in thread order) to out[prev ...]: rank by
// wave ballot, per-wave counts through LDS.  Returns the workgroup's number of kept entries.  Contains barriers.
template <uint32_t WAVES>
__device__ __forceinline__ uint32_t ranked_scatter(int32_t v, uint32_t prev, int32_t *__restrict__ out, uint32_t *wave_counts /*[WAVES]*/) {
    const bool keep = v >= 0;
    const unsigned long long mask = __ballot(keep);
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t below = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();  // protects wave_counts against the previous use
    if (lane == 0) wave_counts[wid] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t carry = 0, total = 0;
    for (uint32_t w = 0; w < WAVES; w++) {
        const uint32_t c = wave_counts[w];
        if (w < wid) carry += c;
        total += c;
    }
    if (keep) out[prev + carry + below] = v;
    return total;
}

}  // namespace
