// Error-map importance sampling on the device (reference: nerf/utils.py:105-118 -- torch.multinomial on one row of the trainer's
// [frames, 128 * 128] error map, then a random pixel inside each drawn cell).
//
// torch.multinomial(w, N, replacement=False) draws q_i ~ Exp(1) and keeps the N largest w_i / q_i.  sdn_error_map_sample builds
// those keys and SELECTS the N largest in one launch of one workgroup -- nothing is sorted:
//   * 1024 threads, thread t owns the 16 consecutive cells 16 t .. 16 t + 15; their keys never leave its registers (a non-negative
//     float orders like its bit pattern, so a key is a uint32);
//   * a radix select finds the N-th largest key T exactly: four passes over 8 bits each, most significant first, every pass one LDS
//     histogram of the keys that still match the prefix found so far, one suffix scan over its 256 bins, one bin chosen.  After the
//     last pass `remaining` is the number of cells with key == T that belong to the draw;
//   * the draw is every cell with key > T plus the `remaining` lowest-indexed cells with key == T.  One prefix scan over the
//     per-thread counts gives every drawn cell its output slot: the results come out in ascending cell order, the same for every run.
// LDS: 8 copies of the histogram (a float's top bits put most keys of a pass into a handful of bins, and LDS atomics on one address
// serialise; thread t adds into copy t % 8, laid out so that one bin's copies sit on 8 banks) + the scans' wave totals, ~8.3 KiB.
#include "sdn_common.h"

namespace {

constexpr uint32_t kThreads = 1024, kPerThread = 16, kMaxCells = kThreads * kPerThread;   // 16 384 = the reference's 128 x 128
constexpr uint32_t kBins = 256, kCopies = 8, kCopyStride = kBins + 1;
static_assert(kMaxCells == 16384, "sdn_error_map_sample: S * S <= 16 384");

// Exclusive prefix sum of `v` over the workgroup's 1024 threads, in thread order; total = the sum over all of them.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *s_wave, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    #pragma unroll
    for (uint32_t w = 0; w < kThreads / 64; w++) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();       // (s_wave is reused by the next scan)
    total = all;
    return before + incl - v;
}

// uniform in the OPEN interval (0, 1): 23 random bits + 1/2, exact in fp32
__device__ __forceinline__ float u_open(uint64_t seed, uint32_t counter) {
    return ((float)(uint32_t)(sdn_splitmix64(seed, counter) >> 41) + 0.5f) * (1.0f / 8388608.0f);
}
// uniform in [0, 1) on torch.rand's 24-bit grid
__device__ __forceinline__ float u_half_open(uint64_t seed, uint32_t counter) {
    return (float)(uint32_t)(sdn_splitmix64(seed, counter) >> 40) * (1.0f / 16777216.0f);
}

__global__ void __launch_bounds__(kThreads) k_error_map_sample(const float *__restrict__ error_row, uint32_t S, uint32_t N, uint32_t H, uint32_t W,
                                                               const float *__restrict__ u_key, const float *__restrict__ u_fine, uint64_t seed,
                                                               int32_t *__restrict__ inds_coarse, int32_t *__restrict__ inds) {
    __shared__ uint32_t s_hist[kCopies * kCopyStride];
    __shared__ uint32_t s_wave[kThreads / 64];
    __shared__ uint32_t s_pick[2];                    // the chosen bin of a pass, and what is left to take inside it
    const uint32_t tid = threadIdx.x, cells = S * S, first = tid * kPerThread;

    // ---- keys: w / (-log u), 0 for a cell without weight; a positive weight whose key underflows still ranks above every zero ------
    uint32_t key[kPerThread];
    #pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t c = first + k;
        key[k] = 0u;
        if (c < cells) {
            const float w = error_row[c];
            const float u = u_key ? u_key[c] : u_open(seed, c);
            const float q = w > 0.0f ? w / (-logf(u)) : 0.0f;
            const uint32_t bits = __float_as_uint(q);
            key[k] = w > 0.0f ? (bits != 0u && bits <= 0x7F800000u ? bits : 1u) : 0u;
        }
    }

    // ---- radix select of the N-th largest key -------------------------------------------------------------------------------------------
    uint32_t prefix = 0, remaining = N;               // keys with (key >> (shift + 8)) == prefix are still in play
    #pragma unroll
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (uint32_t i = tid; i < kCopies * kCopyStride; i += kThreads) s_hist[i] = 0u;
        __syncthreads();
        #pragma unroll
        for (uint32_t k = 0; k < kPerThread; k++) {
            const bool in_play = first + k < cells && (shift == 24 || (key[k] >> (shift + 8)) == prefix);
            if (in_play) atomicAdd(&s_hist[(tid % kCopies) * kCopyStride + ((key[k] >> shift) & 255u)], 1u);
        }
        __syncthreads();
        // thread t < 256 stands for bin 255 - t: its exclusive prefix is the number of keys in the bins above
        uint32_t h = 0;
        if (tid < kBins)
            for (uint32_t cp = 0; cp < kCopies; cp++) h += s_hist[cp * kCopyStride + (kBins - 1u - tid)];
        uint32_t total;
        const uint32_t above = block_exclusive_scan(h, s_wave, total);
        if (tid < kBins && above < remaining && remaining <= above + h) {   // exactly one bin: the keys in play number >= remaining
            s_pick[0] = kBins - 1u - tid;
            s_pick[1] = remaining - above;
        }
        __syncthreads();
        prefix = (prefix << 8) | s_pick[0];
        remaining = s_pick[1];
        __syncthreads();   // (s_pick and s_hist are rewritten by the next pass)
    }
    const uint32_t T = prefix, ties_taken = remaining;

    // ---- output slots: cells above T and the first `ties_taken` cells at T, in cell order ----------------------------------------------
    uint32_t n_gt = 0, n_eq = 0;
    #pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const bool live = first + k < cells;
        n_gt += live && key[k] > T;
        n_eq += live && key[k] == T;
    }
    uint32_t total;
    const uint32_t packed = block_exclusive_scan(n_gt | (n_eq << 16), s_wave, total);     // (both counts <= 16 384: no carry between the halves)
    uint32_t gt_before = packed & 0xFFFFu, eq_before = packed >> 16;
    const float sx = (float)H / (float)S, sy = (float)W / (float)S;
    #pragma unroll
    for (uint32_t k = 0; k < kPerThread; k++) {
        const uint32_t c = first + k;
        if (c >= cells) continue;
        const bool gt = key[k] > T, eq = key[k] == T;
        if (gt || (eq && eq_before < ties_taken)) {
            const uint32_t slot = gt_before + (eq_before < ties_taken ? eq_before : ties_taken);
            if (slot < N) {
                const float r0 = u_fine ? u_fine[slot] : u_half_open(seed, kMaxCells + c);
                const float r1 = u_fine ? u_fine[N + slot] : u_half_open(seed, 2u * kMaxCells + c);
                // nerf/utils.py:108-112: (inds_x * sx + rand * sx).long().clamp(max = H - 1), the same for y
                long long x = (long long)((float)(c / S) * sx + r0 * sx), y = (long long)((float)(c % S) * sy + r1 * sy);
                x = x < (long long)H - 1 ? x : (long long)H - 1;
                y = y < (long long)W - 1 ? y : (long long)W - 1;
                inds_coarse[slot] = (int32_t)c;
                inds[slot] = (int32_t)(x * (long long)W + y);
            }
        }
        gt_before += gt;
        eq_before += eq;
    }
}

}  // namespace

extern "C" int sdn_error_map_sample(const float *error_row, uint32_t S, uint32_t N, uint32_t H, uint32_t W, const float *u_key, const float *u_fine,
                                    uint64_t seed, int32_t *inds_coarse, int32_t *inds, void *stream) {
    if (!error_row || !inds_coarse || !inds || S == 0 || S > 128 || N == 0 || N > S * S || H == 0 || W == 0 || (uint64_t)H * W > 0x7FFFFFFFull)
        return SDN_E_BADARG;
    hipLaunchKernelGGL(k_error_map_sample, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, error_row, S, N, H, W, u_key, u_fine, seed, inds_coarse, inds);
    return sdn_launch_status();
}
