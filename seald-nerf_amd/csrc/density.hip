// Density-grid maintenance on the device (reference: NeRFRenderer.update_extra_state, dnerf/renderer.py:453-555).
//
// The reference evaluates the density network on every cell of every time slice (64 x 128^3 = 134 M points on the first 16
// calls, half of that afterwards) through the op-by-op network, fills a full-size tmp_grid, applies the EMA / maximum update with
// boolean-mask indexing, takes the mean with a host read-back and packs the bitfield slice by slice.  Here:
//   * sdn_density_query_cells_f16: one launch of the fused field kernel (CELLS variant, field.hip) per time slice -- the cell
//     centres are built and jittered in the kernel, nothing but sigma * density_scale is written;
//   * sdn_density_grid_ema: density = max(density * decay, tmp) where both are >= 0, plus the running sum of clamp(density, 0)
//     for the mean (fp64 accumulator on the device);
//   * sdn_density_grid_pack: threshold = min(mean, density_thresh) taken on the device, bitfield for all slices in one pass.
// No host synchronisation anywhere; one time slice of tmp_grid (8 MiB) is live at a time instead of 512 MiB.
//
// Before the first update the trainer marks the cells no training camera sees (NeRFRenderer.mark_untrained_grid, dnerf/renderer.py:
// 389-451) with -1, which the EMA above then never touches:
//   * sdn_mark_untrained_grid: one lane per cell tests the cell's centre against every camera's frustum and writes -1 to the cell in
//     every time slice if none sees it.  The reference builds an [S, 64^3, 3] tensor per pose batch and a full-size boolean mask.
#include "sdn_common.h"
#include "sdn_internal.h"
#include "cell_points.h"

namespace {

constexpr int kEmaBlock = 256;

constexpr int kEmaPerThread = 8;   // float4s per thread: few, fat workgroups -- the fp64 atomics on one address serialise (2048 of them cost ~20 us)

// dnerf/renderer.py:536-538.  Block partial sums reduced in fp64, one atomic per block.
__global__ void __launch_bounds__(kEmaBlock) k_density_ema(float4 *__restrict__ grid, const float4 *__restrict__ tmp, uint32_t n4, float decay,
                                                           double *__restrict__ sum) {
    double v = 0.0;
    #pragma unroll
    for (int k = 0; k < kEmaPerThread; k++) {
        const uint32_t i = threadIdx.x + (blockIdx.x * kEmaPerThread + k) * kEmaBlock;
        if (i < n4) {
            float4 g = grid[i];
            const float4 t = tmp[i];
            // valid = (grid >= 0) & (tmp >= 0) -- false for NaN on either side, as in the reference's mask
            if (g.x >= 0 && t.x >= 0) g.x = fmaxf(g.x * decay, t.x);
            if (g.y >= 0 && t.y >= 0) g.y = fmaxf(g.y * decay, t.y);
            if (g.z >= 0 && t.z >= 0) g.z = fmaxf(g.z * decay, t.z);
            if (g.w >= 0 && t.w >= 0) g.w = fmaxf(g.w * decay, t.w);
            grid[i] = g;
            v += (double)((fmaxf(g.x, 0.0f) + fmaxf(g.y, 0.0f)) + (fmaxf(g.z, 0.0f) + fmaxf(g.w, 0.0f)));
        }
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __shared__ double s_part[kEmaBlock / 64];
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double b = 0;
        #pragma unroll
        for (int w = 0; w < kEmaBlock / 64; w++) b += s_part[w];
        atomicAdd(sum, b);
    }
}

// dnerf/renderer.py:539-545 + raymarching.cu:268-289: mean -> threshold -> one byte per 8 cells (bit i%8 of byte i/8)
__global__ void __launch_bounds__(256) k_density_pack(const float4 *__restrict__ grid, uint32_t n8, const double *__restrict__ sum,
                                                      double cells, float density_thresh, float *__restrict__ mean_out,
                                                      uint8_t *__restrict__ bitfield) {
    const float mean = (float)(*sum / cells);
    const float thresh = fminf(mean, density_thresh);
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n == 0 && mean_out) {
        mean_out[0] = mean;
        mean_out[1] = thresh;
    }
    if (n >= n8) return;
    const float4 a = grid[(size_t)n * 2], b = grid[(size_t)n * 2 + 1];
    uint32_t bits = 0;
    bits |= (a.x > thresh) ? 1u : 0u;
    bits |= (a.y > thresh) ? 2u : 0u;
    bits |= (a.z > thresh) ? 4u : 0u;
    bits |= (a.w > thresh) ? 8u : 0u;
    bits |= (b.x > thresh) ? 16u : 0u;
    bits |= (b.y > thresh) ? 32u : 0u;
    bits |= (b.z > thresh) ? 64u : 0u;
    bits |= (b.w > thresh) ? 128u : 0u;
    bitfield[n] = (uint8_t)bits;
}

constexpr int kMarkBlock = 256;
constexpr int kPoseChunk = SDN_MARK_POSE_CHUNK;   // poses staged in LDS at a time: 3 float4 each (rows of [R | t]), 12 KiB

// dnerf/renderer.py:403-449.  Lane i of a workgroup row owns Morton cell i of cascade blockIdx.y, so a wave's 64 cells are 256
// contiguous bytes of every time slice.  Every lane of the workgroup reads the same pose at the same time (an LDS broadcast); a lane
// whose cell has been seen skips the tests but stays in the chunk loop: the barriers sit in control flow that is uniform per workgroup.
__global__ void __launch_bounds__(kMarkBlock) k_mark_untrained(float *__restrict__ grid, uint32_t T, uint32_t H, float bound,
                                                               const float *__restrict__ poses, uint32_t B, float tan_x, float tan_y,
                                                               uint32_t *__restrict__ marked) {
    __shared__ float4 s_pose[kPoseChunk * 3];
    const uint32_t H3 = H * H * H, cas = blockIdx.y;
    const uint32_t cell = blockIdx.x * kMarkBlock + threadIdx.x;
    // :424-427  bound = min(2 ** cas, self.bound); the cell's centre, un-jittered (r = 0.5)
    const float cas_bound = fminf((float)(1u << (cas < 31u ? cas : 31u)), bound);
    const float half = cas_bound / (float)H, span = cas_bound - half, inv = 1.0f / (float)(H - 1u), pad = half * 2.0f;
    const float px = sdn_cells::cell_coord(cell, 0, 0.5f, inv, span, half), py = sdn_cells::cell_coord(cell, 1, 0.5f, inv, span, half),
                pz = sdn_cells::cell_coord(cell, 2, 0.5f, inv, span, half);
    bool seen = cell >= H3;       // lanes past the grid (H^3 < 256) have nothing to test or write
    for (uint32_t base = 0; base < B; base += kPoseChunk) {
        const uint32_t n = min((uint32_t)kPoseChunk, B - base);
        for (uint32_t k = threadIdx.x; k < n * 12u; k += kMarkBlock)
            reinterpret_cast<float *>(s_pose)[k] = poses[(size_t)(base + k / 12u) * 16u + k % 12u];
        __syncthreads();
        for (uint32_t b = 0; b < n && !seen; b++) {
            const float4 r0 = s_pose[b * 3], r1 = s_pose[b * 3 + 1], r2 = s_pose[b * 3 + 2];
            // :435-441  cam = (p - pose[:3, 3]) @ pose[:3, :3]
            const float dx = px - r0.w, dy = py - r1.w, dz = pz - r2.w;
            const float cx = dx * r0.x + dy * r1.x + dz * r2.x;
            const float cy = dx * r0.y + dy * r1.y + dz * r2.y;
            const float cz = dx * r0.z + dy * r1.z + dz * r2.z;
            seen = cz > 0.0f && fabsf(cx) < tan_x * cz + pad && fabsf(cy) < tan_y * cz + pad;
        }
        __syncthreads();          // everyone is done with this chunk before the next one overwrites it
    }
    const bool unseen = !seen;
    // :449  density_grid[count == 0, in every time slice] = -1
    if (unseen) {
        float *p = grid + (size_t)cas * H3 + cell;
        const size_t slice = (size_t)gridDim.y * H3;
        for (uint32_t t = 0; t < T; t++, p += slice) *p = -1.0f;
    }
    if (marked) {
        const uint32_t n_wave = (uint32_t)__popcll(__ballot(unseen));
        if ((threadIdx.x & (SDN_WAVE - 1)) == 0 && n_wave) atomicAdd(marked + cas, n_wave);
    }
}

}  // namespace

extern "C" {

int sdn_density_query_cells_f16(const int32_t *cells, const uint32_t *cell_count, uint32_t n, const float *noise, uint32_t seed,
                                uint32_t grid_size, float cas_bound, const void *weights, const float *bias0, const void *table,
                                const int32_t *offsets_host, float S, uint32_t H, float bound, float density_scale, int zero_deform,
                                float *tmp_slice, void *stream) {
    return sdn_int::field_cells_checked(0, {.f = {.live_idx = (const uint32_t *)cells, .live_count = cell_count, .M = n, .weights = weights, .bias0 = bias0,
                                                  .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                                  .density_scale = density_scale, .zero_deform = zero_deform ? 1 : 0, .sigmas = tmp_slice},
                                            .noise = noise, .seed = seed, .grid_size = grid_size, .cas_bound = cas_bound},
                                        stream);
}

int sdn_density_grid_ema(float *density_grid, const float *tmp_grid, uint64_t n, float decay, double *sum, void *stream) {
    if (n == 0) return 0;
    if (!density_grid || !tmp_grid || !sum) return SDN_E_BADARG;
    if ((n & 3u) != 0 || (n >> 2) > 0xFFFFFFFFull || (((uintptr_t)density_grid | (uintptr_t)tmp_grid) & 15u) != 0) return SDN_E_BADARG;
    const uint32_t n4 = (uint32_t)(n >> 2);
    hipLaunchKernelGGL(k_density_ema, dim3(sdn_div_up(n4, (uint32_t)(kEmaBlock * kEmaPerThread))), dim3(kEmaBlock), 0, (hipStream_t)stream, (float4 *)density_grid,
                       (const float4 *)tmp_grid, n4, decay, sum);
    return sdn_launch_status();
}

int sdn_density_grid_pack(const float *density_grid, uint64_t n, const double *sum, float density_thresh, float *mean_out,
                          uint8_t *bitfield, void *stream) {
    if (n == 0) return 0;
    if (!density_grid || !sum || !bitfield) return SDN_E_BADARG;
    if ((n & 7u) != 0 || (n >> 3) > 0xFFFFFFFFull || ((uintptr_t)density_grid & 15u) != 0) return SDN_E_BADARG;
    const uint32_t n8 = (uint32_t)(n >> 3);
    hipLaunchKernelGGL(k_density_pack, dim3(sdn_div_up(n8, 256u)), dim3(256), 0, (hipStream_t)stream, (const float4 *)density_grid, n8, sum,
                       (double)n, density_thresh, mean_out, bitfield);
    return sdn_launch_status();
}

int sdn_mark_untrained_grid(float *density_grid, uint32_t T, uint32_t cascade, uint32_t H, float bound, const float *poses, uint32_t B,
                            float fx, float fy, float cx, float cy, uint32_t *marked, void *stream) {
    if (!density_grid || !poses || B == 0 || H == 0 || (H & (H - 1u)) != 0 || fx == 0.0f || fy == 0.0f) return SDN_E_BADARG;
    if (H > 1024u || cascade > 65535u) return SDN_E_UNSUPPORTED;      // morton3D spreads 10 bits per axis; cascades are gridDim.y
    if (cascade == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    if (marked && hipMemsetAsync(marked, 0, cascade * sizeof(uint32_t), st) != hipSuccess) return sdn_launch_status();
    // :440-441  cx / fx and cy / fy are Python (fp64) quotients that meet the fp32 tensor as fp32 scalars
    hipLaunchKernelGGL(k_mark_untrained, dim3(sdn_div_up(H * H * H, (uint32_t)kMarkBlock), cascade), dim3(kMarkBlock), 0, st, density_grid, T, H,
                       bound, poses, B, (float)((double)cx / (double)fx), (float)((double)cy / (double)fy), marked);
    return sdn_launch_status();
}

}  // extern "C"
