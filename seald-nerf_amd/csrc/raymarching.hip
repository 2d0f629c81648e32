// Drop-in ray utilities and the cull-grid build for gfx950 (MI355X).
//
// Holds the reference's stand-alone utilities (near_far_from_aabb, sph_from_ray, morton3D, morton3D_invert, packbits:
// raymarching/src/raymarching.cu:92-289, line ranges cited per kernel) and the kernels that build, initialise and copy the cull grid
// the marchers read (sdn_int::build_cull, build_cull_group, copy_cull; layout and exactness argument: march_core.h).
// The training marcher and compositors are in march_train.hip, the inference marcher, compositor, compaction and the device-driven
// loop in render_loop.hip; the three units share the device code of march_core.h and are built with the same flags
// (-ffp-contract=off: every float operation rounds on its own, in the order the reference source writes it, which is what
// oracle/sdn_oracle.c evaluates on the CPU).
#include "march_core.h"

namespace {

constexpr float kRPi = 0.3183098861837907f;

__device__ __forceinline__ const uint8_t *frame_grid_uniform_y(const sdn_int::FrameSel &fs) { return fs.grid[blockIdx.y]; }

__global__ void __launch_bounds__(256) k_build_cull_grid(const uint8_t *__restrict__ bitfield, uint32_t *__restrict__ cull_bits,
                                                         sdn_int::FrameSel fs) {
    if (fs.n_frames > 1) {   // frame group: blockIdx.y = frame
        bitfield = frame_grid_uniform_y(fs);
        cull_bits += (size_t)blockIdx.y * fs.cull_stride;
    }
    const uint32_t c = threadIdx.x + blockIdx.x * blockDim.x;  // grid.x is exactly 32^3 threads
    const int cx = c & 31, cy = (c >> 5) & 31, cz = c >> 10;
    const unsigned long long *__restrict__ blocks = reinterpret_cast<const unsigned long long *>(bitfield);
    bool any = false;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int x = cx + dx, y = cy + dy, z = cz + dz;
                if (x < 0 || y < 0 || z < 0 || x > 31 || y > 31 || z > 31) continue;
                // a 4x4x4 block of the 128^3 grid is 64 consecutive Morton bits = one aligned 8-byte word
                any |= blocks[morton3D_((uint32_t)x, (uint32_t)y, (uint32_t)z)] != 0ull;
            }
    const unsigned long long m = __ballot(any);  // lane i <-> cell c0 + i
    if ((threadIdx.x & 63u) == 0) {
        cull_bits[c >> 5] = (uint32_t)m;
        cull_bits[(c >> 5) + 1] = (uint32_t)(m >> 32);
    }
    if (any) {
        int *meta = reinterpret_cast<int *>(cull_bits + kCullWords);
        atomicMin(meta + 0, cx); atomicMin(meta + 1, cy); atomicMin(meta + 2, cz);
        atomicMax(meta + 3, cx); atomicMax(meta + 4, cy); atomicMax(meta + 5, cz);
    }
}

__global__ void k_cull_meta_init(uint32_t *__restrict__ cull_bits, uint32_t n_frames, uint32_t cull_stride) {
    if (threadIdx.x < n_frames && blockIdx.x == 0) {
        int *meta = reinterpret_cast<int *>(cull_bits + (size_t)threadIdx.x * cull_stride + kCullWords);
        meta[0] = meta[1] = meta[2] = (int)kCullRes;
        meta[3] = meta[4] = meta[5] = -1;
        meta[6] = meta[7] = 0;
    }
}

__global__ void __launch_bounds__(256) k_build_fine_image(const uint8_t *__restrict__ bitfield, uint32_t *__restrict__ cull_bits, sdn_int::FrameSel fs) {
    if (fs.n_frames > 1) {   // frame group: blockIdx.y = frame
        bitfield = frame_grid_uniform_y(fs);
        cull_bits += (size_t)blockIdx.y * fs.cull_stride;
    }
    int *meta = reinterpret_cast<int *>(cull_bits + kCullWords);
    const int fx0 = meta[0], fy0 = meta[1], fz0 = meta[2];
    const int fnx = meta[3] - fx0 + 1, fny = meta[4] - fy0 + 1, fnz = meta[5] - fz0 + 1;
    const bool fits = fnx > 0 && fny > 0 && fnz > 0 && (uint32_t)(fnx * fny * fnz) <= kFineCacheCells;
    const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i == 0) meta[6] = fits ? 1 : 0;
    if (!fits || i >= (uint32_t)(fnx * fny * fnz)) return;
    const unsigned long long *__restrict__ blocks = reinterpret_cast<const unsigned long long *>(bitfield);
    unsigned long long *img = reinterpret_cast<unsigned long long *>(cull_bits + kCullImageWord);
    const int cx = fx0 + (int)i % fnx, cy = fy0 + ((int)i / fnx) % fny, cz = fz0 + (int)i / (fnx * fny);
    img[i] = blocks[morton3D_8bit((uint32_t)cx, (uint32_t)cy, (uint32_t)cz)];
}

// ---------------------------------------------------------------------------
// utils
// ---------------------------------------------------------------------------
// raymarching.cu:92-145
__global__ void __launch_bounds__(256) k_near_far_from_aabb(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                            const float *__restrict__ aabb, uint32_t N, float min_near,
                                                            float *__restrict__ nears, float *__restrict__ fars) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const float ox = rays_o[n * 3], oy = rays_o[n * 3 + 1], oz = rays_o[n * 3 + 2];
    const float rdx = 1 / rays_d[n * 3], rdy = 1 / rays_d[n * 3 + 1], rdz = 1 / rays_d[n * 3 + 2];
    const float mx = __FLT_MAX__;
    float near = (aabb[0] - ox) * rdx, far = (aabb[3] - ox) * rdx;
    if (near > far) { float c = near; near = far; far = c; }
    float near_y = (aabb[1] - oy) * rdy, far_y = (aabb[4] - oy) * rdy;
    if (near_y > far_y) { float c = near_y; near_y = far_y; far_y = c; }
    if (near > far_y || near_y > far) { nears[n] = mx; fars[n] = mx; return; }
    if (near_y > near) near = near_y;
    if (far_y < far) far = far_y;
    float near_z = (aabb[2] - oz) * rdz, far_z = (aabb[5] - oz) * rdz;
    if (near_z > far_z) { float c = near_z; near_z = far_z; far_z = c; }
    if (near > far_z || near_z > far) { nears[n] = mx; fars[n] = mx; return; }
    if (near_z > near) near = near_z;
    if (far_z < far) far = far_z;
    if (near < min_near) near = min_near;
    nears[n] = near;
    fars[n] = far;
}

// raymarching.cu:163-198
__global__ void __launch_bounds__(256) k_sph_from_ray(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                      float radius, uint32_t N, float *__restrict__ coords) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const float ox = rays_o[n * 3], oy = rays_o[n * 3 + 1], oz = rays_o[n * 3 + 2];
    const float dx = rays_d[n * 3], dy = rays_d[n * 3 + 1], dz = rays_d[n * 3 + 2];
    const float A = dx * dx + dy * dy + dz * dz;
    const float B = ox * dx + oy * dy + oz * dz;
    const float C = ox * ox + oy * oy + oz * oz - radius * radius;
    const float t = (-B + sqrtf(B * B - A * C)) / A;
    const float x = ox + t * dx, y = oy + t * dy, z = oz + t * dz;
    const float theta = atan2f(sqrtf(x * x + z * z), y);
    const float phi = atan2f(z, x);
    coords[n * 2] = 2 * theta * kRPi - 1;
    coords[n * 2 + 1] = phi * kRPi;
}

// raymarching.cu:214-254
__global__ void __launch_bounds__(256) k_morton3D(const int32_t *__restrict__ coords, uint32_t N, int32_t *__restrict__ indices) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    indices[n] = (int32_t)morton3D_((uint32_t)coords[n * 3], (uint32_t)coords[n * 3 + 1], (uint32_t)coords[n * 3 + 2]);
}
__global__ void __launch_bounds__(256) k_morton3D_invert(const int32_t *__restrict__ indices, uint32_t N, int32_t *__restrict__ coords) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const int ind = indices[n];
    coords[n * 3] = (int32_t)morton3D_invert_((uint32_t)(ind >> 0));
    coords[n * 3 + 1] = (int32_t)morton3D_invert_((uint32_t)(ind >> 1));
    coords[n * 3 + 2] = (int32_t)morton3D_invert_((uint32_t)(ind >> 2));
}

// raymarching.cu:268-289.  One lane per output byte; the 8 floats are fetched as two float4
// (32 B per lane, 2 KiB per wave-instruction pair: fully coalesced).
__global__ void __launch_bounds__(256) k_packbits(const float4 *__restrict__ grid, uint32_t N, float thresh, uint8_t *__restrict__ bitfield) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
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

}  // namespace

namespace sdn_int {

// with_image: the buffer has sdn_cull_grid_bytes() behind it (marks + meta + packed fine bits); false: marks + meta only
int build_cull(const uint8_t *bitfield, uint32_t *cull_bits, hipStream_t st, bool with_image) {
    hipLaunchKernelGGL(k_cull_meta_init, dim3(1), dim3(64), 0, st, cull_bits, 1u, 0u);
    hipLaunchKernelGGL(k_build_cull_grid, dim3(kCullRes * kCullRes * kCullRes / 256), dim3(256), 0, st, bitfield, cull_bits, FrameSel());
    if (with_image) hipLaunchKernelGGL(k_build_fine_image, dim3(kFineCacheCells / 256), dim3(256), 0, st, bitfield, cull_bits, FrameSel());
    return sdn_launch_status();
}

// cull grids the caller kept per occupancy slice -> the context's contiguous copy (one launch, 4 KiB per frame)
struct CullCopy { const uint32_t *src[SDN_MAX_GROUP_FRAMES]; };
__global__ void __launch_bounds__(256) k_copy_cull_grids(CullCopy srcs, uint32_t *__restrict__ dst, uint32_t words, uint32_t stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) dst[(size_t)blockIdx.y * stride + i] = srcs.src[blockIdx.y][i];
}

int copy_cull(const void *const *prebuilt, uint32_t n_frames, uint32_t *cull_bits, hipStream_t st) {
    CullCopy c{};
    for (uint32_t f = 0; f < n_frames && f < (uint32_t)SDN_MAX_GROUP_FRAMES; f++) c.src[f] = (const uint32_t *)prebuilt[f];
    const uint32_t words = sdn_cull_grid_bytes() / 4u;
    hipLaunchKernelGGL(k_copy_cull_grids, dim3(sdn_div_up(words, 256u), n_frames), dim3(256), 0, st, c, cull_bits, words, n_frames > 1 ? words : 0u);
    return sdn_launch_status();
}

int build_cull_group(const FrameSel &fs, uint32_t *cull_bits, hipStream_t st) {
    hipLaunchKernelGGL(k_cull_meta_init, dim3(1), dim3(64), 0, st, cull_bits, fs.n_frames, fs.cull_stride);
    hipLaunchKernelGGL(k_build_cull_grid, dim3(kCullRes * kCullRes * kCullRes / 256, fs.n_frames), dim3(256), 0, st, (const uint8_t *)nullptr,
                       cull_bits, fs);
    hipLaunchKernelGGL(k_build_fine_image, dim3(kFineCacheCells / 256, fs.n_frames), dim3(256), 0, st, (const uint8_t *)nullptr, cull_bits, fs);
    return sdn_launch_status();
}

}  // namespace sdn_int

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int sdn_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N, float min_near,
                           float *nears, float *fars, void *stream) {
    if (N == 0) return 0;
    if (!rays_o || !rays_d || !aabb || !nears || !fars) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_near_far_from_aabb, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, aabb, N,
                       min_near, nears, fars);
    return sdn_launch_status();
}

int sdn_sph_from_ray(const float *rays_o, const float *rays_d, float radius, uint32_t N, float *coords, void *stream) {
    if (N == 0) return 0;
    if (!rays_o || !rays_d || !coords) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_sph_from_ray, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, radius, N, coords);
    return sdn_launch_status();
}

int sdn_morton3D(const int32_t *coords, uint32_t N, int32_t *indices, void *stream) {
    if (N == 0) return 0;
    if (!coords || !indices) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_morton3D, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, coords, N, indices);
    return sdn_launch_status();
}

int sdn_morton3D_invert(const int32_t *indices, uint32_t N, int32_t *coords, void *stream) {
    if (N == 0) return 0;
    if (!coords || !indices) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_morton3D_invert, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, indices, N, coords);
    return sdn_launch_status();
}

int sdn_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield, void *stream) {
    if (N == 0) return 0;
    if (!grid || !bitfield) return SDN_E_BADARG;
    if (((uintptr_t)grid & 15u) != 0) return SDN_E_BADARG;  // float4 loads
    hipLaunchKernelGGL(k_packbits, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, (const float4 *)grid, N, density_thresh,
                       bitfield);
    return sdn_launch_status();
}

uint32_t sdn_cull_grid_bytes(void) { return kCullImageWord * 4 + kFineCacheCells * 8; }  // marks + bounding-box record + packed fine bits

int sdn_build_cull_grid(const uint8_t *bitfield, uint32_t H, uint8_t *cull_grid, void *stream) {
    if (!bitfield || !cull_grid) return SDN_E_BADARG;
    if (H != 128) return SDN_E_UNSUPPORTED;
    if (((uintptr_t)bitfield & 7u) != 0 || ((uintptr_t)cull_grid & 15u) != 0) return SDN_E_BADARG;
    return sdn_int::build_cull(bitfield, (uint32_t *)cull_grid, (hipStream_t)stream);
}

}  // extern "C"
