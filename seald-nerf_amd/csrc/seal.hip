// SealD-NeRF bounding-box, anchor (control-point) and brush seal mappers on the sample stream (scope row "next" #1) for gfx950.
//
// Behavioural contract: SealNeRF/seal_utils.py of the reference --
//   map_mask            :132-153  (points.all(1) & strict AABB test of each bound, then points_in_mesh)
//   points_in_mesh      :675-693  (inside iff the ray along trimesh's test direction AND the opposite ray hit the mesh)
//   moller_trumbore     :638-672  (t, u, v exactly as written there, eps = 1e-8, t >= 0, u >= 0, v >= 0, u + v <= 1)
//   SealBBoxMapper.map_to_origin :245-286 (inverse transform, inverse scale about the source centre, inverse rotation of dirs)
//   modify_hsv :747-758 with color_utils.py:31-63 (rgb -> hsv, + modification, -> rgb)
//   modify_rgb :761-777 (hue / saturation of a target colour, brightness = its V + (V - mean V of the masked samples) + light offset)
//   the `mapSource` redirect of SealBBoxMapper.map_to_origin :269-273 (samples strictly inside the source box are sent to one point --
//   only in calls that map at least one sample: the early return of :251-252 comes first)
//   SealAnchorMapper.map_to_origin :522-578 with project_points :736-744 (the cone / plane-side deformation, see k_seal_anchor_apply)
//   SealBrushMapper.map_to_origin :415-461 (the surface pushed along the stroke's normal, attenuated towards the stroke's border, see k_seal_brush_map)
//   the `image` branch of map_color :58-79 (the brush's `imageConfig` texture stamp: a texel per sample is modify_rgb's target, alpha-blended, see SealStamp)
// The mappers and colour edits share their steps: seal_in_aabb / seal_in_bounds, project_point, rgb_to_hsv / hsv_to_rgb, seal_mean_v, the
// second colour pass k_seal_apply<per iteration?, SealTint | SealStamp>; on the host fill_bounds, launch_lanes, seal_recolour[_whole_rays].
// The reference evaluates this with boolean-mask gathers / scatters and O(points x triangles) temporaries in torch, inside the
// render loop; here it is one lane per sample slot, in place, between the marcher and the field kernel.  Dot products are
// accumulated x, y, z in fp32 (torch's einsum order is library-defined): masks agree with the torch restatement except for
// points within rounding of a face, mapped coordinates to ~1e-6 -- the tolerances its tests state.
#include "sdn_common.h"

#include <atomic>

namespace {

struct SealBoxTest {        // map_mask's inputs
    float bounds[4][6];     // up to 4 AABBs {lo xyz, hi xyz}
    uint32_t n_bounds;
    const float *tris;      // [F][12]: v0, E1, E2, N (host-precomputed from the box triangles)
    uint32_t n_tris;
    float test_dir[3];
};

struct SealBoxArgs {
    SealBoxTest box;
    float tinv[12];         // inverse transform, rows of [3 x 4]
    float rinv[9];          // inverse rotation
    float scale[3], center[3];
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

// project_points(n, o, p), seal_utils.py:736-744: q = p - ((p - o) . n / n . n) n; n_sq: n . n, as the caller holds it
__device__ __forceinline__ void project_point(float nx, float ny, float nz, float n_sq, float ox, float oy, float oz, float px, float py, float pz,
                                              float &qx, float &qy, float &qz) {
    const float along = dot3(px - ox, py - oy, pz - oz, nx, ny, nz) / n_sq;
    qx = px - along * nx; qy = py - along * ny; qz = pz - along * nz;
}

__device__ __forceinline__ bool any_hit(const float *__restrict__ tris, uint32_t F, float ox, float oy, float oz, float dx, float dy, float dz) {
    bool hit = false;
    for (uint32_t f = 0; f < F; f++) {
        const float *t = tris + 12 * f;
        const float a0x = ox - t[0], a0y = oy - t[1], a0z = oz - t[2];
        const float invdet = 1.0f / -(dot3(dx, dy, dz, t[9], t[10], t[11]) + 1e-8f);
        const float cx = a0y * dz - a0z * dy, cy = a0z * dx - a0x * dz, cz = a0x * dy - a0y * dx;   // A0 x d
        const float u = dot3(cx, cy, cz, t[6], t[7], t[8]) * invdet;
        const float v = -dot3(cx, cy, cz, t[3], t[4], t[5]) * invdet;
        const float tt = dot3(a0x, a0y, a0z, t[9], t[10], t[11]) * invdet;
        hit |= (tt >= 0.0f) & (u >= 0.0f) & (v >= 0.0f) & ((u + v) <= 1.0f);
    }
    return hit;
}

// strictly inside the box lo .. hi
__device__ __forceinline__ bool seal_in_aabb(const float *lo, const float *hi, float x, float y, float z) {
    return (hi[0] > x) & (x > lo[0]) & (hi[1] > y) & (y > lo[1]) & (hi[2] > z) & (z > lo[2]);
}

// The bound test of map_mask (seal_utils.py:132-153) of one point: non-zero in every coordinate (`points.all(1)`: empty slots and exact
// zeros are never inside) and strictly inside one of the AABBs.  B: SealBoxTest or SealBrushArgs
template <class Bounds>
__device__ __forceinline__ bool seal_in_bounds(const Bounds &B, float x, float y, float z) {
    bool in = false;
    if (x != 0.0f && y != 0.0f && z != 0.0f) {
        for (uint32_t b = 0; b < B.n_bounds; b++) in |= seal_in_aabb(B.bounds[b], B.bounds[b] + 3, x, y, z);
    }
    return in;
}

// map_mask of one point: the bound test, then inside the mesh
__device__ __forceinline__ bool seal_in_box(const SealBoxTest &B, float x, float y, float z) {
    bool in = seal_in_bounds(B, x, y, z);
    if (in)
        in = any_hit(B.tris, B.n_tris, x, y, z, B.test_dir[0], B.test_dir[1], B.test_dir[2]) &&
             any_hit(B.tris, B.n_tris, x, y, z, -B.test_dir[0], -B.test_dir[1], -B.test_dir[2]);
    return in;
}

struct SealSourceArgs {
    float lo[3], hi[3];     // the source box (`empty_bound`)
    float to[3];            // `map_source`
    uint32_t tag;           // this call's tag: *flag == tag <=> some sample of this call was mapped
    uint32_t *flag;         // device word, only ever raised (atomicMax) -- tags increase from call to call, nothing is reset
};

__global__ void __launch_bounds__(256) k_seal_bbox_map(float *__restrict__ xyzs, float *__restrict__ dirs, uint32_t M, SealBoxArgs A,
                                                       uint8_t *__restrict__ mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float x = xyzs[(size_t)i * 3], y = xyzs[(size_t)i * 3 + 1], z = xyzs[(size_t)i * 3 + 2];
    const bool in = seal_in_box(A.box, x, y, z);
    mask[i] = in ? 1 : 0;
    if (!in) return;
    float m[3];
    #pragma unroll
    for (int r = 0; r < 3; r++) {
        const float moved = A.tinv[4 * r] * x + A.tinv[4 * r + 1] * y + A.tinv[4 * r + 2] * z + A.tinv[4 * r + 3];
        m[r] = (moved - A.center[r]) * A.scale[r] + A.center[r];
    }
    const float dx = dirs[(size_t)i * 3], dy = dirs[(size_t)i * 3 + 1], dz = dirs[(size_t)i * 3 + 2];
    #pragma unroll
    for (int r = 0; r < 3; r++) {
        xyzs[(size_t)i * 3 + r] = m[r];
        dirs[(size_t)i * 3 + r] = A.rinv[3 * r] * dx + A.rinv[3 * r + 1] * dy + A.rinv[3 * r + 2] * dz;
    }
}

// The samples of a call: all M slots, or -- in the device-driven loop, whose sample buffers may hold stale slots of earlier iterations
// beyond the live ones -- the slots of the iteration's live list (count read on the device: live_count[SdnLoopRecord::iteration] with the loop record).
struct SealSlots {
    const uint32_t *live_idx;     // or nullptr = slots 0 .. M-1
    const uint32_t *live_count;
    const int32_t *state;
    uint32_t M;
    __device__ __forceinline__ uint32_t count() const { return live_idx ? (state ? live_count[sdn_loop(state)->iteration] : live_count[0]) : M; }
    __device__ __forceinline__ uint32_t slot(uint32_t j) const { return live_idx ? live_idx[j] : j; }
};

// did this call map any of its samples?  (raises *flag to the call's tag)
__global__ void __launch_bounds__(256) k_seal_any(const uint8_t *__restrict__ mask, SealSlots L, uint32_t *__restrict__ flag, uint32_t tag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = j < L.count() && mask[L.slot(j)] != 0;
    const unsigned long long vote = __ballot(in ? 1 : 0);
    if (vote != 0ull && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)vote) - 1u) atomicMax(flag, tag);
}

// seal_utils.py:269-273 behind the early return of :251-252: in a call that mapped at least one sample, every UNMAPPED sample strictly
// inside the source box moves to `map_source` (the mapped ones were overwritten after the redirect in the reference: they keep theirs)
__global__ void __launch_bounds__(256) k_seal_source_redirect(float *__restrict__ xyzs, const uint8_t *__restrict__ mask, uint32_t M, SealSourceArgs S) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M || *S.flag != S.tag || mask[i]) return;
    const float x = xyzs[(size_t)i * 3], y = xyzs[(size_t)i * 3 + 1], z = xyzs[(size_t)i * 3 + 2];
    if (seal_in_aabb(S.lo, S.hi, x, y, z)) {
        xyzs[(size_t)i * 3] = S.to[0]; xyzs[(size_t)i * 3 + 1] = S.to[1]; xyzs[(size_t)i * 3 + 2] = S.to[2];
    }
}

// ---- anchor (control-point) mapper, SealAnchorMapper.map_to_origin, seal_utils.py:522-578 -------------------------------------------
// Step 1 of a call: map_mask of every slot into `mask` (k_seal_any then raises the call's flag if one of the call's samples is inside).
__global__ void __launch_bounds__(256) k_seal_box_mask(const float *__restrict__ xyzs, uint32_t M, SealBoxTest B, uint8_t *__restrict__ mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    mask[i] = seal_in_box(B, xyzs[(size_t)i * 3], xyzs[(size_t)i * 3 + 1], xyzs[(size_t)i * 3 + 2]) ? 1 : 0;
}

struct SealAnchorArgs {
    float v_anchor[3], v_offset[3], v_h[3];
    float len_h, radius;
    float scale[3];
    uint32_t tag;
    const uint32_t *flag;
};

// Step 2.  The box only gates the call (the early return of :527-528): in a call whose flag was raised the cone and plane-side
// predicates of :545-551 are evaluated for EVERY slot -- `valid_mask` is not ANDed with `map_mask` in the reference.  That includes
// the empty slots (a zero coordinate): they fail map_mask, so they never raise the flag, but they are candidates for valid_mask as any
// other point is, and are mapped when the origin-side point they hold lies in the cone (the loops never evaluate or composite them).
// The statements follow the reference's order in fp32; `d / (radius - pop)` is left to IEEE (pop == radius: +inf, or NaN for d == 0 --
// both compare false, as they do in torch).  mask: 1 for valid slots, 0 otherwise; all zeros, points untouched, in a call that maps nothing.
__global__ void __launch_bounds__(256) k_seal_anchor_apply(float *__restrict__ xyzs, uint32_t M, SealAnchorArgs A, uint8_t *__restrict__ mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (*A.flag != A.tag) { mask[i] = 0; return; }
    const float p[3] = {xyzs[(size_t)i * 3], xyzs[(size_t)i * 3 + 1], xyzs[(size_t)i * 3 + 2]};
    float proj[3], to_plane[3];                                // project_points(v_h, v_anchor, points)
    project_point(A.v_h[0], A.v_h[1], A.v_h[2], dot3(A.v_h[0], A.v_h[1], A.v_h[2], A.v_h[0], A.v_h[1], A.v_h[2]), A.v_anchor[0], A.v_anchor[1], A.v_anchor[2],
                  p[0], p[1], p[2], proj[0], proj[1], proj[2]);
    #pragma unroll
    for (int k = 0; k < 3; k++) to_plane[k] = proj[k] - p[k];
    const float d = sqrtf(dot3(to_plane[0], to_plane[1], to_plane[2], to_plane[0], to_plane[1], to_plane[2]));   // points_plane_dist
    const float offset_scale = d / A.len_h;
    float pop[3], r[3];                                        // projected_offset_points, and their offset from the anchor
    #pragma unroll
    for (int k = 0; k < 3; k++) {
        pop[k] = proj[k] - offset_scale * A.v_offset[k];
        r[k] = pop[k] - A.v_anchor[k];
    }
    const float pop_dist = sqrtf(dot3(r[0], r[1], r[2], r[0], r[1], r[2]));
    const bool in_cone = (pop_dist <= A.radius) & (d / (A.radius - pop_dist) < A.len_h / A.radius * 1.1f);
    const bool valid_side = dot3(to_plane[0], to_plane[1], to_plane[2], A.v_h[0], A.v_h[1], A.v_h[2]) > 0.0f;
    const bool valid = in_cone & valid_side;
    mask[i] = valid ? 1 : 0;
    if (!valid) return;
    const float lift = -((A.len_h - d) / 10.0f);               // v_map = lift * v_h / len_h, :555-556
    #pragma unroll
    for (int k = 0; k < 3; k++) {
        const float mapped = pop[k] - lift * A.v_h[k] / A.len_h;
        xyzs[(size_t)i * 3 + k] = (mapped - A.v_anchor[k]) * A.scale[k] + A.v_anchor[k];
    }
}

// ---- brush mapper, SealBrushMapper.map_to_origin, seal_utils.py:415-461 -----------------------------------------------------------------
// The brush's mesh has on the order of a thousand triangles (the box and anchor mappers have 12), so its map_mask does not walk them
// per lane through seal_in_box:
//   * the AABB test comes first, and the workgroup packs the slots that pass it into its leading lanes (LDS): a wave without a
//     candidate returns before the triangle loop, whatever n_tris is, and the waves that stay are full of candidates instead of
//     holding the few lanes of a ray bundle that cross the stroke;
//   * the triangle records [F][16] = v0, E1, E2, N = E1 x E2, 1 / -(d . N + eps), 1 / -(-d . N + eps), 0, 0 are prepared on the host --
//     one direction serves all points, so both inverse determinants are lane-independent -- and reach the lanes through an LDS tile
//     per wave, fetched coalesced one tile ahead (walking them with wave-uniform scalar loads was measured first: every wave then
//     waits out a load's latency per two triangles, 0.37 ms for a 2198-triangle mesh however few samples there are); the border
//     points, a few dozen, are read with wave-uniform addresses (scalar loads);
//   * the ray along d and the opposite ray share A0 = p - v0 and A0 x d (the opposite ray's cross product is its exact negation), so
//     one pass over the triangles serves both;
//   * every kBrushChunk triangles a wave stops once each of its candidates has both hits (a tile's tail is padded with NaN records,
//     which no comparison accepts, so chunks are always whole and unrolled).
// n_tris and n_border are not limited: the tiles and the border loop run over any count.
// t, u, v and eps are moller_trumbore's (:638-672); dot products are accumulated x, y, z as in any_hit.
constexpr uint32_t kBrushTriVec4 = 4;           // a triangle record is 16 floats
constexpr uint32_t kBrushTile = 64;            // triangles per LDS tile of a wave (one float4 per lane and record quarter)
constexpr uint32_t kBrushChunk = 16;
constexpr uint32_t kBrushBlock = 256;
static_assert(kBrushTile % kBrushChunk == 0 && kBrushTile * kBrushTriVec4 == 4 * 64, "a tile is whole chunks, and one float4 per lane and record quarter");

// orders the LDS stores and loads of the lanes of ONE wave (a wave's lanes run in lockstep; this keeps the compiler from moving them)
__device__ __forceinline__ void brush_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct SealBrushArgs {
    float bounds[4][6];
    uint32_t n_bounds, n_tris, n_border;
    float test_dir[3];
    float normal_expand[3], center[3];
    float attenuation_distance;
    uint32_t mode;             // 0 linear, 1 dry
};

__global__ void __launch_bounds__(kBrushBlock) k_seal_brush_map(float *__restrict__ xyzs, uint32_t M, SealBrushArgs A, const float4 *__restrict__ tris,
                                                                const float *__restrict__ border, uint8_t *__restrict__ mask) {
    __shared__ float s_p[kBrushBlock][3];
    __shared__ uint32_t s_slot[kBrushBlock];
    __shared__ uint32_t s_count[kBrushBlock / 64];
    __shared__ float4 s_tile[kBrushBlock / 64][kBrushTile * kBrushTriVec4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t i = blockIdx.x * kBrushBlock + tid;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    bool cand = false;
    if (i < M) {
        x = xyzs[(size_t)i * 3]; y = xyzs[(size_t)i * 3 + 1]; z = xyzs[(size_t)i * 3 + 2];
        cand = seal_in_bounds(A, x, y, z);
        if (!cand) mask[i] = 0;
    }
    // pack the candidates of the workgroup into its leading lanes
    const unsigned long long vote = __ballot(cand ? 1 : 0);
    if (lane == 0u) s_count[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t base = 0, total = 0;
    #pragma unroll
    for (uint32_t w = 0; w < kBrushBlock / 64; w++) {
        base += w < wave ? s_count[w] : 0u;
        total += s_count[w];
    }
    if (total == 0u) return;                                   // workgroup-uniform
    if (cand) {
        const uint32_t k = base + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
        s_p[k][0] = x; s_p[k][1] = y; s_p[k][2] = z;
        s_slot[k] = i;
    }
    __syncthreads();
    if ((tid & ~63u) >= total) return;                         // wave-uniform: no candidate left for this wave
    const bool act = tid < total;
    const float px = act ? s_p[tid][0] : 0.0f, py = act ? s_p[tid][1] : 0.0f, pz = act ? s_p[tid][2] : 0.0f;
    const uint32_t slot = act ? s_slot[tid] : 0u;
    const float dx = A.test_dir[0], dy = A.test_dir[1], dz = A.test_dir[2];
    bool hit_pos = false, hit_neg = false;
    // The wave's own LDS tile of kBrushTile triangle records: each lane fetches kBrushTriVec4 float4 of the NEXT tile (coalesced) while
    // the wave walks the current one, whose records every lane then reads at the same address (LDS broadcast).  The tile belongs to
    // one wave, so a wave-level fence orders its stores and loads and no workgroup barrier stands between the waves.
    float4 *tile = s_tile[wave];
    const uint32_t n_vec = A.n_tris * kBrushTriVec4;
    const float4 pad = make_float4(NAN, NAN, NAN, NAN);   // a record past the list: every comparison with it is false
    const auto fetch = [&](size_t first, uint32_t j) -> float4 {
        const size_t v = first + j * 64u + lane;
        float4 r = pad;
        if (v < n_vec) r = tris[v];
        return r;
    };
    float4 pre0 = fetch(0, 0), pre1 = fetch(0, 1), pre2 = fetch(0, 2), pre3 = fetch(0, 3);
    bool done = false;
    for (uint32_t t0 = 0; t0 < A.n_tris && !done; t0 += kBrushTile) {
        brush_wave_sync();                                     // the walk of the previous tile is over
        tile[lane] = pre0; tile[64u + lane] = pre1; tile[128u + lane] = pre2; tile[192u + lane] = pre3;
        const size_t next = (size_t)(t0 + kBrushTile) * kBrushTriVec4;
        pre0 = fetch(next, 0); pre1 = fetch(next, 1); pre2 = fetch(next, 2); pre3 = fetch(next, 3);
        brush_wave_sync();
        const uint32_t count = min(kBrushTile, A.n_tris - t0);
        for (uint32_t f0 = 0; f0 < count; f0 += kBrushChunk) {
            // whole chunks, unrolled, so that the LDS reads of several records are in flight at once (the tile's tail is padded)
            #pragma unroll 8
            for (uint32_t k = 0; k < kBrushChunk; k++) {
                const uint32_t f = f0 + k;
                const float4 r0 = tile[kBrushTriVec4 * f], r1 = tile[kBrushTriVec4 * f + 1], r2 = tile[kBrushTriVec4 * f + 2], r3 = tile[kBrushTriVec4 * f + 3];
                const float a0x = px - r0.x, a0y = py - r0.y, a0z = pz - r0.z;
                const float cx = a0y * dz - a0z * dy, cy = a0z * dx - a0x * dz, cz = a0x * dy - a0y * dx;   // A0 x d; A0 x (-d) is its negation
                const float ce2 = dot3(cx, cy, cz, r1.z, r1.w, r2.x);
                const float ce1 = dot3(cx, cy, cz, r0.w, r1.x, r1.y);
                const float an = dot3(a0x, a0y, a0z, r2.y, r2.z, r2.w);
                const float up = ce2 * r3.x, vp = -ce1 * r3.x, tp = an * r3.x;
                const float un = -ce2 * r3.y, vn = ce1 * r3.y, tn = an * r3.y;
                hit_pos |= (tp >= 0.0f) & (up >= 0.0f) & (vp >= 0.0f) & ((up + vp) <= 1.0f);
                hit_neg |= (tn >= 0.0f) & (un >= 0.0f) & (vn >= 0.0f) & ((un + vn) <= 1.0f);
            }
            if (__ballot((act && !(hit_pos && hit_neg)) ? 1 : 0) == 0ull) { done = true; break; }      // wave-uniform
        }
    }
    if (!act) return;
    const bool in = hit_pos && hit_neg;
    mask[slot] = in ? 1 : 0;
    if (!in || A.mode != 0u) return;                           // dry brush: the mask only, no space mapping
    const float nx = A.normal_expand[0], ny = A.normal_expand[1], nz = A.normal_expand[2];
    float qx, qy, qz;                                          // project_points(normal_expand, center, p)
    project_point(nx, ny, nz, dot3(nx, ny, nz, nx, ny, nz), A.center[0], A.center[1], A.center[2], px, py, pz, qx, qy, qz);
    // distance to the nearest border point from coordinate differences (the minimum of the squares has the minimum's root)
    float best = INFINITY;
    for (uint32_t b = 0; b < A.n_border; b++) {
        const float ex = qx - border[3 * (size_t)b], ey = qy - border[3 * (size_t)b + 1], ez = qz - border[3 * (size_t)b + 2];
        best = fminf(best, dot3(ex, ey, ez, ex, ey, ez));
    }
    const float dist = sqrtf(best);
    float ox = px - nx, oy = py - ny, oz = pz - nz;
    if (A.attenuation_distance > dist) {
        const float k = fabsf(A.attenuation_distance - dist) / A.attenuation_distance;
        ox += k * nx; oy += k * ny; oz += k * nz;
    }
    xyzs[(size_t)slot * 3] = ox; xyzs[(size_t)slot * 3 + 1] = oy; xyzs[(size_t)slot * 3 + 2] = oz;
}

// color_utils.py:31-46 for one colour: (h / 6, s, v)
__device__ __forceinline__ void rgb_to_hsv(float r, float g, float b, float &h, float &s, float &v) {
    const float cmax = fmaxf(r, fmaxf(g, b)), cmin = fminf(r, fminf(g, b));
    const float delta = cmax - cmin;
    if (delta == 0.0f) h = 0.0f;
    else if (r >= g && r >= b) { h = (g - b) / delta; h = h - 6.0f * floorf(h / 6.0f); }   // torch `% 6` (the result has the divisor's sign); the first maximum wins ties
    else if (g >= b) h = (b - r) / delta + 2.0f;
    else h = (r - g) / delta + 4.0f;
    h = h / 6.0f;
    s = cmax == 0.0f ? 0.0f : delta / cmax;
    v = cmax;
}
// color_utils.py:49-63
__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float &o0, float &o1, float &o2) {
    const float c = v * s;
    const float h6 = h * 6.0f;
    const float xx = c * (-fabsf((h6 - 2.0f * floorf(h6 / 2.0f)) - 1.0f) + 1.0f);
    const float m = v - c;
    const uint32_t idx = ((uint32_t)(uint8_t)(int)h6) % 6u;   // `.type(torch.uint8)` truncation, then % 6
    switch (idx) {
        case 0: o0 = c; o1 = xx; o2 = 0; break;
        case 1: o0 = xx; o1 = c; o2 = 0; break;
        case 2: o0 = 0; o1 = c; o2 = xx; break;
        case 3: o0 = 0; o1 = xx; o2 = c; break;
        case 4: o0 = xx; o1 = 0; o2 = c; break;
        default: o0 = c; o1 = 0; o2 = xx; break;
    }
    o0 += m; o1 += m; o2 += m;
}

// modify_rgb, pass 1: sum and count of V = max(r, g, b) over the masked samples.  The sum is taken in 2^-40 fixed point in a 64-bit
// integer: exact for the fp16- or fp32-valued colours of [0, 1] up to 2^-40 per sample and, above all, INDEPENDENT OF THE ORDER -- the
// host-stepped loop and the device loop hold the same samples in different slots and must tint them by the same mean, bit for bit
// (torch.mean's own fp32 pairwise order is library-defined; the two agree to ~1e-7, far inside the 1e-4 bar of the fixture test).
constexpr double kSealFixedOne = 1099511627776.0;      // 1.0 in 2^-40 fixed point
__device__ __forceinline__ unsigned long long seal_rgb_fixed_v(const float *__restrict__ rgbs, uint32_t i) {
    const float mx = fmaxf(rgbs[(size_t)i * 3], fmaxf(rgbs[(size_t)i * 3 + 1], rgbs[(size_t)i * 3 + 2]));
    return (unsigned long long)((double)fminf(fmaxf(mx, 0.0f), 4.0f) * kSealFixedOne + 0.5);
}
__global__ void __launch_bounds__(256) k_seal_rgb_sum(const float *__restrict__ rgbs, const uint8_t *__restrict__ mask, SealSlots L,
                                                      unsigned long long *__restrict__ acc) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = 0ull, c = 0ull;
    const uint32_t i = j < L.count() ? L.slot(j) : 0u;
    if (j < L.count() && mask[i]) {
        v = seal_rgb_fixed_v(rgbs, i);
        c = 1ull;
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v += __shfl_down(v, off, 64);
        c += __shfl_down(c, off, 64);
    }
    if ((threadIdx.x & 63u) == 0u && c != 0ull) {
        atomicAdd(&acc[0], v);
        atomicAdd(&acc[1], c);
    }
}
// the mean V of a {sum, count} pair (count != 0)
__device__ __forceinline__ float seal_mean_v(const unsigned long long *__restrict__ acc) {
    return (float)(((double)acc[0] / kSealFixedOne) / (double)acc[1]);
}
// pass 2 of one sample (k_seal_apply), the tint: hue and saturation of the target colour, brightness re-centred on it
// (seal_utils.py:769-775), -> rgb, in place.  acc: the {sum, count} pair of the call the slot belongs to (count != 0)
struct SealTint {
    float r, g, b, light_offset;
    __device__ __forceinline__ void operator()(float *__restrict__ rgbs, uint32_t i, const unsigned long long *__restrict__ acc) const {
        const float mean = seal_mean_v(acc);
        float h, s, v, mh, ms, mv;
        rgb_to_hsv(rgbs[(size_t)i * 3], rgbs[(size_t)i * 3 + 1], rgbs[(size_t)i * 3 + 2], h, s, v);
        rgb_to_hsv(r, g, b, mh, ms, mv);
        const float nv = fminf(1.0f, fmaxf(0.0f, (mv + (v - mean)) + light_offset));
        float o0, o1, o2;
        hsv_to_rgb(mh, ms, nv, o0, o1, o2);
        rgbs[(size_t)i * 3] = o0; rgbs[(size_t)i * 3 + 1] = o1; rgbs[(size_t)i * 3 + 2] = o2;
    }
};

// ---- the tint of a WHOLE-RAY sample list (the one-pass renderer: march_rays_train's (offset, count) layout, every ray's samples up front) --
// modify_rgb re-centres brightness on the mean V of the masked samples of ONE map_color call, and in the inference loop a call is one
// iteration (SealDNeRF/renderer.py:271-272).  Which samples share an iteration follows from the sample counts, the sigmas and the
// loop's rule n_step = max(min(N // n_alive, 8), 1) alone -- the tint changes colours, never which ray dies when -- so the loop's
// schedule is replayed here after the one field launch, and the two tint passes run per iteration on the result.
constexpr int32_t kNoIteration = -1;          // slot_iter of a slot the loop never marched (0xFF bytes: the call's memset writes it)
constexpr uint32_t kScheduleBlock = 1024;     // the replay is ONE workgroup; each lane keeps up to kScheduleMaxPerLane rays in registers
constexpr uint32_t kScheduleMaxPerLane = 16;

// Phase A, one lane per ray: {index of the sample at which the loop kills the ray, number of samples}.  The kill is k_composite_rays':
// the first sample whose transmittance IN FRONT of it (1 - weights_sum, accumulated by composite_step) is < T_thresh -- that sample is
// still composited -- else the sample count.  A zero step length ends the ray's list (as in k_composite_whole_rays); a ray whose
// samples did not fit the buffer has none (as there).
__global__ void __launch_bounds__(256) k_whole_rays_stop(const float *__restrict__ sigmas, const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                         uint32_t M, uint32_t N, float T_thresh, int32_t *__restrict__ ray_stop) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const uint32_t offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    uint32_t stop = 0, count = 0;
    if (num_steps != 0 && (uint64_t)offset + num_steps <= (uint64_t)M) {
        const float *s = sigmas + offset, *dl = deltas + (size_t)offset * 2;
        CompositeAcc a = {0, 0, 0, 0, 0, 0};
        stop = count = num_steps;
        for (uint32_t step = 0; step < num_steps; step++) {
            if (dl[0] == 0) { stop = count = step; break; }
            if (composite_step(a, s[0], dl[0], dl[1], 0.0f, 0.0f, 0.0f) < T_thresh) { stop = step; break; }
            s++; dl += 2;
        }
    }
    ray_stop[n * 2] = (int32_t)stop;
    ray_stop[n * 2 + 1] = (int32_t)count;
}

// Phase B, one workgroup: the loop of dnerf/renderer.py:340-381 on the rays' progress alone.  Per iteration: count the alive rays
// (wave shuffles + LDS, two LDS rows used in turn so that one barrier per iteration is enough), n_step exactly as advance_record
// (render_loop.hip) and the reference set it, every alive ray stamps the slots the marcher would have filled -- [pos, pos + n_step),
// cut at its sample count, INCLUDING those behind a kill inside the window: the loop marched, evaluated and averaged them -- and dies
// when k_composite_rays would have killed it: its stop sample lies in the window (for a ray without one, stop == count: fewer than
// n_step samples were left).  Ends as the loop does: step >= max_steps, or nobody alive.
template <uint32_t R>
__global__ void __launch_bounds__(kScheduleBlock) k_whole_rays_schedule(const int32_t *__restrict__ rays, const int32_t *__restrict__ ray_stop, uint32_t N,
                                                                        uint32_t max_steps, int32_t *__restrict__ slot_iter, int32_t *__restrict__ n_iter) {
    __shared__ uint32_t s_alive[2][kScheduleBlock / 64];
    uint32_t pos[R], stop[R], count[R], offset[R];
    uint32_t alive = 0;                        // bit k: ray k * kScheduleBlock + threadIdx.x is alive
    #pragma unroll
    for (uint32_t k = 0; k < R; k++) {
        const uint32_t n = k * kScheduleBlock + threadIdx.x;
        pos[k] = 0; stop[k] = 0; count[k] = 0; offset[k] = 0;
        if (n < N) {
            offset[k] = (uint32_t)rays[n * 3 + 1];
            stop[k] = (uint32_t)ray_stop[n * 2];
            count[k] = (uint32_t)ray_stop[n * 2 + 1];
            alive |= 1u << k;
        }
    }
    uint32_t step = 0, it = 0;
    while (true) {
        uint32_t c = (uint32_t)__popc(alive);
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if ((threadIdx.x & 63u) == 0u) s_alive[it & 1u][threadIdx.x >> 6] = c;
        __syncthreads();
        uint32_t n_alive = 0;
        #pragma unroll
        for (uint32_t w = 0; w < kScheduleBlock / 64; w++) n_alive += s_alive[it & 1u][w];
        if (step >= max_steps || n_alive == 0) break;          // workgroup-uniform
        const uint32_t ns = N / n_alive;
        const uint32_t n_step = ns > 8u ? 8u : (ns < 1u ? 1u : ns);
        #pragma unroll
        for (uint32_t k = 0; k < R; k++) {
            if (alive & (1u << k)) {
                const uint32_t end = min(pos[k] + n_step, count[k]);
                for (uint32_t q = pos[k]; q < end; q++) slot_iter[(size_t)offset[k] + q] = (int32_t)it;
                if (stop[k] < pos[k] + n_step) alive &= ~(1u << k);
                else pos[k] += n_step;
            }
        }
        step += n_step;
        it++;
    }
    if (threadIdx.x == 0) n_iter[0] = (int32_t)it;
}

// pass 1 per iteration: acc[2 * it + {0, 1}] += {V, 1} of the masked slots of iteration it.  A wave's 64 slots span a few iterations:
// it reduces one iteration at a time (that of its first pending lane) and adds one pair per iteration it holds.
__global__ void __launch_bounds__(256) k_seal_rgb_sum_iter(const float *__restrict__ rgbs, const uint8_t *__restrict__ mask, const int32_t *__restrict__ slot_iter,
                                                           uint32_t M, unsigned long long *__restrict__ acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t it = i < M ? slot_iter[i] : kNoIteration;
    const bool in = it != kNoIteration && mask[i] != 0;
    const unsigned long long mine = in ? seal_rgb_fixed_v(rgbs, i) : 0ull;
    unsigned long long pending = __ballot(in ? 1 : 0);
    while (pending != 0ull) {                                   // wave-uniform
        const int32_t cur = __shfl(it, __ffsll((long long)pending) - 1, 64);
        const bool now = in && it == cur;
        unsigned long long v = now ? mine : 0ull, c = now ? 1ull : 0ull;
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            v += __shfl_down(v, off, 64);
            c += __shfl_down(c, off, 64);
        }
        if ((threadIdx.x & 63u) == 0u) {
            atomicAdd(&acc[2 * (size_t)cur], v);
            atomicAdd(&acc[2 * (size_t)cur + 1], c);
        }
        pending &= ~__ballot(now ? 1 : 0);
    }
}

// ---- the brush's texture stamp, the `image` branch of SealMapper.map_color, seal_utils.py:58-79 -------------------------------------------
// A streaming pass: per masked sample 12 + 12 bytes of position and colour in, one 16-byte texel record, 12 bytes out.  The texture is
// read straight from global memory (a 256 x 256 stamp is 1 MiB of records: it stays in L2); nothing is staged in LDS.
struct SealImageArgs {
    const float4 *texels;      // [H][W]: hue / 6, saturation, value of the texel (rgb_to_hsv, once, k_seal_image_texels), alpha
    uint32_t W, H;
    float v_o[3], v_norm[3], v_ow[3], v_oh[3];
    float norm_sq, len_ow_sq, len_oh_sq, light_offset;
};

// r, g, b, alpha -> hue / 6, saturation, value, alpha, in place: what modify_rgb's `rgb2hsv_torch(modification)` gives for this texel,
// by the helper the per-sample conversion uses -- the same values as converting the texel for every sample
__global__ void __launch_bounds__(256) k_seal_image_texels(float4 *__restrict__ texels, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 t = texels[i];
    float h, s, v;
    rgb_to_hsv(t.x, t.y, t.z, h, s, v);
    texels[i] = make_float4(h, s, v, t.w);
}

// pass 2 of one sample (k_seal_apply), the stamp: the reference's fp32 statements in their order (dot products accumulated x, y, z).
// xyzs: the samples' mapped positions; acc: the {sum, count} pair of the call the slot belongs to (count != 0)
struct SealStamp {
    const float *xyzs;
    SealImageArgs A;
    __device__ __forceinline__ void operator()(float *__restrict__ rgbs, uint32_t i, const unsigned long long *__restrict__ acc) const {
        const float mean = seal_mean_v(acc);
        const float px = xyzs[(size_t)i * 3], py = xyzs[(size_t)i * 3 + 1], pz = xyzs[(size_t)i * 3 + 2];
        float qx, qy, qz;                                                                            // project_points(v_image_norm, v_image_o, points)
        project_point(A.v_norm[0], A.v_norm[1], A.v_norm[2], A.norm_sq, A.v_o[0], A.v_o[1], A.v_o[2], px, py, pz, qx, qy, qz);
        const float ox = qx - A.v_o[0], oy = qy - A.v_o[1], oz = qz - A.v_o[2];                      // v_op
        // idx = min(max(0, floor(v_op . v_ow / len_ow^2 * W)), W - 1), :72-75 (fmaxf sends a NaN to texel 0: the index stays in bounds)
        const float fw = floorf(dot3(ox, oy, oz, A.v_ow[0], A.v_ow[1], A.v_ow[2]) / A.len_ow_sq * (float)A.W);
        const float fh = floorf(dot3(ox, oy, oz, A.v_oh[0], A.v_oh[1], A.v_oh[2]) / A.len_oh_sq * (float)A.H);
        // (the upper clamp is taken on integers: (float)(W - 1) may round up for W > 2^24; W, H < 2^28)
        const uint32_t iw = min((uint32_t)fminf(fmaxf(fw, 0.0f), 268435456.0f), A.W - 1u);
        const uint32_t ih = min((uint32_t)fminf(fmaxf(fh, 0.0f), 268435456.0f), A.H - 1u);
        const float4 tex = A.texels[(size_t)ih * A.W + iw];
        // modify_rgb(colors, image[idx_h, idx_w], rgb_light_offset), :761-777
        const float r = rgbs[(size_t)i * 3], g = rgbs[(size_t)i * 3 + 1], b = rgbs[(size_t)i * 3 + 2];
        float h, s, v;
        rgb_to_hsv(r, g, b, h, s, v);
        const float nv = fminf(1.0f, fmaxf(0.0f, (tex.z + (v - mean)) + A.light_offset));
        float o0, o1, o2;
        hsv_to_rgb(tex.x, tex.y, nv, o0, o1, o2);
        // colors = mask * modified + (1 - mask) * colors, :79
        const float a = tex.w, na = 1.0f - tex.w;
        rgbs[(size_t)i * 3] = a * o0 + na * r; rgbs[(size_t)i * 3 + 1] = a * o1 + na * g; rgbs[(size_t)i * 3 + 2] = a * o2 + na * b;
    }
};

// pass 2, the tint (Op = SealTint) or the stamp (SealStamp) of the masked slots, each by the mean of the call it belongs to: acc is the
// call's {sum, count} pair, or, for a whole-ray list (kPerIteration), the pairs of its iterations -- a slot takes that of its own.  A
// masked slot of a call none of whose samples is masked (count == 0: the slot lies outside the call's live list) and a slot the loop
// never marched are left alone
template <bool kPerIteration, class Op>
__global__ void __launch_bounds__(256) k_seal_apply(float *__restrict__ rgbs, const uint8_t *__restrict__ mask, const int32_t *__restrict__ slot_iter,
                                                    uint32_t M, Op op, const unsigned long long *__restrict__ acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M || !mask[i]) return;
    if (kPerIteration) {
        const int32_t it = slot_iter[i];
        if (it == kNoIteration) return;
        acc += 2 * (size_t)it;
    }
    if (acc[1] == 0ull) return;
    op(rgbs, i, acc);
}

// color_utils.py:31-63 + seal_utils.py:747-758 on the masked samples, in place
__global__ void __launch_bounds__(256) k_seal_hsv(float *__restrict__ rgbs, const uint8_t *__restrict__ mask, uint32_t M, float mh, float ms, float mv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M || !mask[i]) return;
    const float r = rgbs[(size_t)i * 3], g = rgbs[(size_t)i * 3 + 1], b = rgbs[(size_t)i * 3 + 2];
    float h, s, v, o0, o1, o2;
    rgb_to_hsv(r, g, b, h, s, v);
    hsv_to_rgb(h + mh, s + ms, v + mv, o0, o1, o2);
    rgbs[(size_t)i * 3] = o0; rgbs[(size_t)i * 3 + 1] = o1; rgbs[(size_t)i * 3 + 2] = o2;
}

// One tag per call that asks "did this call map anything": unique in the process, so any flag word sees increasing tags whichever entry
// points share it (a wrap after 2^32 calls would need the flag cleared: not in this process's life)
std::atomic<uint32_t> g_seal_tag{0};

// one lane per element (sample slot, ray): kernel(args...) over n lanes
template <class... Params, class... Args>
void launch_lanes(void (*kernel)(Params...), uint32_t n, void *stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(sdn_div_up(n, 256u)), dim3(256), 0, (hipStream_t)stream, args...);
}

// checks and fills what the box test and the brush's arguments share: bounds, n_bounds, n_tris, test_dir (B: SealBoxTest or SealBrushArgs)
template <class B>
int fill_bounds(B &b, const float *bounds, uint32_t n_bounds, const float *tris, uint32_t n_tris, const float *test_dir) {
    if (!bounds || !tris || !test_dir) return SDN_E_BADARG;
    if (n_bounds == 0 || n_bounds > 4 || n_tris == 0) return SDN_E_UNSUPPORTED;
    for (uint32_t k = 0; k < n_bounds; k++)
        for (int j = 0; j < 6; j++) b.bounds[k][j] = bounds[6 * k + j];
    b.n_bounds = n_bounds; b.n_tris = n_tris;
    for (int k = 0; k < 3; k++) b.test_dir[k] = test_dir[k];
    return 0;
}

int fill_box_test(SealBoxTest &b, const float *bounds, uint32_t n_bounds, const float *tris, uint32_t n_tris, const float *test_dir) {
    b.tris = tris;
    return fill_bounds(b, bounds, n_bounds, tris, n_tris, test_dir);
}

int fill_image_args(SealImageArgs &a, const SdnSealImage *im) {
    if (!im || !im->texels || ((uintptr_t)im->texels & 15u) != 0) return SDN_E_BADARG;
    if (im->W == 0 || im->H == 0 || (uint64_t)im->W * im->H >= (1ull << 28)) return SDN_E_UNSUPPORTED;
    a.texels = (const float4 *)im->texels; a.W = im->W; a.H = im->H;
    for (int k = 0; k < 3; k++) { a.v_o[k] = im->v_o[k]; a.v_norm[k] = im->v_norm[k]; a.v_ow[k] = im->v_ow[k]; a.v_oh[k] = im->v_oh[k]; }
    a.norm_sq = im->norm_sq; a.len_ow_sq = im->len_ow_sq; a.len_oh_sq = im->len_oh_sq; a.light_offset = im->light_offset;
    return 0;
}

// The two passes of modify_rgb with `op` (SealTint, SealStamp) as the second, on the masked samples of one call: clear the {sum, count}
// pair in scratch16, sum V over the call's samples L, apply.  Three stream operations.
template <class Op>
int seal_recolour(float *rgbs, const uint8_t *mask, uint32_t M, const Op &op, void *scratch16, const SealSlots &L, void *stream) {
    if (hipMemsetAsync(scratch16, 0, 16, (hipStream_t)stream) != hipSuccess) return sdn_launch_status();
    launch_lanes(k_seal_rgb_sum, M, stream, rgbs, mask, L, (unsigned long long *)scratch16);
    launch_lanes(k_seal_apply<false, Op>, M, stream, rgbs, mask, nullptr, M, op, (const unsigned long long *)scratch16);
    return sdn_launch_status();
}

// The same on a whole-ray sample list, as the inference loop does it: sdn_whole_rays_schedule, then the two passes per iteration.
// scratch: 16 * (max_steps + 8) bytes (cleared here).  Six stream operations.
template <class Op>
int seal_recolour_whole_rays(float *rgbs, const uint8_t *mask, const int32_t *rays, const float *sigmas, const float *deltas, uint32_t M, uint32_t N,
                             float T_thresh, uint32_t max_steps, const Op &op, void *scratch, int32_t *ray_stop, int32_t *slot_iter, int32_t *n_iter,
                             void *stream) {
    if (int rc = sdn_whole_rays_schedule(rays, sigmas, deltas, M, N, T_thresh, max_steps, ray_stop, slot_iter, n_iter, stream)) return rc;
    if (hipMemsetAsync(scratch, 0, 16 * ((size_t)max_steps + 8), (hipStream_t)stream) != hipSuccess) return sdn_launch_status();
    launch_lanes(k_seal_rgb_sum_iter, M, stream, rgbs, mask, slot_iter, M, (unsigned long long *)scratch);
    launch_lanes(k_seal_apply<true, Op>, M, stream, rgbs, mask, slot_iter, M, op, (const unsigned long long *)scratch);
    return sdn_launch_status();
}

}  // namespace

extern "C" {

int sdn_seal_bbox_map(float *xyzs, float *dirs, uint32_t M, const float *bounds, uint32_t n_bounds, const float *tris, uint32_t n_tris,
                      const float *test_dir, const float *tinv, const float *rinv, const float *scale, const float *center, uint8_t *mask,
                      void *stream) {
    if (M == 0) return 0;
    if (!xyzs || !dirs || !tinv || !rinv || !scale || !center || !mask) return SDN_E_BADARG;
    SealBoxArgs a;
    if (int rc = fill_box_test(a.box, bounds, n_bounds, tris, n_tris, test_dir)) return rc;
    for (int k = 0; k < 3; k++) { a.scale[k] = scale[k]; a.center[k] = center[k]; }
    for (int k = 0; k < 12; k++) a.tinv[k] = tinv[k];
    for (int k = 0; k < 9; k++) a.rinv[k] = rinv[k];
    launch_lanes(k_seal_bbox_map, M, stream, xyzs, dirs, M, a, mask);
    return sdn_launch_status();
}

// sdn_seal_bbox_map with the `mapSource` option: source_bound {lo xyz, hi xyz}, map_source [3]; flag: one device word owned by the caller
// (zeroed once when allocated; raised to this call's tag if one of the call's samples is mapped).  live_idx / live_count / state: the
// call's samples as a list (the device-driven loop; all NULL = the M slots).  Three launches, no host synchronisation.
int sdn_seal_bbox_map_source(float *xyzs, float *dirs, uint32_t M, const float *bounds, uint32_t n_bounds, const float *tris, uint32_t n_tris,
                             const float *test_dir, const float *tinv, const float *rinv, const float *scale, const float *center,
                             const float *source_bound, const float *map_source, uint32_t *flag, uint8_t *mask, const uint32_t *live_idx,
                             const uint32_t *live_count, const int32_t *state, void *stream) {
    if (M == 0) return 0;
    if (!source_bound || !map_source || !flag || (live_idx && !live_count)) return SDN_E_BADARG;
    int rc = sdn_seal_bbox_map(xyzs, dirs, M, bounds, n_bounds, tris, n_tris, test_dir, tinv, rinv, scale, center, mask, stream);
    if (rc) return rc;
    const uint32_t tag = ++g_seal_tag;
    SealSourceArgs sa;
    for (int k = 0; k < 3; k++) { sa.lo[k] = source_bound[k]; sa.hi[k] = source_bound[3 + k]; sa.to[k] = map_source[k]; }
    sa.tag = tag; sa.flag = flag;
    const SealSlots L{live_idx, live_count, state, M};
    launch_lanes(k_seal_any, M, stream, mask, L, flag, tag);
    launch_lanes(k_seal_source_redirect, M, stream, xyzs, mask, M, sa);
    return sdn_launch_status();
}

// SealAnchorMapper.map_to_origin (seal_utils.py:522-578), in place on xyzs (dirs are returned unchanged by the reference and are not
// touched: the pointer is accepted for symmetry and may be NULL).  flag, live list: as for sdn_seal_bbox_map_source -- the flag is raised
// when a sample OF THE CALL lies in the box, and then every one of the M slots is tested against the cone.  Three launches, no host
// synchronisation.
int sdn_seal_anchor_map(float *xyzs, float *dirs, uint32_t M, const float *bounds, uint32_t n_bounds, const float *tris, uint32_t n_tris,
                        const float *test_dir, const float *v_anchor, const float *v_offset, const float *v_h, float len_h, float radius,
                        const float *scale, uint32_t *flag, uint8_t *mask, const uint32_t *live_idx, const uint32_t *live_count,
                        const int32_t *state, void *stream) {
    (void)dirs;
    if (M == 0) return 0;
    if (!xyzs || !v_anchor || !v_offset || !v_h || !scale || !flag || !mask || (live_idx && !live_count)) return SDN_E_BADARG;
    SealBoxTest b;
    if (int rc = fill_box_test(b, bounds, n_bounds, tris, n_tris, test_dir)) return rc;
    SealAnchorArgs a;
    for (int k = 0; k < 3; k++) { a.v_anchor[k] = v_anchor[k]; a.v_offset[k] = v_offset[k]; a.v_h[k] = v_h[k]; a.scale[k] = scale[k]; }
    a.len_h = len_h; a.radius = radius; a.flag = flag;
    const uint32_t tag = a.tag = ++g_seal_tag;
    const SealSlots L{live_idx, live_count, state, M};
    launch_lanes(k_seal_box_mask, M, stream, xyzs, M, b, mask);
    launch_lanes(k_seal_any, M, stream, mask, L, flag, tag);
    launch_lanes(k_seal_anchor_apply, M, stream, xyzs, M, a, mask);
    return sdn_launch_status();
}

// SealBrushMapper.map_to_origin (seal_utils.py:415-461), in place on xyzs; dirs are not read or written.  Every slot is mapped on its own:
// no flag word, no live list.  One launch, no host synchronisation.
int sdn_seal_brush_map(float *xyzs, float *dirs, uint32_t M, const float *bounds, uint32_t n_bounds, const float *tris, uint32_t n_tris,
                       const float *test_dir, const float *normal_expand, const float *center, float attenuation_distance, uint32_t mode,
                       const float *border, uint32_t n_border, uint8_t *mask, void *stream) {
    (void)dirs;
    if (M == 0) return 0;
    if (!xyzs || !normal_expand || !center || !mask || ((uintptr_t)tris & 15u) != 0) return SDN_E_BADARG;
    SealBrushArgs a;
    if (int rc = fill_bounds(a, bounds, n_bounds, tris, n_tris, test_dir)) return rc;      // (its NULL checks before every count check, as above)
    if (mode > 1u) return SDN_E_UNSUPPORTED;
    if (mode == 0u && (!border || n_border == 0)) return SDN_E_BADARG;
    a.n_border = n_border;
    for (int k = 0; k < 3; k++) { a.normal_expand[k] = normal_expand[k]; a.center[k] = center[k]; }
    a.attenuation_distance = attenuation_distance; a.mode = mode;
    hipLaunchKernelGGL(k_seal_brush_map, dim3(sdn_div_up(M, kBrushBlock)), dim3(kBrushBlock), 0, (hipStream_t)stream, xyzs, M, a, (const float4 *)tris, border,
                       mask);
    return sdn_launch_status();
}

// modify_rgb (seal_utils.py:761-777) on the masked samples, in place: target colour rgb [3], light offset; scratch: 16 bytes of device
// memory (cleared here); live list as above (the MEAN is taken over the call's samples only).  Three stream operations, no host
// synchronisation; the mean is order-independent (see k_seal_rgb_sum).
int sdn_seal_modify_rgb(float *rgbs, const uint8_t *mask, uint32_t M, float r, float g, float b, float light_offset, void *scratch16,
                        const uint32_t *live_idx, const uint32_t *live_count, const int32_t *state, void *stream) {
    if (M == 0) return 0;
    if (!rgbs || !mask || !scratch16 || ((uintptr_t)scratch16 & 7u) != 0 || (live_idx && !live_count)) return SDN_E_BADARG;
    return seal_recolour(rgbs, mask, M, SealTint{r, g, b, light_offset}, scratch16, SealSlots{live_idx, live_count, state, M}, stream);
}

uint32_t sdn_whole_rays_schedule_max_rays(void) { return kScheduleBlock * kScheduleMaxPerLane; }

// The inference loop's schedule for a whole-ray sample list: slot_iter[p] = the iteration of dnerf/renderer.py:340-381 in which the loop
// marches sample slot p, -1 for a slot it never marches; n_iter[0] = its iteration count.  Three stream operations, no host
// synchronisation.
int sdn_whole_rays_schedule(const int32_t *rays, const float *sigmas, const float *deltas, uint32_t M, uint32_t N, float T_thresh, uint32_t max_steps,
                            int32_t *ray_stop, int32_t *slot_iter, int32_t *n_iter, void *stream) {
    if (!rays || !sigmas || !deltas || !ray_stop || !slot_iter || !n_iter || M == 0 || N == 0 || max_steps == 0) return SDN_E_BADARG;
    if (N > kScheduleBlock * kScheduleMaxPerLane) return SDN_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(slot_iter, 0xFF, (size_t)M * sizeof(int32_t), st) != hipSuccess) return sdn_launch_status();
    launch_lanes(k_whole_rays_stop, N, stream, sigmas, deltas, rays, M, N, T_thresh, ray_stop);
    const uint32_t per_lane = sdn_div_up(N, kScheduleBlock);
    #define SDN_SCHEDULE(R) hipLaunchKernelGGL(k_whole_rays_schedule<R>, dim3(1), dim3(kScheduleBlock), 0, st, rays, (const int32_t *)ray_stop, N, max_steps, slot_iter, n_iter)
    if (per_lane <= 1) SDN_SCHEDULE(1);
    else if (per_lane <= 2) SDN_SCHEDULE(2);
    else if (per_lane <= 4) SDN_SCHEDULE(4);
    else if (per_lane <= 8) SDN_SCHEDULE(8);
    else SDN_SCHEDULE(16);
    #undef SDN_SCHEDULE
    return sdn_launch_status();
}

// modify_rgb on a whole-ray sample list, in place, tinted as the inference loop tints it: sdn_whole_rays_schedule, then the two passes of
// sdn_seal_modify_rgb per iteration.  scratch: 16 * (max_steps + 8) bytes, 8-byte aligned (cleared here).  Six stream operations.
int sdn_seal_modify_rgb_whole_rays(float *rgbs, const uint8_t *mask, const int32_t *rays, const float *sigmas, const float *deltas, uint32_t M, uint32_t N,
                                   float T_thresh, uint32_t max_steps, float r, float g, float b, float light_offset, void *scratch,
                                   int32_t *ray_stop, int32_t *slot_iter, int32_t *n_iter, void *stream) {
    if (M == 0 || N == 0) return 0;
    if (!rgbs || !mask || !scratch || ((uintptr_t)scratch & 7u) != 0) return SDN_E_BADARG;
    return seal_recolour_whole_rays(rgbs, mask, rays, sigmas, deltas, M, N, T_thresh, max_steps, SealTint{r, g, b, light_offset}, scratch, ray_stop, slot_iter,
                                    n_iter, stream);
}

int sdn_seal_image_texels(float *texels, uint64_t n, void *stream) {
    if (n == 0) return 0;
    if (!texels || ((uintptr_t)texels & 15u) != 0) return SDN_E_BADARG;
    if (n >= (1ull << 28)) return SDN_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_seal_image_texels, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, (float4 *)texels, n);
    return sdn_launch_status();
}

// The `image` branch of map_color (seal_utils.py:58-79) on the masked samples, in place; xyzs: their mapped positions.  The sum pass is
// sdn_seal_modify_rgb's (k_seal_rgb_sum: every masked sample of the call, wherever it lands on the texture).  Three stream operations.
int sdn_seal_modify_image(float *rgbs, const float *xyzs, const uint8_t *mask, uint32_t M, const SdnSealImage *image, void *scratch16,
                          const uint32_t *live_idx, const uint32_t *live_count, const int32_t *state, void *stream) {
    if (M == 0) return 0;
    if (!rgbs || !xyzs || !mask || !scratch16 || ((uintptr_t)scratch16 & 7u) != 0 || (live_idx && !live_count)) return SDN_E_BADARG;
    SealStamp op{xyzs, {}};
    if (int rc = fill_image_args(op.A, image)) return rc;
    return seal_recolour(rgbs, mask, M, op, scratch16, SealSlots{live_idx, live_count, state, M}, stream);
}

// The stamp on a whole-ray sample list, as the inference loop applies it: sdn_whole_rays_schedule, the per-iteration sum pass of
// sdn_seal_modify_rgb_whole_rays, then the per-iteration stamp.  scratch: 16 * (max_steps + 8) bytes, 8-byte aligned (cleared here).
int sdn_seal_modify_image_whole_rays(float *rgbs, const float *xyzs, const uint8_t *mask, const int32_t *rays, const float *sigmas, const float *deltas,
                                     uint32_t M, uint32_t N, float T_thresh, uint32_t max_steps, const SdnSealImage *image, void *scratch,
                                     int32_t *ray_stop, int32_t *slot_iter, int32_t *n_iter, void *stream) {
    if (M == 0 || N == 0) return 0;
    if (!rgbs || !xyzs || !mask || !scratch || ((uintptr_t)scratch & 7u) != 0) return SDN_E_BADARG;
    SealStamp op{xyzs, {}};
    if (int rc = fill_image_args(op.A, image)) return rc;
    return seal_recolour_whole_rays(rgbs, mask, rays, sigmas, deltas, M, N, T_thresh, max_steps, op, scratch, ray_stop, slot_iter, n_iter, stream);
}

int sdn_seal_modify_hsv(float *rgbs, const uint8_t *mask, uint32_t M, float dh, float ds, float dv, void *stream) {
    if (M == 0) return 0;
    if (!rgbs || !mask) return SDN_E_BADARG;
    launch_lanes(k_seal_hsv, M, stream, rgbs, mask, M, dh, ds, dv);
    return sdn_launch_status();
}

}  // extern "C"
