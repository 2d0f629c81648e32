// Occupancy-grid ray marching + alpha compositing for gfx950 (MI355X).
//
// Behavioural contract: raymarching/src/raymarching.cu of the reference
// (line ranges cited per kernel).  Arithmetic contract: this file is built with
// -ffp-contract=off so that every float operation rounds on its own, in the
// order the reference source writes it -- which is what oracle/sdn_oracle.c
// evaluates on the CPU; ray/sample indices and counts are therefore bit-exact
// against the oracle, not merely close.
//
// Layout notes (MI355X): one lane per ray, 256-thread workgroups (4 waves, one
// per SIMD).  The density bitfield of one time slice is 256 KiB and lives in the
// XCD's L2 after first touch; the marcher is bound by dependent L2 byte gathers
// and by wave divergence, not by HBM.  Rays keep image order in rays_alive
// (stable compaction), so a wave's 64 rays are neighbouring pixels and take
// similar trip counts.
#include <stdlib.h>

#include "sdn_common.h"
#include "sdn_internal.h"

namespace {
using sdn_int::FrameSel;

constexpr float kSqrt3 = 1.7320508075688772f;
constexpr float kRPi = 0.3183098861837907f;

__device__ __forceinline__ float signf_(float x) { return copysignf(1.0f, x); }
__device__ __forceinline__ float clampf_(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }

// raymarching.cu:42-47
__device__ __forceinline__ int mip_from_pos(float x, float y, float z, float max_cascade) {
    const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    int exponent;
    frexpf(mx, &exponent);
    return (int)fminf(max_cascade - 1, fmaxf(0.0f, (float)exponent));
}
// raymarching.cu:49-54
__device__ __forceinline__ int mip_from_dt(float dt, float H, float max_cascade) {
    const float mx = (float)((double)(dt * H) * 0.5);
    int exponent;
    frexpf(mx, &exponent);
    return (int)fminf(max_cascade - 1, fmaxf(0.0f, (float)exponent));
}
// raymarching.cu:56-81
__host__ __device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__host__ __device__ __forceinline__ uint32_t morton3D_(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
// coordinates < 256: the first spreading step of expand_bits is the identity
__device__ __forceinline__ uint32_t expand_bits8(uint32_t v) {
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3D_8bit(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits8(x) | (expand_bits8(y) << 1) | (expand_bits8(z) << 2);
}
__host__ __device__ __forceinline__ uint32_t morton3D_invert_(uint32_t x) {
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

// ---------------------------------------------------------------------------
// The DDA stepper shared by the three marching kernels
// (raymarching.cu:359-400 == 427-479 == 750-804).
// ---------------------------------------------------------------------------
constexpr uint32_t kCullRes = 32;  // cull grid resolution (see "Exact early-out" below)
constexpr uint32_t kCullWords = kCullRes * kCullRes * kCullRes / 32;  // 1024 words of marks, followed by 8 words of meta:
// meta = {x0, y0, z0, x1, y1, z1 (inclusive bounding box of the marked cells), -, -}
constexpr uint32_t kFineCacheCells = 4096;  // LDS budget for the fine-bit cache: 32 KiB
// meta[6] = 1: the cull-grid buffer also carries the PACKED fine-bit image of the marked bounding box (one 64-bit word per 4x4x4 block,
// x fastest) behind the meta record -- built once per occupancy slice, so a marching workgroup fills its LDS cache with a contiguous
// copy instead of a Morton gather with three integer divisions per word.
constexpr uint32_t kCullImageWord = kCullWords + 8;   // uint32 offset of the image (16-byte aligned)
__device__ __forceinline__ uint32_t m2(uint32_t v) { return (v & 1u) | ((v & 2u) << 2); }  // 2-bit Morton spread
__device__ __forceinline__ bool cull_marked(const uint32_t *cull_bits, int cx, int cy, int cz) {
    const uint32_t c = ((uint32_t)cz * kCullRes + (uint32_t)cy) * kCullRes + (uint32_t)cx;
    return (cull_bits[c >> 5] >> (c & 31u)) & 1u;
}

// FAST = (cascade == 1, bound == 1, H a power of two <= 256): the configuration dnerf runs (bound 1, grid 128).
// Then the mip level is always 0 and every scaling in the index / voxel-edge arithmetic is by a power of two, i.e.
// exact, so the float-only forms below produce the same bits as the reference's double / multi-step expressions.
template <bool FAST>
struct MarcherT {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
    float rH, H3, Hf, Cf, Hm1;
    float bound, dt_gamma, dt_min, dt_max;
    float halfH, twoRH, ex, ey, ez;  // FAST only
    float dt_const;                  // step when dt_gamma == 0 (clamp(t * 0, dt_min, dt_max) for every finite t)
    bool dt_is_const;
    double Hd;
    const uint8_t *__restrict__ grid;
    // FAST only: LDS copy of the fine bits of the cull grid's bounding box (one 64-bit word = one 4x4x4 voxel block)
    const unsigned long long *fine = nullptr;
    int fx0 = 0, fy0 = 0, fz0 = 0, fnx = 0, fny = 0, fnz = 0;

    __device__ __forceinline__ void init(const float *o, const float *d, float bound_, float dt_gamma_,
                                         uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t *grid_) {
        ox = o[0]; oy = o[1]; oz = o[2];
        dx = d[0]; dy = d[1]; dz = d[2];
        rdx = 1 / dx; rdy = 1 / dy; rdz = 1 / dz;
        rH = 1 / (float)H;
        H3 = (float)(H * H * H);
        Hf = (float)H; Hd = (double)H; Cf = (float)C; Hm1 = (float)(H - 1);
        bound = bound_; dt_gamma = dt_gamma_;
        dt_min = 2 * kSqrt3 / (float)max_steps;
        dt_max = 2 * kSqrt3 * (float)(1 << (C - 1)) / (float)H;
        dt_is_const = (dt_gamma_ == 0.0f);
        dt_const = clampf_(0.0f, dt_min, dt_max);
        grid = grid_;
        halfH = 0.5f * Hf; twoRH = 2.0f * rH;
        // nx + 0.5f + 0.5f * signf(d) == nx + (signbit(d) ? 0 : 1), exactly
        ex = signbit(dx) ? 0.0f : 1.0f; ey = signbit(dy) ? 0.0f : 1.0f; ez = signbit(dz) ? 0.0f : 1.0f;
    }

    __device__ __forceinline__ float step_size(float t) const { return dt_is_const ? dt_const : clampf_(t * dt_gamma, dt_min, dt_max); }

    // ---- the pieces of one FAST loop-body evaluation (shared by the sequential chain below and certified_jump) ----
    // position and voxel of the parameter t (raymarching.cu:752-768 with the exact float forms of the FAST configuration)
    __device__ __forceinline__ void locate(float t, float &x, float &y, float &z, int &nx, int &ny, int &nz) const {
        x = clampf_(ox + t * dx, -bound, bound);
        y = clampf_(oy + t * dy, -bound, bound);
        z = clampf_(oz + t * dz, -bound, bound);
        nx = (int)clampf_((x + 1) * halfH, 0.0f, Hm1);
        ny = (int)clampf_((y + 1) * halfH, 0.0f, Hm1);
        nz = (int)clampf_((z + 1) * halfH, 0.0f, Hm1);
    }
    // occupancy bit of a voxel (raymarching.cu:770-772)
    __device__ __forceinline__ bool occupied(int nx, int ny, int nz, const uint32_t *cull_bits) const {
        bool occ = false;
        if (fine) {
            // The LDS image holds the fine bits of every 4x4x4 block inside the bounding box of the marked cull cells, and
            // every occupied voxel lies in a marked cell: one LDS read answers the probe inside the box (a block of an unmarked
            // cell reads as zero), three register compares answer it outside.  bit = Morton code of the low two bits per axis.
            const int bx = (nx >> 2) - fx0, by = (ny >> 2) - fy0, bz = (nz >> 2) - fz0;
            if ((uint32_t)bx < (uint32_t)fnx && (uint32_t)by < (uint32_t)fny && (uint32_t)bz < (uint32_t)fnz) {
                const uint32_t b = m2((uint32_t)nx & 3u) | (m2((uint32_t)ny & 3u) << 1) | (m2((uint32_t)nz & 3u) << 2);
                // (24-bit multiplies: full-rate v_mad_u32_u24 instead of quarter-rate v_mul_lo_u32; all factors < 32)
                occ = (fine[__umul24(__umul24((uint32_t)bz, (uint32_t)fny) + (uint32_t)by, (uint32_t)fnx) + (uint32_t)bx] >> b) & 1ull;
            }
        } else if (!cull_bits || cull_marked(cull_bits, nx >> 2, ny >> 2, nz >> 2)) {
            // an unmarked cull cell holds no occupied voxel: the fine bit (a dependent L2 load) is only fetched near the object
            const uint32_t index = morton3D_8bit((uint32_t)nx, (uint32_t)ny, (uint32_t)nz);
            occ = grid[index >> 3] & (1u << (index & 7u));
        }
        return occ;
    }
    // parameter at which the ray leaves the voxel, evaluated at t (raymarching.cu:786-791)
    __device__ __forceinline__ float exit_t(float t, float x, float y, float z, int nx, int ny, int nz) const {
        const float tx = ((((float)nx + ex) * twoRH - 1) - x) * rdx;
        const float ty = ((((float)ny + ey) * twoRH - 1) - y) * rdy;
        const float tz = ((((float)nz + ez) * twoRH - 1) - z) * rdz;
        return t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
    }

    // One loop-body evaluation at parameter t.  Occupied: returns true with the sample in
    // (x,y,z,dt), t untouched.  Empty: returns false with t advanced past the voxel.
    __device__ __forceinline__ bool probe(float &t, float &x, float &y, float &z, float &dt, const uint32_t *cull_bits = nullptr) const {
        if constexpr (FAST) {
            int nx, ny, nz;
            locate(t, x, y, z, nx, ny, nz);
            dt = step_size(t);
            if (occupied(nx, ny, nz, cull_bits)) return true;
            const float tt = exit_t(t, x, y, z, nx, ny, nz);
            if (dt_is_const) {
                // `do t += dt while (t < tt)` with the same additions in the same order, without a divergent loop: one 128^3 voxel is
                // crossed in at most 8 steps of dt_min = 2 sqrt(3) / 1024; anything longer falls through to the loop
                const float d = dt_const;
                t += d;
                #pragma unroll
                for (int k = 0; k < 8; k++) t = (t < tt) ? t + d : t;
                while (t < tt) t += d;
            } else {
                do {
                    t += step_size(t);
                } while (t < tt);
            }
            return false;
        } else {
            x = clampf_(ox + t * dx, -bound, bound);
            y = clampf_(oy + t * dy, -bound, bound);
            z = clampf_(oz + t * dz, -bound, bound);
            dt = step_size(t);
            const int l0 = mip_from_pos(x, y, z, Cf), l1 = mip_from_dt(dt, Hf, Cf);
            const int level = l0 > l1 ? l0 : l1;
            const float mip_bound = fminf(scalbnf(1.0f, level), bound);
            const float mip_rbound = 1 / mip_bound;
            // `0.5 * (...) * H` is a double expression in the reference (0.5 is a double literal)
            const int nx = (int)clampf_((float)(0.5 * (double)(x * mip_rbound + 1) * Hd), 0.0f, Hm1);
            const int ny = (int)clampf_((float)(0.5 * (double)(y * mip_rbound + 1) * Hd), 0.0f, Hm1);
            const int nz = (int)clampf_((float)(0.5 * (double)(z * mip_rbound + 1) * Hd), 0.0f, Hm1);
            const uint32_t index = (uint32_t)((float)level * H3 + (float)morton3D_((uint32_t)nx, (uint32_t)ny, (uint32_t)nz));
            const bool occ = grid[index >> 3] & (1u << (index & 7u));
            if (occ) return true;
            const float tx = (((nx + 0.5f + 0.5f * signf_(dx)) * rH * 2 - 1) * mip_bound - x) * rdx;
            const float ty = (((ny + 0.5f + 0.5f * signf_(dy)) * rH * 2 - 1) * mip_bound - y) * rdy;
            const float tz = (((nz + 0.5f + 0.5f * signf_(dz)) * rH * 2 - 1) * mip_bound - z) * rdz;
            const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
            do {
                t += step_size(t);
            } while (t < tt);
            return false;
        }
    }
};
using Marcher = MarcherT<false>;

static inline bool fast_config(float bound, uint32_t C, uint32_t H) {
    return C == 1 && bound == 1.0f && H >= 2 && H <= 256 && (H & (H - 1)) == 0;
}

// ---------------------------------------------------------------------------
// Exact early-out for rays that cannot produce a sample ("cull grid").
// cull[32^3] (x fastest) marks coarse cells (4^3 fine voxels of the 128^3 grid) whose 3x3x3 coarse neighbourhood
// holds any occupied voxel.  A ray whose remaining segment [t, far], tested every cell width, only sees unmarked
// cells stays >= half a coarse cell (2 fine voxels) away from every occupied voxel, so the reference's marcher --
// whose probe points lie on that segment up to float rounding -- emits nothing for it: returning "no samples"
// is exact, not an approximation.  Rays that may hit take the full reference chain from their own t.
// ---------------------------------------------------------------------------

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

// The range of the cull scan: ds, the parameter step of one cull cell along the ray, and the part [s0, s1] of [t, far] to scan.  Marked
// cells only exist inside their bounding box (origin b*0, extent bn*, in cull cells): only the part of [t, far] that can be inside it is
// scanned (slab test, widened by one scan step against rounding), not the whole chord of the unit cube.  may == false: the ray meets
// no marked cell (nothing is marked, or the segment misses the box).
struct CullRange { bool may; float s0, s1, ds; };
__device__ __forceinline__ CullRange cull_scan_range(float ox, float oy, float oz, float dx, float dy, float dz, float t, float far,
                                                     int bx0, int by0, int bz0, int bnx, int bny, int bnz) {
    CullRange r;
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    r.ds = (2.0f / kCullRes) / fmaxf(len, 1e-12f);
    r.s0 = t; r.s1 = far;
    r.may = !(bnx <= 0 || bny <= 0 || bnz <= 0);              // nothing is marked: nothing is occupied
    if (r.may) {
        const float cw = 2.0f / kCullRes;
        const float lo[3] = {(float)bx0 * cw - 1.0f, (float)by0 * cw - 1.0f, (float)bz0 * cw - 1.0f};
        const float hi[3] = {(float)(bx0 + bnx) * cw - 1.0f, (float)(by0 + bny) * cw - 1.0f, (float)(bz0 + bnz) * cw - 1.0f};
        const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
        #pragma unroll
        for (int a = 0; a < 3; a++) {
            if (d[a] != 0.0f) {
                const float q = 1.0f / d[a];
                const float ta = (lo[a] - o[a]) * q, tb = (hi[a] - o[a]) * q;
                r.s0 = fmaxf(r.s0, fminf(ta, tb) - r.ds);
                r.s1 = fminf(r.s1, fmaxf(ta, tb) + r.ds);
            } else if (o[a] < lo[a] - cw || o[a] > hi[a] + cw) {
                r.may = false;                                 // parallel to the slab and outside it
            }
        }
        if (!(r.s0 <= r.s1)) r.may = false;
    }
    return r;
}

// Scans the remaining segment [t, far] once per cull-cell width.  Returns false if no marked cell is met (the ray
// cannot produce a sample).  Otherwise t_end receives a parameter beyond which no marked cell is met any more: the
// marcher may stop there -- the reference would only step through empty voxels from there to `far`.
// t_safe (optional): a parameter up to which the ray certainly stays >= 2 fine voxels away from every occupied voxel -- the scan
// position one cell width before the first marked one (-FLT_MAX when unknown): certified_jump starts the march shortly before it.
__device__ __forceinline__ bool ray_may_hit(const uint32_t *cull_bits, float ox, float oy, float oz, float dx, float dy, float dz,
                                            float t, float far, float &t_end, int bx0, int by0, int bz0, int bnx, int bny, int bnz,
                                            float *t_safe = nullptr) {
    if (t_safe) *t_safe = -__FLT_MAX__;
    t_end = far;
    const CullRange r = cull_scan_range(ox, oy, oz, dx, dy, dz, t, far, bx0, by0, bz0, bnx, bny, bnz);
    if (!r.may) return false;
    const float ds = r.ds, s1 = r.s1;
    float s = r.s0;
    bool hit = false;
    // bounded: a unit-cube diagonal is 2*sqrt(3) / (2/32) = 56 cells; anything longer (degenerate direction, huge far)
    // falls through to "may hit, no early end" and takes the ordinary marcher
    for (int it = 0; it < 96; it++, s += ds) {
        const float ss = fminf(s, s1);
        const float x = clampf_(ox + ss * dx, -1.0f, 1.0f), y = clampf_(oy + ss * dy, -1.0f, 1.0f), z = clampf_(oz + ss * dz, -1.0f, 1.0f);
        const int cx = (int)fminf((x + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
        const int cy = (int)fminf((y + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
        const int cz = (int)fminf((z + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
        if (cull_marked(cull_bits, cx, cy, cz)) {
            if (!hit && t_safe) *t_safe = ss - ds;
            hit = true; t_end = ss + ds;
        }
        if (s >= s1) return hit;
    }
    t_end = far;
    if (t_safe) *t_safe = -__FLT_MAX__;
    return true;
}

// LDS-resident occupancy caches of the marching kernels (FAST configuration with a cull grid only)
struct OccCache {
    const uint32_t *s_cull = nullptr;            // 32^3 mark bits
    const unsigned long long *fine = nullptr;    // fine bits of the marked bounding box (one word = 4x4x4 voxels)
    int fx0 = 0, fy0 = 0, fz0 = 0, fnx = 0, fny = 0, fnz = 0;   // bounding box of the marked cull cells (origin, extent)
};

// Cooperative load by a 256-thread workgroup; contains a barrier, so every thread of the workgroup must call it.
template <bool FAST>
__device__ __forceinline__ void occ_cache_load(const uint32_t *__restrict__ cull, const uint8_t *__restrict__ grid, uint4 *s_cull4,
                                               unsigned long long *s_fine, OccCache &oc) {
    if constexpr (FAST) {
        if (cull) {  // kernel-uniform
            s_cull4[threadIdx.x] = reinterpret_cast<const uint4 *>(cull)[threadIdx.x];
            const int *meta = reinterpret_cast<const int *>(cull + kCullWords);
            oc.fx0 = meta[0]; oc.fy0 = meta[1]; oc.fz0 = meta[2];
            oc.fnx = meta[3] - oc.fx0 + 1; oc.fny = meta[4] - oc.fy0 + 1;
            const int fnz = meta[5] - oc.fz0 + 1;
            oc.fnz = fnz;
            if (oc.fnx > 0 && oc.fny > 0 && fnz > 0 && (uint32_t)(oc.fnx * oc.fny * fnz) <= kFineCacheCells && meta[6] == 1) {
                const int pairs = (oc.fnx * oc.fny * fnz + 1) / 2;        // contiguous copy, 16 bytes per lane
                const uint4 *__restrict__ img = reinterpret_cast<const uint4 *>(cull + kCullImageWord);
                for (int i = (int)threadIdx.x; i < pairs; i += 256) reinterpret_cast<uint4 *>(s_fine)[i] = img[i];
                oc.fine = s_fine;
            } else if (oc.fnx > 0 && oc.fny > 0 && fnz > 0 && (uint32_t)(oc.fnx * oc.fny * fnz) <= kFineCacheCells) {
                const unsigned long long *__restrict__ blocks = reinterpret_cast<const unsigned long long *>(grid);
                const int cells = oc.fnx * oc.fny * fnz;
                for (int i = (int)threadIdx.x; i < cells; i += 256) {
                    const int cx = oc.fx0 + i % oc.fnx, cy = oc.fy0 + (i / oc.fnx) % oc.fny, cz = oc.fz0 + i / (oc.fnx * oc.fny);
                    s_fine[i] = blocks[morton3D_8bit((uint32_t)cx, (uint32_t)cy, (uint32_t)cz)];
                }
                oc.fine = s_fine;
            }
            __syncthreads();
            oc.s_cull = reinterpret_cast<const uint32_t *>(s_cull4);
        }
    }
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

// ---------------------------------------------------------------------------
// training march: count pass -> deterministic exclusive scan -> write pass
// (raymarching.cu:312-480; the reference allocates slots with two racing atomicAdds)
// ---------------------------------------------------------------------------
constexpr uint32_t kScanBlock = 1024;

template <bool FAST>
__global__ void __launch_bounds__(256) k_march_train_count(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                           const uint8_t *__restrict__ grid, float bound, float dt_gamma,
                                                           uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                                                           const float *__restrict__ nears, const float *__restrict__ fars,
                                                           const float *__restrict__ noises, uint32_t *__restrict__ num_steps_out,
                                                           const uint32_t *__restrict__ cull, float *__restrict__ sample_t) {
    // The one marching pass of a training step: counts every ray's samples AND records their parameters t (sample_t
    // [N, max_steps]), from which the emit pass rebuilds positions and deltas with the marcher's own expressions -- the reference
    // (and the first version of this file) marches every ray a second time to write them.  Same LDS occupancy caches and exact
    // cull-grid early-out as the inference marcher: most rays of a training batch miss the object and stop here at once.
    __shared__ uint4 s_cull4[FAST ? 256 : 1];
    __shared__ unsigned long long s_fine[FAST ? kFineCacheCells : 1];
    OccCache oc;
    occ_cache_load<FAST>(cull, grid, s_cull4, s_fine, oc);
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    MarcherT<FAST> m;
    m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, dt_gamma, max_steps, C, H, grid);
    m.fine = oc.fine; m.fx0 = oc.fx0; m.fy0 = oc.fy0; m.fz0 = oc.fz0; m.fnx = oc.fnx; m.fny = oc.fny; m.fnz = oc.fnz;
    const float far = fars[n];
    float t = nears[n];
    t += m.step_size(t) * noises[n];
    uint32_t num_steps = 0;
    float x, y, z, dt;
    bool go = t < far;
    float t_end = far;
    if (FAST && oc.s_cull && go)
        go = ray_may_hit(oc.s_cull, m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t, far, t_end, oc.fx0, oc.fy0, oc.fz0, oc.fnx, oc.fny, oc.fnz);
    float *ts = sample_t + (size_t)n * max_steps;
    while (go && t < far && t < t_end && num_steps < max_steps) {
        if (m.probe(t, x, y, z, dt, oc.s_cull)) {
            ts[num_steps] = t;
            num_steps++;
            t += dt;
        }
    }
    num_steps_out[n] = num_steps;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Wave-per-ray form of the counting pass (FAST configuration with a constant step, i.e. dt_gamma == 0: what dnerf runs).
//
// With a constant step every parameter the marcher ever visits is a point of ONE lattice  L_0 = t_start, L_{k+1} = fl(L_k + dt):
// a sample advances by dt, and an empty voxel is left by `do t += dt while (t < tt)` -- the same additions.  Which lattice points
// are VISITED is a chain: next(k) = k + 1 if L_k lies in an occupied voxel, else the first m > k with L_m >= tt_k (tt_k: the voxel's
// exit parameter, from L_k alone).  So 64 lanes take 64 consecutive lattice points, evaluate occupancy / exit parameter in
// parallel with the sequential marcher's own expressions, and the wave walks the chain over ballots (scalar work, one readlane
// per empty voxel).  Visited set, samples, counts and the recorded parameters are the sequential kernel's bit for bit: nothing
// is approximated, the dependent chain of ~1000 cycles per voxel probe just becomes one probe round per 64 lattice points.
// One ray per wave instead of one per lane: 4096 rays fill the chip (4 waves per SIMD) where the lane-per-ray kernel kept 64
// waves busy for as long as its longest ray.  Occupancy bits and cull marks are read from global memory (L2-resident, 256 KiB +
// 4 KiB): a probe round is one parallel load, an LDS image per 4-ray workgroup would cost more than it saves.
// ---------------------------------------------------------------------------------------------------------------------------
// The closed form of the lattice L_0 = t, L_(k+1) = fl(L_k + dt).  While L stays in one binade every L_k is a multiple of the binade's
// ulp U, so fl(L_k + dt) = L_k + c with the SAME c = round(dt / U) U for every k -- unless dt / U sits exactly between two integers (a tie
// rounds to even, which depends on L_k).  Then L_k = t + k c exactly (k c and the sum are multiples of U below 2^24 U).  Returns whether
// that holds at t, with the step c and t's biased exponent eb (which must be below eb_ceiling); staying inside the binade for as many
// steps as it looks at is the caller's to check.
__device__ __forceinline__ bool lattice_closed_form(float t, float dt, uint32_t eb_ceiling, float &c, uint32_t &eb) {
    const float first = t + dt;
    c = first - t;                                                  // exact (Sterbenz-like: both multiples of U, |c| << t)
    const float err = dt - c;                                       // rounding error of t + dt (FastTwoSum, exact for t >= dt)
    eb = __float_as_uint(t) >> 23;                                  // sign bit clear: t > 0
    const bool normal = t >= dt && dt > 0.0f && eb > 30u && eb < eb_ceiling;
    const float half_ulp = __uint_as_float((eb - 24u) << 23), c_cap = __uint_as_float((eb - 5u) << 23);   // U / 2, 2^18 U
    return normal && fabsf(err) != half_ulp && c < c_cap;
}

__device__ __forceinline__ float lane_lattice(float base, float dt, uint32_t lane, float &next_base, float &closed_step) {
    // L_{lane} of the lattice starting at base, by `lane` successive additions (float addition is not associative: the values
    // must come from the recurrence); also returns L_64.
    // Closed form for the common case (lattice_closed_form, and no binade crossing inside the window).  All conditions are
    // wave-uniform; anything else (binade crossing inside the window, a tie, a tiny base) takes the recurrence.
    {
        float c;
        uint32_t eb;
        const bool closed = lattice_closed_form(base, dt, 255u, c, eb);
        const float last = base + 64.0f * c;
        if (closed && eb == (__float_as_uint(last) >> 23)) {
            next_base = last;
            closed_step = c;                                        // L_k = base + k c holds for k = 0 .. 64
            return base + (float)lane * c;
        }
    }
    closed_step = 0.0f;
    float v = base, mine = base;
    #pragma unroll 8
    for (uint32_t i = 0; i < 64; i++) {
        if (i == lane) mine = v;
        v += dt;
    }
    next_base = v;
    return mine;
}

__global__ void __launch_bounds__(256) k_march_train_count_wave(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                                const uint8_t *__restrict__ grid, float bound, uint32_t max_steps, uint32_t N,
                                                                uint32_t H, const float *__restrict__ nears, const float *__restrict__ fars,
                                                                const float *__restrict__ noises, uint32_t *__restrict__ num_steps_out,
                                                                const uint32_t *__restrict__ cull, float *__restrict__ sample_t) {
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (n >= N) return;   // wave-uniform
    MarcherT<true> m;
    m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, 0.0f, max_steps, 1u, H, grid);
    const float far = fars[n], dt = m.dt_const;
    float t0 = nears[n];
    t0 += m.step_size(t0) * noises[n];
    bool go = t0 < far;
    float t_end = far;
    if (cull && go) {
        // ray_may_hit with the scan positions spread over the lanes (same positions: s_i by i successive additions of ds)
        const int *meta = reinterpret_cast<const int *>(cull + kCullWords);
        const int bx0 = meta[0], by0 = meta[1], bz0 = meta[2];
        const int bnx = meta[3] - bx0 + 1, bny = meta[4] - by0 + 1, bnz = meta[5] - bz0 + 1;
        const CullRange r = cull_scan_range(m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t0, far, bx0, by0, bz0, bnx, bny, bnz);
        const float ds = r.ds, s1 = r.s1;
        if (!r.may) {
            go = false;
        } else {
            bool hit = false, ended = false;
            float base = r.s0;
            for (int round = 0; round < 2 && !ended; round++) {   // 96 scan positions: lanes 0..63, then 0..31
                float nb, unused_step;
                const float s = lane_lattice(base, ds, lane, nb, unused_step);
                base = nb;
                const bool in_range = round == 0 || lane < 32u;
                const float ss = fminf(s, s1);
                const float x = clampf_(m.ox + ss * m.dx, -1.0f, 1.0f), y = clampf_(m.oy + ss * m.dy, -1.0f, 1.0f), z = clampf_(m.oz + ss * m.dz, -1.0f, 1.0f);
                const int cx = (int)fminf((x + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
                const int cy = (int)fminf((y + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
                const int cz = (int)fminf((z + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
                const bool marked = in_range && cull_marked(cull, cx, cy, cz);
                // the sequential scan stops after the first position with s >= s1 (that position is still tested)
                const unsigned long long stop = __ballot(in_range && s >= s1);
                const uint32_t last = stop ? (uint32_t)__builtin_ctzll(stop) : (round == 0 ? 63u : 31u);
                const unsigned long long mk = __ballot(marked && lane <= last);
                if (mk) {
                    hit = true;
                    const uint32_t top = 63u - (uint32_t)__builtin_clzll(mk);
                    t_end = __shfl(ss + ds, (int)top, 64);
                }
                if (stop) ended = true;
            }
            if (!ended) { t_end = far; hit = true; }   // longer than 96 cells: "may hit, no early end"
            go = hit;
        }
    }
    uint32_t num_steps = 0;
    float *ts = sample_t + (size_t)n * max_steps;
    float base = t0;
    float carry_tt = -__FLT_MAX__;      // exit parameter of an empty voxel whose successor lies beyond the previous window
    // One window = 64 consecutive lattice points, one per lane.  A window's occupancy bytes are loaded while the window BEFORE it is
    // walked (the lattice does not depend on the walk), and for every lattice point, marked by the cull grid or not: the two
    // dependent loads per window of the first version (cull word, then occupancy byte: two L2 round trips with nothing to hide them
    // but three sibling waves doing the same) were the kernel's time.  An unmarked cull cell has no occupied voxel, so reading the
    // voxel's own bit gives the same answer.
    struct Window { float t, nb, cstep, x, y, z; int nx, ny, nz; uint32_t byte, bit; bool act; };
    auto fetch = [&](float from) __attribute__((always_inline)) {
        Window w;
        w.t = lane_lattice(from, dt, lane, w.nb, w.cstep);
        w.act = w.t < far && w.t < t_end;           // the loop condition of the sequential marcher at this lattice point
        // occupancy and (for an empty voxel) the exit parameter, with MarcherT<true>::probe's expressions
        w.x = clampf_(m.ox + w.t * m.dx, -bound, bound); w.y = clampf_(m.oy + w.t * m.dy, -bound, bound); w.z = clampf_(m.oz + w.t * m.dz, -bound, bound);
        w.nx = (int)clampf_((w.x + 1) * m.halfH, 0.0f, m.Hm1); w.ny = (int)clampf_((w.y + 1) * m.halfH, 0.0f, m.Hm1);
        w.nz = (int)clampf_((w.z + 1) * m.halfH, 0.0f, m.Hm1);
        const uint32_t index = morton3D_8bit((uint32_t)w.nx, (uint32_t)w.ny, (uint32_t)w.nz);
        w.byte = grid[index >> 3];                  // positions are clamped: a valid address for every lattice point
        w.bit = index & 7u;
        return w;
    };
    Window cur_w{};
    if (go) cur_w = fetch(base);
    while (go && num_steps < max_steps) {
        const Window nxt_w = fetch(cur_w.nb);
        const float t = cur_w.t, nb = cur_w.nb, cstep = cur_w.cstep, x = cur_w.x, y = cur_w.y, z = cur_w.z;
        const int nx = cur_w.nx, ny = cur_w.ny, nz = cur_w.nz;
        const bool act = cur_w.act;
        const bool occ = act && ((cur_w.byte >> cur_w.bit) & 1u);
        const float tx = ((((float)nx + m.ex) * m.twoRH - 1) - x) * m.rdx;
        const float ty = ((((float)ny + m.ey) * m.twoRH - 1) - y) * m.rdy;
        const float tz = ((((float)nz + m.ez) * m.twoRH - 1) - z) * m.rdz;
        const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
        const unsigned long long occ_m = __ballot(act && occ), act_m = __ballot(act);
        // successor of an empty lane inside this window: the first later lattice point >= tt (at least one step), else 64
        // (a 128^3 voxel is crossed in at most 8 steps of dt_min; longer crossings walk on)
        uint32_t nxt = lane + 1u;
        const bool empty = act && !occ;
        if (cstep > 0.0f) {
            // closed-form window (wave-uniform): the lattice values are base + j cstep exactly, so the successor is an index
            // computation per lane -- an estimate by division, then exact comparisons against the lattice values themselves
            if (empty) {
                const float q = (tt - base) / cstep;
                int j = q < 64.0f ? (int)ceilf(q) : 64;
                if (j < (int)lane + 1) j = (int)lane + 1;
                while (j > (int)lane + 1 && base + (float)(j - 1) * cstep >= tt) j--;
                while (j < 64 && base + (float)j * cstep < tt) j++;
                nxt = (uint32_t)j;
            }
        } else {
            for (int k = 0; k < 64; k++) {
                const float lv = __shfl(t, (int)(nxt & 63u), 64);
                const bool more = empty && nxt < 64u && lv < tt;
                if (!__any(more)) break;
                if (more) nxt++;
            }
        }
        // entry point of the chain into this window
        uint32_t cur0 = 0;
        float new_carry = -__FLT_MAX__;
        if (carry_tt != -__FLT_MAX__) {
            const unsigned long long ge = __ballot(t >= carry_tt);
            cur0 = ge ? (uint32_t)__builtin_ctzll(ge) : 64u;
            if (!ge) new_carry = carry_tt;      // the voxel's exit lies beyond this window too: keep walking
        }
        // The walk itself is a SCALAR loop: position, masks, budget and the emitted set live in SGPRs (pinned with readfirstlane --
        // the compiler's uniformity analysis does not see through the loop-carried values and otherwise runs the loop as divergent
        // vector code under exec masks: measured 440 cycles per hop, 55 000 of a long ray's 81 000 cycles).
        uint32_t cur = __builtin_amdgcn_readfirstlane(cur0);
        uint32_t budget = __builtin_amdgcn_readfirstlane(max_steps - num_steps);
        uint32_t emit_lo = 0, emit_hi = 0;
        bool done = false;
        while (cur < 64u) {
            const unsigned long long am = act_m >> cur, om = occ_m >> cur;
            if (!(am & 1ull)) { done = true; break; }                      // t >= far or t >= t_end: the ray is finished
            if (om & 1ull) {
                // a run of occupied lattice points: every one is visited and sampled
                const unsigned long long rest = ~om;
                uint32_t run = rest ? (uint32_t)__builtin_ctzll(rest) : 64u - cur;
                if (run > 64u - cur) run = 64u - cur;
                if (run >= budget) { run = budget; done = true; }
                const unsigned long long bits = ((run >= 64u) ? ~0ull : ((1ull << run) - 1ull)) << cur;
                emit_lo = __builtin_amdgcn_readfirstlane(emit_lo | (uint32_t)bits);
                emit_hi = __builtin_amdgcn_readfirstlane(emit_hi | (uint32_t)(bits >> 32));
                budget = __builtin_amdgcn_readfirstlane(budget - run);
                cur = __builtin_amdgcn_readfirstlane(cur + run);
                if (done) break;
            } else {
                // (v_readlane with a scalar lane index, not an LDS-latency ds_bpermute)
                const uint32_t to = (uint32_t)__builtin_amdgcn_readlane((int)nxt, (int)cur);
                if (to >= 64u) new_carry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tt), (int)cur));
                cur = to;
            }
        }
        const unsigned long long emit = ((unsigned long long)emit_hi << 32) | emit_lo;
        if ((emit >> lane) & 1ull) ts[num_steps + (uint32_t)__popcll(emit & ((1ull << lane) - 1ull))] = t;
        num_steps = __builtin_amdgcn_readfirstlane(num_steps + (uint32_t)__popcll(emit));
        if (done) break;
        carry_tt = new_carry;
        base = nb;
        cur_w = nxt_w;
    }
    if (lane == 0) num_steps_out[n] = num_steps;
}

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

// pass A: per-block totals
__global__ void __launch_bounds__(kScanBlock) k_scan_block_totals(const uint32_t *__restrict__ vals, uint32_t N, uint32_t *__restrict__ block_totals) {
    __shared__ uint32_t lds[16];
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t total;
    block_inclusive_scan(i < N ? vals[i] : 0u, lds, total);
    if (threadIdx.x == 0) block_totals[blockIdx.x] = total;
}

// pass B: offsets[i] = exclusive scan (every block re-sums the totals of the blocks before it:
// <= 625 L2-resident words for a full 800x800 frame); writes rays[] and bumps counter[] like
// the reference's atomics would, but in ray order.
__global__ void __launch_bounds__(kScanBlock) k_march_train_offsets(const uint32_t *__restrict__ num_steps, uint32_t N,
                                                                    const uint32_t *__restrict__ block_totals,
                                                                    int32_t *__restrict__ rays, int32_t *__restrict__ counter,
                                                                    uint32_t *__restrict__ base_out) {
    __shared__ uint32_t lds[16];
    __shared__ uint32_t s_prev;
    // sum of previous blocks' totals, cooperatively
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kScanBlock) part += block_totals[b];
    uint32_t prev_total;
    block_inclusive_scan(part, lds, prev_total);
    if (threadIdx.x == 0) s_prev = prev_total;
    __syncthreads();
    const uint32_t base = (uint32_t)counter[0];  // reference semantics: slots start at the counter's current value
    const uint32_t ray_base = (uint32_t)counter[1];
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t v = i < N ? num_steps[i] : 0u;
    uint32_t total;
    const uint32_t incl = block_inclusive_scan(v, lds, total);
    if (i < N) {
        const uint32_t ri = ray_base + i;
        rays[ri * 3] = (int32_t)i;
        rays[ri * 3 + 1] = (int32_t)(base + s_prev + incl - v);
        rays[ri * 3 + 2] = (int32_t)v;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        base_out[0] = base;  // consumed by the write pass; counter itself is bumped by k_march_train_finish
        base_out[1] = s_prev + total;
        base_out[2] = ray_base;
    }
}

// A training batch (N of a few thousand rays) does not need the two-pass scan: ONE workgroup walks the rays in chunks of its size with
// a running carry, writes the ray records and bumps the counters itself (the emit pass takes its bases from base_out) -- three
// launches (block totals, offsets, finish) become one.
__global__ void __launch_bounds__(kScanBlock) k_march_train_offsets_small(const uint32_t *__restrict__ num_steps, uint32_t N, int32_t *__restrict__ rays,
                                                                          int32_t *__restrict__ counter, uint32_t *__restrict__ base_out) {
    __shared__ uint32_t lds[16];
    const uint32_t base = (uint32_t)counter[0], ray_base = (uint32_t)counter[1];
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < N; c0 += kScanBlock) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t v = i < N ? num_steps[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_inclusive_scan(v, lds, total);
        if (i < N) {
            const uint32_t ri = ray_base + i;
            rays[ri * 3] = (int32_t)i;
            rays[ri * 3 + 1] = (int32_t)(base + carry + incl - v);
            rays[ri * 3 + 2] = (int32_t)v;
        }
        carry += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        base_out[0] = base; base_out[1] = carry; base_out[2] = ray_base;
        counter[0] = (int32_t)(base + carry);
        counter[1] = (int32_t)(ray_base + N);
    }
}

__global__ void k_march_train_finish(int32_t *__restrict__ counter, const uint32_t *__restrict__ base_out, uint32_t N) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counter[0] += (int32_t)base_out[1];
        counter[1] += (int32_t)N;
    }
}

// Emit pass: one wave per ray, one lane per sample.  From the recorded t of a sample the marcher's own expressions give its
// position (clamp(o + t d)), its step dt = step_size(t) and the parameter after it, t + dt; delta[1] is the difference of two
// consecutive "after" parameters (the first one against the perturbed start) -- bit for bit what the sequential loop wrote
// (raymarching.cu:427-479), but coalesced and without marching again.
template <bool FAST>
__global__ void __launch_bounds__(256) k_march_train_emit(const float *__restrict__ rays_o, const float *__restrict__ rays_d, float bound,
                                                          float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                                                          const float *__restrict__ nears, const float *__restrict__ noises,
                                                          const int32_t *__restrict__ rays, const uint32_t *__restrict__ bases,
                                                          const float *__restrict__ sample_t, float *__restrict__ xyzs,
                                                          float *__restrict__ dirs, float *__restrict__ deltas) {
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (n >= N) return;
    const uint32_t ray_base = bases[2];              // the ray counter's value before this call (the offsets pass recorded it)
    const uint32_t point_index = (uint32_t)rays[(size_t)(ray_base + n) * 3 + 1];
    const uint32_t num_steps = (uint32_t)rays[(size_t)(ray_base + n) * 3 + 2];
    if (num_steps == 0 || point_index + num_steps > M) return;
    MarcherT<FAST> m;
    m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, dt_gamma, max_steps, C, H, nullptr);
    float t0 = nears[n];
    t0 += m.step_size(t0) * noises[n];
    const float *ts = sample_t + (size_t)n * max_steps;
    for (uint32_t k = lane; k < num_steps; k += 64u) {
        const float t = ts[k];
        const float dt = m.step_size(t);
        const float after = t + dt;
        float last = t0;
        if (k > 0) { const float tp = ts[k - 1]; last = tp + m.step_size(tp); }
        const size_t p = (size_t)point_index + k;
        xyzs[p * 3] = clampf_(m.ox + t * m.dx, -bound, bound);
        xyzs[p * 3 + 1] = clampf_(m.oy + t * m.dy, -bound, bound);
        xyzs[p * 3 + 2] = clampf_(m.oz + t * m.dz, -bound, bound);
        dirs[p * 3] = m.dx; dirs[p * 3 + 1] = m.dy; dirs[p * 3 + 2] = m.dz;
        deltas[p * 2] = dt;
        deltas[p * 2 + 1] = after - last;
    }
}

// raymarching.cu:501-577
__global__ void __launch_bounds__(256) k_composite_train_fwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                             const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                             uint32_t M, uint32_t N, float T_thresh, float *__restrict__ weights_sum,
                                                             float *__restrict__ depth, float *__restrict__ image) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    if (num_steps == 0 || offset + num_steps > M) {
        weights_sum[index] = 0; depth[index] = 0;
        image[(size_t)index * 3] = 0; image[(size_t)index * 3 + 1] = 0; image[(size_t)index * 3 + 2] = 0;
        return;
    }
    const float *s = sigmas + offset, *c = rgbs + (size_t)offset * 3, *dl = deltas + (size_t)offset * 2;
    uint32_t step = 0;
    float T = 1.0f, r = 0, g = 0, b = 0, ws = 0, t = 0, d = 0;
    while (step < num_steps) {
        const float alpha = 1.0f - sdn_exp_cr(-s[0] * dl[0]);
        const float weight = alpha * T;
        r += weight * c[0]; g += weight * c[1]; b += weight * c[2];
        t += dl[1];
        d += weight * t;
        ws += weight;
        T *= 1.0f - alpha;
        if (T < T_thresh) break;
        s++; c += 3; dl += 2; step++;
    }
    weights_sum[index] = ws; depth[index] = d;
    image[(size_t)index * 3] = r; image[(size_t)index * 3 + 1] = g; image[(size_t)index * 3 + 2] = b;
}

// (CompositeAcc / composite_step, one step of the inference compositing recurrence: sdn_common.h -- the one-pass tint's schedule replay
// in seal.hip finds a ray's termination sample with the same code)

// The INFERENCE compositing arithmetic (kernel_composite_rays, raymarching.cu:819-905: transmittance as 1 - weights_sum, the stop
// test on the transmittance IN FRONT of a sample, t running from the ray's near bound) over ALL samples of a ray at once, in the
// (offset, count) layout of march_rays_train.  With a ray's samples listed up front the iteration loop of the inference branch
// (dnerf/renderer.py:333-381) collapses into march -> field -> this kernel: per ray the same additions in the same order, so image and
// weights_sum are those of the loop bit for bit; the loop only exists to stop marching terminated rays early, which pays for a
// frame of 640 000 rays and costs a chain of ~30 dependent launches for a batch of 4 096.
__global__ void __launch_bounds__(256) k_composite_whole_rays(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                              const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                              const float *__restrict__ nears, uint32_t M, uint32_t N, float T_thresh,
                                                              float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    CompositeAcc a = {0, 0, 0, 0, 0, 0};
    if (num_steps != 0 && offset + num_steps <= M) {
        const float *s = sigmas + offset, *c = rgbs + (size_t)offset * 3, *dl = deltas + (size_t)offset * 2;
        a.t = nears[index];
        for (uint32_t step = 0; step < num_steps; step++) {
            if (dl[0] == 0) break;
            if (composite_step(a, s[0], dl[0], dl[1], c[0], c[1], c[2]) < T_thresh) break;
            s++; c += 3; dl += 2;
        }
    }
    weights_sum[index] = a.weight_sum; depth[index] = a.d;
    image[(size_t)index * 3] = a.r; image[(size_t)index * 3 + 1] = a.g; image[(size_t)index * 3 + 2] = a.b;
}

// raymarching.cu:602-682
__global__ void __launch_bounds__(256) k_composite_train_bwd(const float *__restrict__ grad_weights_sum, const float *__restrict__ grad_image,
                                                             const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                             const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                             const float *__restrict__ weights_sum, const float *__restrict__ image,
                                                             uint32_t M, uint32_t N, float T_thresh, float *__restrict__ grad_sigmas,
                                                             float *__restrict__ grad_rgbs) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    if (num_steps == 0 || offset + num_steps > M) return;
    const float gws = grad_weights_sum[index];
    const float gi0 = grad_image[(size_t)index * 3], gi1 = grad_image[(size_t)index * 3 + 1], gi2 = grad_image[(size_t)index * 3 + 2];
    const float r_final = image[(size_t)index * 3], g_final = image[(size_t)index * 3 + 1], b_final = image[(size_t)index * 3 + 2];
    const float ws_final = weights_sum[index];
    const float *s = sigmas + offset, *c = rgbs + (size_t)offset * 3, *dl = deltas + (size_t)offset * 2;
    float *gs = grad_sigmas + offset, *gc = grad_rgbs + (size_t)offset * 3;
    uint32_t step = 0;
    float T = 1.0f, r = 0, g = 0, b = 0;
    while (step < num_steps) {
        const float alpha = 1.0f - sdn_exp_cr(-s[0] * dl[0]);
        const float weight = alpha * T;
        r += weight * c[0]; g += weight * c[1]; b += weight * c[2];
        T *= 1.0f - alpha;
        gc[0] = gi0 * weight; gc[1] = gi1 * weight; gc[2] = gi2 * weight;
        gs[0] = dl[0] * (gi0 * (T * c[0] - (r_final - r)) + gi1 * (T * c[1] - (g_final - g)) +
                         gi2 * (T * c[2] - (b_final - b)) + gws * (1 - ws_final));
        if (T < T_thresh) break;
        s++; c += 3; dl += 2; gs++; gc += 3; step++;
    }
}

// ---------------------------------------------------------------------------
// inference
// ---------------------------------------------------------------------------
// raymarching.cu:701-805.  Extras over the reference kernel (all optional, none changes a sample):
//   * slots [step, n_step) of each alive ray are written as zeros here and the alignment tail [n_alive*n_step, M_pad)
//     is cleared by the same launch, so the caller never memsets the sample buffers;
//   * cull: exact early-out for rays that cannot produce a sample (see ray_may_hit);
//   * live_idx / live_count: the slots that received a sample are appended (one atomicAdd per wave, ballot-free prefix
//     via wave shuffles) to a compact list so that the field network is evaluated on samples, not on padded slots.
// Marches one ray from parameter t for up to n_step samples into its slots (the loop of raymarching.cu:750-804), zero-fills
// the unused slots and returns the number of samples written.
// tend (may be null): this ray's cached cull result.  The bound t_end found by ray_may_hit -- beyond it the ray meets no
// marked cell -- is a property of the ray, not of where the scan started, so the device loop computes it on a ray's first
// march and later iterations only compare (kTendUnset: not computed yet; kTendDead: the ray cannot produce a sample).
constexpr float kTendUnset = -2.0f, kTendDead = -1.0f;
// device loop: the cache's base pointer travels in the loop record (sdn_loop_tend; nullptr = no cache)
template <bool FAST>
__device__ __forceinline__ uint32_t march_ray(MarcherT<FAST> &m, const OccCache &oc, float t, float far, uint32_t n_step, float *px, float *pd,
                                              float *pl, float *tend = nullptr, uint8_t *psf = nullptr, uint32_t frame = 0,
                                              const float *t_begin = nullptr) {
    m.fine = oc.fine; m.fx0 = oc.fx0; m.fy0 = oc.fy0; m.fz0 = oc.fz0; m.fnx = oc.fnx; m.fny = oc.fny; m.fnz = oc.fnz;
    uint32_t step = 0;
    // t_begin: the walk resumes at t, a later point of the chain that started at *t_begin (k_cull_start's certified jump): the first
    // sample's second delta is measured from the chain's start, as the walk from there would have measured it
    float last_t = t_begin ? *t_begin : t, x, y, z, dt;
    bool go = t < far;
    float t_end = far;
    if (FAST && oc.s_cull && go) {
        const float cached = tend ? *tend : kTendUnset;
        if (cached != kTendUnset) {
            t_end = cached;                 // kTendDead (< every t) ends the ray here
            go = t < t_end;
        } else {
            go = ray_may_hit(oc.s_cull, m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t, far, t_end, oc.fx0, oc.fy0, oc.fz0, oc.fnx, oc.fny, oc.fnz);
            if (tend) *tend = go ? t_end : kTendDead;
        }
    }
    if (go) {
        while (t < far && t < t_end && step < n_step) {
            if (m.probe(t, x, y, z, dt, oc.s_cull)) {
                px[0] = x; px[1] = y; px[2] = z;
                pd[0] = m.dx; pd[1] = m.dy; pd[2] = m.dz;
                t += dt;
                pl[0] = dt;
                pl[1] = t - last_t;
                last_t = t;
                px += 3; pd += 3; pl += 2;
                if (psf) psf[step] = (uint8_t)frame;   // frame group: which frame's time constants the field network applies
                step++;
            }
        }
    }
    for (uint32_t k = step; k < n_step; k++) {
        px[0] = 0; px[1] = 0; px[2] = 0;
        pd[0] = 0; pd[1] = 0; pd[2] = 0;
        pl[0] = 0; pl[1] = 0;
        px += 3; pd += 3; pl += 2;
    }
    return step;
}

// ---- frame groups (FrameSel::n_frames > 1) -------------------------------------------------------------------------------------
// The alive list is ordered by ray id (stable compaction; the steady mode's frozen list keeps that order) and rays are
// frame-major, so a 256-entry workgroup sees one frame, or two at a frame boundary.  A marching workgroup therefore loops over the
// frames present among its live entries (ascending; one round in all but the <= n_frames - 1 boundary workgroups of a launch):
// per round it loads the LDS occupancy caches of that frame and the lanes of that frame march.  Same code, same LDS address
// space, no per-lane indexing of the kernel-argument record (fs.grid[] is only ever indexed with a workgroup-uniform value).
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
constexpr uint32_t kNoFrame = 0xFFFFFFFFu;
__device__ __forceinline__ const uint8_t *frame_grid_uniform(const FrameSel &fs, uint32_t frame_uniform) {
    return fs.grid[__builtin_amdgcn_readfirstlane(frame_uniform)];
}

// A marching lane's ray: origin, direction and far bound.  The marching kernels fetch them BEFORE their workgroup's barriers and LDS
// fill, so that the loads land under those instead of behind them.
struct RayIn { float o[3] = {0, 0, 0}, d[3] = {0, 0, 1}, far = 0; };
__device__ __forceinline__ void ray_in_fetch(RayIn &r, int index, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                             const float *__restrict__ fars) {
    r.o[0] = rays_o[(size_t)index * 3]; r.o[1] = rays_o[(size_t)index * 3 + 1]; r.o[2] = rays_o[(size_t)index * 3 + 2];
    r.d[0] = rays_d[(size_t)index * 3]; r.d[1] = rays_d[(size_t)index * 3 + 1]; r.d[2] = rays_d[(size_t)index * 3 + 2];
    r.far = fars[index];
}

// The frame rounds of a marching workgroup (see above): one round per frame present among its marching lanes -- exactly one without a
// frame group -- in which the workgroup loads that frame's LDS occupancy caches and the lanes of that frame call
// march(oc, grid_f, frame, grouped).  Contains barriers: every thread of the workgroup must call it (marches: this lane has a ray to
// march, index: its ray).  s_cull4 / s_fine / s_min4: the kernel's LDS for the caches and the frame minimum.
template <bool FAST, typename March>
__device__ __forceinline__ void frame_rounds(const FrameSel &fs, bool marches, int index, const uint8_t *__restrict__ grid,
                                             const uint32_t *__restrict__ cull, uint4 *s_cull4, unsigned long long *s_fine, uint32_t *s_min4,
                                             March march) {
    const bool grouped = fs.n_frames > 1;  // kernel-uniform
    const uint32_t frame = (grouped && marches) ? (uint32_t)index / fs.rays_per_frame : (grouped ? kNoFrame : 0u);
    uint32_t fcur = grouped ? block_min_256(frame, s_min4) : 0u;
    while (fcur != kNoFrame) {
        const uint8_t *grid_f = grouped ? frame_grid_uniform(fs, fcur) : grid;   // (fcur is workgroup-uniform)
        const uint32_t *cull_f = (grouped && cull) ? cull + (size_t)fcur * fs.cull_stride : cull;
        OccCache oc;
        occ_cache_load<FAST>(cull_f, grid_f, s_cull4, s_fine, oc);
        if (marches && frame == fcur) march(oc, grid_f, frame, grouped);
        if (!grouped) break;
        fcur = block_min_256((frame != kNoFrame && frame > fcur) ? frame : kNoFrame, s_min4);   // (the barriers inside also fence the LDS caches)
    }
}

// Appends the slots n*n_step .. +step of every lane to the live list: one atomicAdd per wave, prefix by wave shuffles.
// Must be called by all 64 lanes of the wave.
__device__ __forceinline__ void live_append(uint32_t step, uint32_t n, uint32_t n_step, uint32_t *__restrict__ live_idx,
                                            uint32_t *__restrict__ live_count) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t incl = step;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += u;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(live_count, total);
    base = __shfl(base, 63, 64);
    const uint32_t dst = base + incl - step;
    for (uint32_t k = 0; k < step; k++) live_idx[dst + k] = n * n_step + k;
}

// Resumes the compositing of one ray over its n_step slots (raymarching.cu:845-904).  Returns true if the ray survives.
// The per-ray state and -- in the n_step == 8 case the loop spends most of its iterations in -- all 8 slots of the ray
// (8 sigmas, 24 colours, 16 deltas: twelve 16-byte loads) are fetched before the serial recurrence starts, so the ray pays one
// memory round trip instead of one per sample (a lane is a ray here and there is at most one wave per SIMD to hide latency
// behind); the arithmetic and its order, including the two early exits, are the reference's.
__device__ __forceinline__ bool composite_ray(int index, uint32_t n_step, float T_thresh, const float *s, const float *c, const float *dl,
                                              float *__restrict__ rays_t, float *__restrict__ weights_sum, float *__restrict__ depth,
                                              float *__restrict__ image, float *t_out = nullptr) {
    CompositeAcc a = {rays_t[index], weights_sum[index], depth[index], image[(size_t)index * 3], image[(size_t)index * 3 + 1],
                      image[(size_t)index * 3 + 2]};
    uint32_t step = 0;
    if (n_step == 8) {
        float sv[8], cv[24], dv[16];
        #pragma unroll
        for (int q = 0; q < 2; q++) *reinterpret_cast<float4 *>(sv + 4 * q) = *reinterpret_cast<const float4 *>(s + 4 * q);
        #pragma unroll
        for (int q = 0; q < 6; q++) *reinterpret_cast<float4 *>(cv + 4 * q) = *reinterpret_cast<const float4 *>(c + 4 * q);
        #pragma unroll
        for (int q = 0; q < 4; q++) *reinterpret_cast<float4 *>(dv + 4 * q) = *reinterpret_cast<const float4 *>(dl + 4 * q);
        bool open = true;   // false once the reference's loop would have left through a break
        #pragma unroll
        for (int k = 0; k < 8; k++) {
            if (open && dv[2 * k] == 0) open = false;
            if (open) {
                if (composite_step(a, sv[k], dv[2 * k], dv[2 * k + 1], cv[3 * k], cv[3 * k + 1], cv[3 * k + 2]) < T_thresh) open = false;
                else step++;
            }
        }
    } else {
        while (step < n_step) {
            if (dl[0] == 0) break;
            if (composite_step(a, s[0], dl[0], dl[1], c[0], c[1], c[2]) < T_thresh) break;
            s++; c += 3; dl += 2; step++;
        }
    }
    const bool survives = !(step < n_step);
    if (survives) rays_t[index] = a.t;
    if (t_out) *t_out = a.t;
    weights_sum[index] = a.weight_sum; depth[index] = a.d;
    image[(size_t)index * 3] = a.r; image[(size_t)index * 3 + 1] = a.g; image[(size_t)index * 3 + 2] = a.b;
    return survives;
}

// raymarching.cu:701-805.  Extras over the reference kernel (all optional, none changes a sample):
//   * slots [step, n_step) of each alive ray are written as zeros here and the alignment tail [n_alive*n_step, M_pad)
//     is cleared by the same launch, so the caller never memsets the sample buffers;
//   * cull: exact early-out for rays that cannot produce a sample (see ray_may_hit), LDS occupancy caches;
//   * live_idx / live_count: the slots that received a sample are appended to a compact list so that the field network is
//     evaluated on samples, not on padded slots.
template <bool FAST>
__global__ void __launch_bounds__(256) k_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive,
                                                    const float *__restrict__ rays_t, const float *__restrict__ rays_o,
                                                    const float *__restrict__ rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                                    uint32_t C, uint32_t H, const uint8_t *__restrict__ grid,
                                                    const float *__restrict__ fars, float *__restrict__ xyzs, float *__restrict__ dirs,
                                                    float *__restrict__ deltas, const float *__restrict__ noises, uint32_t M_pad,
                                                    const uint32_t *__restrict__ cull, uint32_t *__restrict__ live_idx,
                                                    uint32_t *__restrict__ live_count, const int32_t *__restrict__ state,
                                                    const int32_t *__restrict__ rays_alive_b, FrameSel fs, const float *__restrict__ jump) {
    const SdnLoopRecord *rec = sdn_loop(state);
    if (rec) {  // device-driven loop: sizes, ping-pong side and the iteration's live counter come from the loop record
        n_alive = (uint32_t)rec->n_alive;
        n_step = (uint32_t)rec->n_step;
        if (n_alive == 0) return;
        if (rec->side) rays_alive = rays_alive_b;
        live_count += rec->iteration;
        const uint32_t m0 = n_alive * n_step;
        M_pad = m0 + (128u - m0 % 128u);
        if (!(rec->culled_start && rec->iteration == 0)) jump = nullptr;   // the per-ray jump targets of k_cull_start hold for the first march only
        if (rec->iteration != 0) noises = nullptr;   // the loop's noises (SdnRenderCtx::noises) perturb the march of iteration 0 only
        if (blockIdx.x * 256u >= n_alive + 128u) return;   // workgroup-uniform: beyond the list and its alignment tail (the host sizes the grid by a bound)
    }
    __shared__ uint4 s_cull4[FAST ? 256 : 1];  // 32^3 bits = 4 KiB
    __shared__ unsigned long long s_fine[FAST ? kFineCacheCells : 1];  // <= 32 KiB
    __shared__ uint32_t s_min4[4];
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    const int index = n < n_alive ? rays_alive[n] : -1;
    uint32_t step = 0;
    // the ray's inputs are fetched NOW: they land under the workgroup's barriers and its LDS fill instead of behind them
    RayIn ray;
    float t_ray = 0, t_jump = 0, noise = 0;
    if (index >= 0) {
        ray_in_fetch(ray, index, rays_o, rays_d, fars);
        t_ray = rays_t[index];
        if (jump) t_jump = jump[index];
        // drop-in ABI: one offset per list position (the reference's noises[n]); the loop's are per RAY -- iteration 0 of a culled start
        // runs on the compacted list, where position and ray differ (on the reference's arange(N) list they coincide)
        if (noises) noise = noises[rec ? (uint32_t)index : n];
    }
    frame_rounds<FAST>(fs, index >= 0, index, grid, cull, s_cull4, s_fine, s_min4,
                       [&](const OccCache &oc, const uint8_t *grid_f, uint32_t frame, bool grouped) __attribute__((always_inline)) {
        MarcherT<FAST> m;
        m.init(ray.o, ray.d, bound, dt_gamma, max_steps, C, H, grid_f);
        float t = t_ray;
        t += m.step_size(t) * noise;
        float *tend = rec ? sdn_loop_tend(*rec) : nullptr;
        if (tend) tend += index;
        const float t_walk = jump ? t_jump : t;   // (== t where k_cull_start certified no jump)
        step = march_ray<FAST>(m, oc, t_walk, ray.far, n_step, xyzs + (size_t)n * n_step * 3, dirs + (size_t)n * n_step * 3,
                               deltas + (size_t)n * n_step * 2, tend, grouped ? fs.slot_frame + (size_t)n * n_step : nullptr, frame,
                               jump ? &t : nullptr);
    });
    if (n >= n_alive) {
        const uint32_t slot = n_alive * n_step + (n - n_alive);  // spare lanes of the last blocks clear the alignment tail
        if (slot < M_pad) {
            xyzs[(size_t)slot * 3] = 0; xyzs[(size_t)slot * 3 + 1] = 0; xyzs[(size_t)slot * 3 + 2] = 0;
            dirs[(size_t)slot * 3] = 0; dirs[(size_t)slot * 3 + 1] = 0; dirs[(size_t)slot * 3 + 2] = 0;
            deltas[(size_t)slot * 2] = 0; deltas[(size_t)slot * 2 + 1] = 0;
        }
    }
    if (live_idx) live_append(step, n, n_step, live_idx, live_count);  // kernel-uniform condition
}

// raymarching.cu:819-905
__global__ void __launch_bounds__(256) k_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *__restrict__ rays_alive,
                                                        float *__restrict__ rays_t, const float *__restrict__ sigmas,
                                                        const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                                        float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
                                                        const int32_t *__restrict__ state, int32_t *__restrict__ rays_alive_b,
                                                        uint32_t *__restrict__ block_totals) {
    if (state) {
        const SdnLoopRecord &rec = *sdn_loop(state);
        n_alive = sdn_loop_list_len(rec);
        n_step = (uint32_t)rec.n_step;
        if (rec.side) rays_alive = rays_alive_b;
    }
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    bool survives = false;
    if (n < n_alive) {
        const int index = rays_alive[n];
        if (index >= 0) {    // (a frozen list holds dead entries)
            survives = composite_ray(index, n_step, T_thresh, sigmas + (size_t)n * n_step, rgbs + (size_t)n * n_step * 3,
                                     deltas + (size_t)n * n_step * 2, rays_t, weights_sum, depth, image);
            if (!survives) rays_alive[n] = -1;
        }
    }
    if (block_totals) {  // kernel-uniform: survivor count of this 256-ray block, for the fused compaction of the device loop
        __shared__ uint32_t s_cnt[4];
        const uint32_t c = block_count_256(survives, s_cnt);
        if (threadIdx.x == 0) block_totals[blockIdx.x] = c;
    }
}

// ---------------------------------------------------------------------------
// stable compaction of rays_alive >= 0 (replaces the torch mask-select of dnerf/renderer.py:372)
// two launches: per-block survivor counts (wave ballot + popcount), then scatter.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kScanBlock) k_compact_count(const int32_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ block_totals,
                                                              const int32_t *__restrict__ state, const int32_t *__restrict__ in_b) {
    if (state) {
        const SdnLoopRecord &rec = *sdn_loop(state);
        n = sdn_loop_list_len(rec);
        if (rec.side) in = in_b;
        if (blockIdx.x * kScanBlock >= n) return;  // workgroup-uniform
    }
    __shared__ uint32_t lds[16];
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    const bool keep = i < n && in[i] >= 0;
    const unsigned long long mask = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < (kScanBlock >> 6); w++) t += lds[w];
        block_totals[blockIdx.x] = t;
    }
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

__global__ void __launch_bounds__(kScanBlock) k_compact_scatter(const int32_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_totals,
                                                                int32_t *__restrict__ out, int32_t *__restrict__ n_out,
                                                                const int32_t *__restrict__ state, const int32_t *__restrict__ in_b,
                                                                int32_t *__restrict__ out_b, uint32_t totals_per_block) {
    // totals_per_block: block_totals holds one count per (kScanBlock / totals_per_block) entries -- 1: k_compact_count's, 4: the
    // per-256-ray survivor counts k_composite_rays wrote (the device loop skips the count launch)
    uint32_t last_block = gridDim.x - 1;
    if (state) {
        const SdnLoopRecord &rec = *sdn_loop(state);
        n = sdn_loop_list_len(rec);
        if (rec.side) { in = in_b; out = out_b; }
        if (n == 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) n_out[0] = 0;
            return;
        }
        last_block = (n - 1) / kScanBlock;
        if (blockIdx.x > last_block) return;  // workgroup-uniform
    }
    __shared__ uint32_t lds[16];
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x * totals_per_block; b += kScanBlock) part += block_totals[b];
    uint32_t prev;   // survivors of the blocks before this one (the scan hands the block's total to every thread)
    block_inclusive_scan(part, lds, prev);
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t total = ranked_scatter<kScanBlock / 64>(i < n ? in[i] : -1, prev, out, lds);
    if (blockIdx.x == last_block && threadIdx.x == 0) n_out[0] = (int32_t)(prev + total);
}


// ---------------------------------------------------------------------------
// device-driven inference loop (dnerf/renderer.py:340-381 without a host round trip per iteration)
// The loop record `state` is an SdnLoopRecord (include/sdn_hip.h documents every word); kernels view it through sdn_loop().
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_loop_init(uint32_t N, uint32_t max_steps, const float *__restrict__ nears, int32_t *__restrict__ alive_a,
                                                   float *__restrict__ rays_t, float *__restrict__ weights_sum, float *__restrict__ depth,
                                                   float *__restrict__ image, int32_t *__restrict__ state, int32_t *__restrict__ live_counts,
                                                   uint32_t n_counters, unsigned long long mailbox, uint32_t frame_tag,
                                                   float *__restrict__ rays_tend) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n < N) {
        if (rays_tend) rays_tend[n] = kTendUnset;
        alive_a[n] = (int32_t)n;
        rays_t[n] = nears[n];
        weights_sum[n] = 0; depth[n] = 0;
        image[(size_t)n * 3] = 0; image[(size_t)n * 3 + 1] = 0; image[(size_t)n * 3 + 2] = 0;
    }
    if (n < n_counters) live_counts[n] = 0;
    if (n == 0) {
        SdnLoopRecord &rec = *sdn_loop(state);
        rec.n_alive = (int32_t)N; rec.n_step = 1; rec.steps_done = 0; rec.iteration = 0; rec.side = 0;
        rec.N = (int32_t)N; rec.max_steps = (int32_t)max_steps; rec.advance_calls = 0;
        rec.frozen_len = 0; rec.survivors = 0;
        rec.mailbox_lo = (int32_t)(uint32_t)mailbox;
        rec.mailbox_hi = (int32_t)(uint32_t)(mailbox >> 32);
        rec.frame_tag = (int32_t)frame_tag;
        const unsigned long long tp = (unsigned long long)(uintptr_t)rays_tend;
        rec.tend_lo = (int32_t)(uint32_t)tp;
        rec.tend_hi = (int32_t)(uint32_t)(tp >> 32);
        rec.culled_start = 0;
    }
}


// Per-iteration snapshot {alive rays entering the next iteration, index of that iteration}: into the device ring `snap`
// (4 deep, immutable once written: the host may copy it out while the next iteration runs) and, when the frame driver
// registered a mailbox in coherent host memory, as ONE 64-bit system-scope store {tag : n_alive} the host polls for --
// no event, no copy, no stream wait on the critical path.  tag = frame_tag << 16 | (call + 1).
__device__ __forceinline__ void publish_snapshot(const SdnLoopRecord &rec, int32_t *__restrict__ snap, int32_t call) {
    snap[(call & 3) * 2] = rec.n_alive;
    snap[(call & 3) * 2 + 1] = call + 1;
    unsigned long long *mb = sdn_loop_mailbox(rec);
    if (mb) {
        const unsigned long long tag = ((uint32_t)rec.frame_tag << 16) | (uint32_t)(call + 1);
        __hip_atomic_store(mb + (call & 3), (tag << 32) | (uint32_t)rec.n_alive, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Advances the loop record past the iteration that just ran; one thread, after every reader of the record in the launch is done.
// Logs the iteration's {n_alive, n_step} in the trace (only iterations that did work), adds its steps, applies `while step < max_steps`
// and sets the survivors n_new as the next iteration's n_alive; freeze: the steady mode starts with the list as it now stands as
// its frozen list; then publishes the snapshot.
// RECOMPACTED: the survivors were compacted to the other side -- the side flips and n_step = max(min(N // n_alive, 8), 1) is set
// (false: the steady mode, whose frozen list stays where it is and whose n_step stays 8: N / n_new >= 8 holds from its start on).
// CULLED_LOGS_N: after a culled start the trace logs N for iteration 0, the reference's N-ray iteration (SdnLoopRecord::culled_start).
template <bool RECOMPACTED, bool CULLED_LOGS_N>
__device__ __forceinline__ void advance_record(SdnLoopRecord &rec, int32_t *__restrict__ trace, int32_t *__restrict__ snap, int32_t n_new,
                                               int freeze) {
    const int32_t it = rec.iteration;
    const int32_t call = rec.advance_calls;   // no-op iterations included
    rec.advance_calls = call + 1;
    if (rec.n_alive > 0) {
        trace[2 * it] = (CULLED_LOGS_N && it == 0 && rec.culled_start) ? rec.N : rec.n_alive;
        trace[2 * it + 1] = rec.n_step;
        rec.steps_done += rec.n_step;
        rec.iteration = it + 1;
        if (RECOMPACTED) rec.side ^= 1;
        if (rec.steps_done >= rec.max_steps) n_new = 0;
        rec.n_alive = n_new;
        if (RECOMPACTED && n_new > 0) {
            const int32_t ns = rec.N / n_new;
            rec.n_step = ns > 8 ? 8 : (ns < 1 ? 1 : ns);
        }
    }
    if (freeze) { rec.frozen_len = rec.n_alive; rec.survivors = 0; }   // (k_steady_begin folded in)
    publish_snapshot(rec, snap, call);
}

// Last-workgroup election of a launch: every workgroup takes a ticket after its last access to what the last one will touch (the
// caller puts a barrier between those accesses and this call); true in every thread of the workgroup that drew the last ticket,
// which then sees the other workgroups' writes.  The ticket is reset for the next launch HERE, before the caller's last-workgroup work
// (every other workgroup of the launch has drawn its ticket by then).  Must be called by the whole workgroup.
__device__ __forceinline__ bool last_workgroup(int32_t *__restrict__ ticket) {
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = (atomicAdd(ticket, 1) == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    if (threadIdx.x == 0) *ticket = 0;
    return true;
}

// The largest lattice point <= target of the lattice t, fl(t + dt), ... (t itself if none): closed form inside a binade, one
// recurrence step across a binade boundary.  Gives up (returns the point reached) where the closed form does not hold.
__device__ __forceinline__ float lattice_floor(float t, float dt, float target) {
    for (int hop = 0; hop < 4; hop++) {
        if (!(t + dt <= target)) break;
        float c;
        uint32_t eb;
        if (!lattice_closed_form(t, dt, 254u, c, eb)) break;
        const float top = __uint_as_float(((eb + 1u) << 23) - 1u);       // the largest float of t's binade
        const float lim = fminf(target, top);
        float k = floorf((lim - t) / c);
        while (t + (k + 1.0f) * c <= lim) k += 1.0f;                       // (products and sums exact: multiples of U below 2^24 U)
        while (k > 0.0f && t + k * c > lim) k -= 1.0f;
        t = t + k * c;
        if (lim == target) break;
        if (!(t + dt <= target)) break;
        t = t + dt;                                                       // the one step that crosses into the next binade
    }
    return t;
}

// Culled start of the device loop (FAST configuration with a cull grid and the per-ray t_end cache).  The reference's iteration 0 marches
// all N rays by one step and the rays without a sample die in its compositing pass; here the exact cull test every ray would run on
// its first march (ray_may_hit: same arguments, same result, the marks read from global memory instead of an LDS copy) runs up front
// for all N rays -- filling the t_end cache -- and iteration 0 then works on the compacted list of the rays that MAY produce a sample:
// dense waves instead of N-ray launches in which most lanes stop at the cull test.  Nothing observable changes: a ray the test rejects
// produces no sample and dies in iteration 0 either way, the survivors of iteration 0 -- and therefore every later iteration, every
// sample and every count -- are the same, and the trace logs N for iteration 0 (SdnLoopRecord::culled_start, advance_record).
// The certified jump.  With a constant step every parameter the marcher visits is a point of the lattice L_0 = t, L_(k+1) = fl(L_k + dt);
// the walk from t visits, of every voxel that holds lattice points, a first one, and leaves it for the first lattice point >= the
// voxel's exit parameter.  Everything before `t_safe` (ray_may_hit) is >= 2 fine voxels away from any occupied voxel, so the walk emits
// nothing there -- it only matters WHERE it stands when it gets there.  lattice_floor gives a lattice point L well before t_safe
// (bit-exact, or it stops early at one); L lies in some run of consecutive lattice points that `locate` puts into the same voxel.
// If every point q of that run has exit_t(q) <= L_a, the first lattice point behind the run, then the walk, wherever in the run it
// lands (it cannot jump the run: the exit parameter of the voxel before it is at most a rounding error beyond the run's first
// point), can never leave it for a point beyond L_a, and every hop advances: L_a is CERTAINLY visited.  The march may start there.
// Returns t when anything is not provable (binade edge, rounding tie, long run).
__device__ __forceinline__ float certified_jump(const MarcherT<true> &m, float t, float t_safe) {
    const float dt = m.dt_const;
    if (!(t_safe > t + 64.0f * dt)) return t;
    const float L = lattice_floor(t, dt, t_safe - 18.0f * dt);
    if (!(L > t)) return t;
    // closed form of the lattice around L (the conditions of lattice_floor, for the 14 steps either side that are looked at)
    float c;
    uint32_t eb;
    if (!(lattice_closed_form(L, dt, 254u, c, eb) && c > 0.0f)) return t;
    if ((__float_as_uint(L - 14.0f * c) >> 23) != eb || (__float_as_uint(L + 14.0f * c) >> 23) != eb) return t;
    float x, y, z;
    int vx, vy, vz, nx, ny, nz;
    m.locate(L, x, y, z, vx, vy, vz);
    // back to the first lattice point of the run
    float q = L;
    int k = 0;
    for (; k < 12; k++) {
        const float qm = q - c;
        if (!(qm > t) || (qm + dt) != q) return t;
        m.locate(qm, x, y, z, nx, ny, nz);
        if (nx != vx || ny != vy || nz != vz) break;
        q = qm;
    }
    if (k == 12) return t;
    // forward over the whole run: the largest exit parameter any of its points computes, and the first point behind it
    float max_tt = -__FLT_MAX__;
    for (k = 0; k < 26; k++) {
        m.locate(q, x, y, z, nx, ny, nz);
        if (nx != vx || ny != vy || nz != vz) break;
        max_tt = fmaxf(max_tt, m.exit_t(q, x, y, z, nx, ny, nz));
        q = q + dt;                                   // the lattice's own recurrence
    }
    if (k == 26 || !(max_tt <= q) || !(q < t_safe - 4.0f * dt)) return t;
    return q;
}

__device__ __forceinline__ bool cull_start_ray(uint32_t n, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                               const float *__restrict__ nears, const float *__restrict__ fars, const uint32_t *__restrict__ cull,
                                               const FrameSel &fs, int32_t *__restrict__ alive_a, float *__restrict__ rays_tend, float bound,
                                               float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, float *__restrict__ jump,
                                               const float *__restrict__ noises) {
    const uint32_t frame = fs.n_frames > 1 ? n / fs.rays_per_frame : 0u;
    const uint32_t *__restrict__ cull_f = fs.n_frames > 1 ? cull + (size_t)frame * fs.cull_stride : cull;
    const int *meta = reinterpret_cast<const int *>(cull_f + kCullWords);
    const int fx0 = meta[0], fy0 = meta[1], fz0 = meta[2];
    const int fnx = meta[3] - fx0 + 1, fny = meta[4] - fy0 + 1, fnz = meta[5] - fz0 + 1;
    const float t = nears[n], far = fars[n];
    bool go = t < far;
    float t_end = far, start = t;
    if (go) {
        MarcherT<true> m;
        m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, dt_gamma, max_steps, C, H, nullptr);
        // Perturbed first march (SdnRenderCtx::noises): the chain of iteration 0 starts at t0 = near + step_size(near) * noise -- the very
        // expression k_march_rays evaluates -- so t0 is the origin of the step lattice certified_jump walks and the `start` of a ray it
        // certifies nothing for.  The cull scan keeps starting at `near`: it then covers [near, far], a superset of the segment
        // [t0, far] the march can sample, so "no marked cell", t_end and t_safe hold for the march from t0 as they do for the march from
        // near (conservative: a ray whose only marked cells lie in [near, t0) stays on the list, marches, emits nothing and dies in
        // iteration 0 like any other ray without a sample).  No sample changes: both tests only ever REMOVE work that emits nothing.
        const float t0 = noises ? t + m.step_size(t) * noises[n] : t;
        start = t0;
        go = t0 < far;        // a ray perturbed to or past `far` emits nothing (march_ray's own first test)
        float t_safe = -__FLT_MAX__;
        if (go) go = ray_may_hit(cull_f, m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t, far, t_end, fx0, fy0, fz0, fnx, fny, fnz, &t_safe);
        rays_tend[n] = go ? t_end : kTendDead;     // what march_ray would cache on the ray's first march
        if (go && jump && m.dt_is_const) start = certified_jump(m, t0, fminf(t_safe, fminf(far, t_end)));
    }
    alive_a[n] = go ? (int32_t)n : -1;
    if (jump) jump[n] = start;
    return go;
}

__global__ void __launch_bounds__(256) k_cull_start(uint32_t N, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                    const float *__restrict__ nears, const float *__restrict__ fars,
                                                    const uint32_t *__restrict__ cull, FrameSel fs, int32_t *__restrict__ alive_a,
                                                    float *__restrict__ rays_tend, float bound, float dt_gamma, uint32_t max_steps, uint32_t C,
                                                    uint32_t H, float *__restrict__ jump, uint32_t *__restrict__ block_totals,
                                                    const float *__restrict__ noises) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    bool go = false;
    if (n < N) go = cull_start_ray(n, rays_o, rays_d, nears, fars, cull, fs, alive_a, rays_tend, bound, dt_gamma, max_steps, C, H, jump, noises);
    // rays of this 256-ray block that go on: the compaction's scatter sums these (no separate count launch)
    __shared__ uint32_t s_cnt[4];
    const uint32_t c = block_count_256(go, s_cnt);
    if (threadIdx.x == 0) block_totals[blockIdx.x] = c;
}

// after the compaction of the culled start: the list is in alive_b (side 1), n_out[0] rays long
__global__ void k_cull_advance(int32_t *__restrict__ state, const int32_t *__restrict__ n_out, int32_t *__restrict__ trace) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SdnLoopRecord &rec = *sdn_loop(state);
    const int32_t n0 = n_out[0];
    rec.side = 1;
    rec.culled_start = 1;     // iteration 0 runs on the culled list: the trace logs N for it
    if (n0 > 0) {
        rec.n_alive = n0;
    } else {                  // no ray can produce a sample: the reference's iteration 0 (N rays, one step) finds nothing and the loop ends
        trace[0] = rec.N;
        trace[1] = rec.n_step;
        rec.steps_done += rec.n_step;
        rec.iteration = 1;
        rec.n_alive = 0;
    }
}

// snap: 4 x {alive rays entering the next iteration, index of that iteration} -- an immutable per-iteration snapshot the
// host copies out on a side stream while the main stream already runs the next iteration.
__global__ void k_loop_advance(int32_t *__restrict__ state, const int32_t *__restrict__ n_out, int32_t *__restrict__ trace,
                               int32_t *__restrict__ snap, int freeze) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    advance_record<true, true>(*sdn_loop(state), trace, snap, n_out[0], freeze);
}

// Stable compaction of the alive list (256-ray blocks, totals produced by k_composite_rays) fused with the loop advance:
// the workgroup that draws the last ticket -- every workgroup of the launch takes one after its last read of the loop
// record -- sums the totals and advances the record, so no workgroup can see a half-updated record.
__global__ void __launch_bounds__(256) k_scatter_advance(int32_t *__restrict__ alive_a, int32_t *__restrict__ alive_b,
                                                         const uint32_t *__restrict__ block_totals, int32_t *__restrict__ state,
                                                         int32_t *__restrict__ ticket, int32_t *__restrict__ trace, int32_t *__restrict__ snap,
                                                         int freeze) {
    __shared__ uint32_t lds4[4];
    SdnLoopRecord &rec = *sdn_loop(state);
    const uint32_t n = sdn_loop_list_len(rec);
    const int32_t *in = rec.side ? alive_b : alive_a;
    int32_t *out = rec.side ? alive_a : alive_b;
    const uint32_t nb = (n + 255u) / 256u;
    if (blockIdx.x < nb) {
        uint32_t part = 0;
        for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256) part += block_totals[b];
        const uint32_t prev = block_sum_256(part, lds4);
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        ranked_scatter<4>(i < n ? in[i] : -1, prev, out, lds4);
    }
    __syncthreads();
    if (!last_workgroup(ticket)) return;
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) part += block_totals[b];
    const uint32_t total = block_sum_256(part, lds4);
    if (threadIdx.x == 0) advance_record<true, true>(rec, trace, snap, (int32_t)total, freeze);
}

// ---------------------------------------------------------------------------
// steady mode of the device loop: once n_alive <= N / 8 the schedule is n_step = 8 for good (n_alive only shrinks), so
// compositing iteration k and marching iteration k+1 of the same ray can be ONE kernel, and the alive list need not be
// compacted any more (dead entries are skipped; the field network only sees live samples through the live list).
// Two launches per iteration (fused field, composite+march) instead of five.  Samples, schedule and counts are unchanged.
// ---------------------------------------------------------------------------
__global__ void k_steady_begin(int32_t *__restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SdnLoopRecord &rec = *sdn_loop(state);
    rec.frozen_len = rec.n_alive;
    rec.survivors = 0;
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_composite_march(float T_thresh, int32_t *__restrict__ alive_a, int32_t *__restrict__ alive_b,
                                                         float *__restrict__ rays_t, const float *__restrict__ rays_o,
                                                         const float *__restrict__ rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                                         uint32_t C, uint32_t H, const uint8_t *__restrict__ grid, const float *__restrict__ fars,
                                                         const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                         float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                                                         float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
                                                         const uint32_t *__restrict__ cull, uint32_t *__restrict__ live_idx,
                                                         uint32_t *__restrict__ live_counts, int32_t *__restrict__ state,
                                                         int32_t *__restrict__ ticket, int32_t *__restrict__ trace, int32_t *__restrict__ snap,
                                                         FrameSel fs) {
    __shared__ uint4 s_cull4[FAST ? 256 : 1];
    __shared__ unsigned long long s_fine[FAST ? kFineCacheCells : 1];
    __shared__ uint32_t s_cnt[4], s_min4[4];
    SdnLoopRecord &rec = *sdn_loop(state);
    const uint32_t n_alive = (uint32_t)rec.n_alive, n_step = (uint32_t)rec.n_step, list_len = (uint32_t)rec.frozen_len;
    const int32_t it = rec.iteration;
    int32_t *__restrict__ alive = rec.side ? alive_b : alive_a;
    const bool march_next = (uint32_t)rec.steps_done + n_step < (uint32_t)rec.max_steps;  // `while step < max_steps` admits another iteration
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    bool survives = false;
    uint32_t emitted = 0;
    if (n_alive > 0 && blockIdx.x * 256u < list_len) {  // workgroup-uniform
        const int index = n < list_len ? alive[n] : -1;
        // composite iteration `it` of this ray; survivors march iteration it + 1 below.  The marcher's inputs are fetched together with
        // the compositing's (they land under it, the barriers and the LDS fill), and the ray's new t travels in a register
        RayIn ray;
        float t_new = 0;
        if (index >= 0) {
            if (march_next) ray_in_fetch(ray, index, rays_o, rays_d, fars);
            survives = composite_ray(index, n_step, T_thresh, sigmas + (size_t)n * n_step, rgbs + (size_t)n * n_step * 3,
                                     deltas + (size_t)n * n_step * 2, rays_t, weights_sum, depth, image, &t_new);
            if (!survives) alive[n] = -1;
        }
        frame_rounds<FAST>(fs, survives && march_next, index, grid, cull, s_cull4, s_fine, s_min4,
                           [&](const OccCache &oc, const uint8_t *grid_f, uint32_t frame, bool grouped) __attribute__((always_inline)) {
            float *px = xyzs + (size_t)n * n_step * 3, *pd = dirs + (size_t)n * n_step * 3, *pl = deltas + (size_t)n * n_step * 2;
            MarcherT<FAST> m;
            m.init(ray.o, ray.d, bound, dt_gamma, max_steps, C, H, grid_f);
            float *tend = sdn_loop_tend(rec);
            if (tend) tend += index;
            emitted = march_ray<FAST>(m, oc, t_new, ray.far, n_step, px, pd, pl, tend, grouped ? fs.slot_frame + (size_t)n * n_step : nullptr,
                                      frame);
        });
        live_append(emitted, n, n_step, live_idx, live_counts + it + 1);
    }
    // survivors of this workgroup -> global accumulator; the last workgroup of the launch advances the loop record
    const uint32_t c = block_count_256(survives, s_cnt);
    if (threadIdx.x == 0 && c) atomicAdd(&rec.survivors, (int32_t)c);
    if (!last_workgroup(ticket) || threadIdx.x != 0) return;
    const int32_t n_new = atomicAdd(&rec.survivors, 0);
    rec.survivors = 0;
    advance_record<false, false>(rec, trace, snap, n_new, 0);
}

// image = image + (1 - weights_sum) * bg ; depth = clamp(depth - nears, 0) / (fars - nears)   (dnerf/renderer.py:378-379)
__global__ void __launch_bounds__(256) k_loop_finish(uint32_t N, const float *__restrict__ nears, const float *__restrict__ fars,
                                                     const float *__restrict__ weights_sum, const float *__restrict__ depth,
                                                     const float *__restrict__ image, float bg, float *__restrict__ image_out,
                                                     float *__restrict__ depth_out) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const float w = (1 - weights_sum[n]) * bg;
    image_out[(size_t)n * 3] = image[(size_t)n * 3] + w;
    image_out[(size_t)n * 3 + 1] = image[(size_t)n * 3 + 1] + w;
    image_out[(size_t)n * 3 + 2] = image[(size_t)n * 3 + 2] + w;
    depth_out[n] = fmaxf(depth[n] - nears[n], 0.0f) / (fars[n] - nears[n]);
}

// k_march_rays' arguments by name, for the one function that picks its instantiation (the public marcher and the loop's share it)
struct MarchRays {
    uint32_t threads = 0;                  // lanes to launch
    uint32_t n_alive = 0, n_step = 0;      // 0, 0: the kernel reads them from `state`
    const int32_t *rays_alive = nullptr, *rays_alive_b = nullptr, *state = nullptr;
    const float *rays_t = nullptr, *rays_o = nullptr, *rays_d = nullptr, *fars = nullptr, *noises = nullptr;
    float bound = 0, dt_gamma = 0;
    uint32_t max_steps = 0, C = 0, H = 0, M_pad = 0;
    const uint8_t *grid = nullptr;
    float *xyzs = nullptr, *dirs = nullptr, *deltas = nullptr;
    const uint32_t *cull = nullptr;
    uint32_t *live_idx = nullptr, *live_count = nullptr;
    FrameSel fs;
    const float *jump = nullptr;           // only used with a cull grid
};
int launch_k_march_rays(const MarchRays &m, hipStream_t st) {
    const dim3 g(sdn_div_up(m.threads, 256u)), b(256);
    const bool fast = fast_config(m.bound, m.C, m.H);
    const uint32_t *cull = (fast && m.H == 128) ? m.cull : nullptr;   // the cull grid is built for the 128^3 grid of the FAST configuration only
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, g, b, 0, st, m.n_alive, m.n_step, m.rays_alive, m.rays_t, m.rays_o, m.rays_d, m.bound, m.dt_gamma, m.max_steps, m.C,
                           m.H, m.grid, m.fars, m.xyzs, m.dirs, m.deltas, m.noises, m.M_pad, cull, m.live_idx, m.live_count, m.state, m.rays_alive_b,
                           m.fs, cull ? m.jump : (const float *)nullptr);
    };
    if (fast) launch(k_march_rays<true>); else launch(k_march_rays<false>);
    return sdn_launch_status();
}

// byte offsets into the training marcher's scratch: scan workspace | cull grid of the time slice | t of every sample [N, max_steps]
struct TrainScratch { uint64_t cull, sample_t; };
TrainScratch train_scratch(uint32_t N) {
    const uint64_t words = (uint64_t)N + sdn_div_up(N, kScanBlock) + 4u;   // num_steps, block totals, bases
    const uint64_t head = (words * sizeof(uint32_t) + 15u) & ~(uint64_t)15u;
    const uint64_t cull_bytes = ((uint64_t)(kCullWords + 8u) * sizeof(uint32_t) + 15u) & ~(uint64_t)15u;
    return {head, head + cull_bytes};
}

}  // namespace

namespace sdn_int {

int loop_begin(const SdnRenderCtx &c, void *mailbox, uint32_t frame_tag, hipStream_t st) {
    const uint32_t threads = c.N > c.n_counters ? c.N : c.n_counters;
    hipLaunchKernelGGL(k_loop_init, dim3(sdn_div_up(threads, 256u)), dim3(256), 0, st, c.N, c.max_steps, c.nears, c.alive_a, c.rays_t, c.weights_sum,
                       c.depth, c.image, c.state, c.live_counts, c.n_counters, (unsigned long long)(uintptr_t)mailbox, frame_tag, c.rays_tend);
    return sdn_launch_status();
}

// Culled start (see k_cull_start): after loop_begin and after the context's cull grid(s) are in place.  Returns 0 without doing
// anything when the configuration has no exact cull test (not the FAST configuration, no cull grid, no t_end cache).
int loop_cull_start(const SdnRenderCtx &c, hipStream_t st) {
    const uint32_t *cull = loop_cull(c);
    if (!cull || !c.rays_tend || c.H != 128 || !fast_config(c.bound, c.C, c.H)) return 0;
    uint32_t *block_totals = (uint32_t *)c.block_totals;
    hipLaunchKernelGGL(k_cull_start, dim3(sdn_div_up(c.N, 256u)), dim3(256), 0, st, c.N, c.rays_o, c.rays_d, c.nears, c.fars, cull, frame_sel(c), c.alive_a,
                       c.rays_tend, c.bound, c.dt_gamma, c.max_steps, c.C, c.H, jump_buffer(c), block_totals, c.noises);
    const uint32_t nb = sdn_div_up(c.N, kScanBlock);
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kScanBlock), 0, st, (const int32_t *)c.alive_a, c.N, (const uint32_t *)block_totals, c.alive_b,
                       snap_n_out(c), (const int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, 4u);
    hipLaunchKernelGGL(k_cull_advance, dim3(1), dim3(64), 0, st, c.state, (const int32_t *)snap_n_out(c), c.trace);
    return sdn_launch_status();
}

// the loop's marcher on the alive list (n_alive / n_step from the loop record); jump: the culled start's targets, or nullptr
static int march(const SdnRenderCtx &c, uint32_t bound_alive, const float *jump, hipStream_t st) {
    MarchRays m;
    m.threads = bound_alive + 128u;
    m.rays_alive = c.alive_a; m.rays_alive_b = c.alive_b; m.rays_t = c.rays_t; m.rays_o = c.rays_o; m.rays_d = c.rays_d;
    m.bound = c.bound; m.dt_gamma = c.dt_gamma; m.max_steps = c.max_steps; m.C = c.C; m.H = c.H; m.grid = c.bitfield; m.fars = c.fars;
    m.xyzs = c.xyzs; m.dirs = c.dirs; m.deltas = c.deltas; m.cull = loop_cull(c); m.live_idx = c.live_idx; m.live_count = live_counters(c);
    m.state = c.state; m.fs = frame_sel(c); m.jump = jump;
    m.noises = c.noises;   // per ray, read by the march of iteration 0 only (k_march_rays)
    return launch_k_march_rays(m, st);
}

int loop_march(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st) { return march(c, bound_alive, jump_buffer(c), st); }

int loop_composite_compact(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st, bool freeze) {
    const dim3 g(sdn_div_up(bound_alive, 256u)), b(256);
    uint32_t *block_totals = (uint32_t *)c.block_totals;
    int32_t *snap = snap_ring(c);
    hipLaunchKernelGGL(k_composite_rays, g, b, 0, st, 0u, 0u, c.T_thresh, c.alive_a, c.rays_t, c.sigmas, c.rgbs, c.deltas, c.weights_sum, c.depth, c.image,
                       (const int32_t *)c.state, c.alive_b, block_totals);          // (+ survivors per 256 rays: no separate count launch)
    if (bound_alive > 65536u) {
        // many rays (the first one or two iterations): every scatter workgroup would re-sum thousands of 256-ray totals;
        // use the 1024-ray count / scatter pair and a separate one-thread advance instead.  (Measured again in round 3 with the fused pair up
        // to 131 072 / 262 144 / 524 288 rays: 0.449 / 0.451 / 0.451 ms per frame against 0.441 -- every workgroup of the fused scatter pays a
        // device-scope fence for the last-workgroup election.)
        static_assert(kScanBlock == 1024, "the compositing kernel's 256-ray survivor counts are summed four to a scatter block");
        const uint32_t nb = sdn_div_up(bound_alive, kScanBlock);
        hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kScanBlock), 0, st, (const int32_t *)c.alive_a, 0u, (const uint32_t *)block_totals,
                           c.alive_b, snap_n_out(c), (const int32_t *)c.state, (const int32_t *)c.alive_b, c.alive_a, 4u);
        hipLaunchKernelGGL(k_loop_advance, dim3(1), dim3(64), 0, st, c.state, (const int32_t *)snap_n_out(c), c.trace, snap, freeze ? 1 : 0);
        return sdn_launch_status();
    }
    // n_out doubles as the ticket counter (zero between launches)
    hipLaunchKernelGGL(k_scatter_advance, g, b, 0, st, c.alive_a, c.alive_b, (const uint32_t *)block_totals, c.state, c.n_out, c.trace, snap, freeze ? 1 : 0);
    return sdn_launch_status();
}

int loop_steady_begin(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st, bool frozen_already) {
    if (!frozen_already) hipLaunchKernelGGL(k_steady_begin, dim3(1), dim3(64), 0, st, c.state);
    return march(c, bound_alive, nullptr, st);
}

int loop_composite_march(const SdnRenderCtx &c, uint32_t bound_list, hipStream_t st) {
    const dim3 g(sdn_div_up(bound_list, 256u)), b(256);
    const FrameSel fs = frame_sel(c);
    int32_t *snap = snap_ring(c);
    const bool fast = fast_config(c.bound, c.C, c.H);
    const uint32_t *cull = (fast && c.H == 128) ? loop_cull(c) : nullptr;   // the cull grid is built for the 128^3 grid of the FAST configuration only
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, g, b, 0, st, c.T_thresh, c.alive_a, c.alive_b, c.rays_t, c.rays_o, c.rays_d, c.bound, c.dt_gamma, c.max_steps, c.C, c.H,
                           c.bitfield, c.fars, c.sigmas, c.rgbs, c.xyzs, c.dirs, c.deltas, c.weights_sum, c.depth, c.image, cull, c.live_idx,
                           live_counters(c), c.state, c.n_out, c.trace, snap, fs);   // (n_out: the ticket counter)
    };
    if (fast) launch(k_composite_march<true>); else launch(k_composite_march<false>);
    return sdn_launch_status();
}

int loop_finish(const SdnRenderCtx &c, float bg, float *image_out, float *depth_out, hipStream_t st) {
    hipLaunchKernelGGL(k_loop_finish, dim3(sdn_div_up(c.N, 256u)), dim3(256), 0, st, c.N, c.nears, c.fars, c.weights_sum, c.depth, c.image, bg, image_out,
                       depth_out);
    return sdn_launch_status();
}

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

FrameSel frame_sel(const SdnRenderCtx &c) {
    FrameSel fs;
    if (c.n_group_frames > 1) {
        fs.n_frames = c.n_group_frames;
        fs.rays_per_frame = c.rays_per_frame;
        fs.cull_stride = sdn_cull_grid_bytes() / 4u;
        for (uint32_t f = 0; f < c.n_group_frames && f < SDN_MAX_GROUP_FRAMES; f++) fs.grid[f] = c.frame_bitfield[f];
        fs.slot_frame = c.slot_frame;
    }
    return fs;
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

uint64_t sdn_march_rays_train_scratch_bytes(uint32_t N, uint32_t max_steps) {
    return train_scratch(N).sample_t + (uint64_t)N * max_steps * sizeof(float);
}

int sdn_march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                         uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *nears,
                         const float *fars, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                         const float *noises, void *scratch, void *stream) {
    return sdn_int::march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, nears, fars, xyzs, dirs, deltas, rays, counter, noises,
                                     scratch, nullptr, (hipStream_t)stream);
}

}  // extern "C"

// prebuilt_cull: the cull grid of `grid` from sdn_build_cull_grid (a caller that marches the same occupancy slice step after step
// keeps it), or nullptr: built here into the scratch
int sdn_int::march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                              uint32_t C, uint32_t H, uint32_t M, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                              int32_t *rays, int32_t *counter, const float *noises, void *scratch, const void *prebuilt_cull, hipStream_t st) {
    if (N == 0) return 0;
    if (!rays_o || !rays_d || !grid || !nears || !fars || !xyzs || !dirs || !deltas || !rays || !counter || !noises || !scratch)
        return SDN_E_BADARG;
    if (C == 0 || C > 16 || H == 0 || max_steps == 0 || ((uintptr_t)scratch & 15u) || ((uintptr_t)prebuilt_cull & 15u)) return SDN_E_BADARG;
    uint32_t *num_steps = (uint32_t *)scratch;
    const uint32_t nb = sdn_div_up(N, kScanBlock);
    uint32_t *block_totals = num_steps + N;
    uint32_t *base_out = block_totals + nb;
    const TrainScratch off = train_scratch(N);
    uint32_t *own_cull = (uint32_t *)((unsigned char *)scratch + off.cull);
    const uint32_t *cull = own_cull;
    float *sample_t = (float *)((unsigned char *)scratch + off.sample_t);
    const bool fast = fast_config(bound, C, H);
    const bool use_cull = fast && H == 128;
    if (use_cull && prebuilt_cull) {
        cull = (const uint32_t *)prebuilt_cull;
    } else if (use_cull) {
        int rc = sdn_int::build_cull(grid, own_cull, st, false);   // (the scratch has no room for the image)
        if (rc) return rc;
    }
    if (fast && dt_gamma == 0.0f && H <= 256u)   // constant step: one WAVE per ray (k_march_train_count_wave), same samples bit for bit
        hipLaunchKernelGGL(k_march_train_count_wave, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, rays_o, rays_d, grid, bound, max_steps, N, H, nears,
                           fars, noises, num_steps, use_cull ? cull : nullptr, sample_t);
    else if (fast) hipLaunchKernelGGL(k_march_train_count<true>, dim3(sdn_div_up(N, 256u)), dim3(256), 0, st, rays_o, rays_d, grid, bound, dt_gamma,
                                 max_steps, N, C, H, nears, fars, noises, num_steps, use_cull ? cull : nullptr, sample_t);
    else hipLaunchKernelGGL(k_march_train_count<false>, dim3(sdn_div_up(N, 256u)), dim3(256), 0, st, rays_o, rays_d, grid, bound, dt_gamma,
                            max_steps, N, C, H, nears, fars, noises, num_steps, (const uint32_t *)nullptr, sample_t);
    // The reference writes ray records at rays[atomicAdd(counter+1, 1)] and points at atomicAdd(counter, n):
    // both bases are read on the device from the counter the caller hands in (zeroed by dnerf/renderer.py:291-292).
    const bool small = N <= 16u * kScanBlock;
    if (small) {
        hipLaunchKernelGGL(k_march_train_offsets_small, dim3(1), dim3(kScanBlock), 0, st, num_steps, N, rays, counter, base_out);
    } else {
        hipLaunchKernelGGL(k_scan_block_totals, dim3(nb), dim3(kScanBlock), 0, st, num_steps, N, block_totals);
        hipLaunchKernelGGL(k_march_train_offsets, dim3(nb), dim3(kScanBlock), 0, st, num_steps, N, block_totals, rays, counter, base_out);
    }
    if (fast) hipLaunchKernelGGL(k_march_train_emit<true>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, rays_o, rays_d, bound, dt_gamma, max_steps, N, C, H, M,
                                 nears, noises, rays, base_out, sample_t, xyzs, dirs, deltas);
    else hipLaunchKernelGGL(k_march_train_emit<false>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, rays_o, rays_d, bound, dt_gamma, max_steps, N, C, H, M,
                            nears, noises, rays, base_out, sample_t, xyzs, dirs, deltas);
    if (!small) hipLaunchKernelGGL(k_march_train_finish, dim3(1), dim3(64), 0, st, counter, base_out, N);
    return sdn_launch_status();
}

extern "C" {

int sdn_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, uint32_t M,
                                     uint32_t N, float T_thresh, float *weights_sum, float *depth, float *image, void *stream) {
    if (N == 0) return 0;
    // (M == 0: empty sample tensors have no address; every ray then takes the kernel's `offset + num_steps > M` exit and reads none)
    if ((M != 0 && (!sigmas || !rgbs || !deltas)) || !rays || !weights_sum || !depth || !image) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_train_fwd, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, sigmas, rgbs, deltas, rays, M, N,
                       T_thresh, weights_sum, depth, image);
    return sdn_launch_status();
}

int sdn_composite_whole_rays(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, const float *nears, uint32_t M,
                             uint32_t N, float T_thresh, float *weights_sum, float *depth, float *image, void *stream) {
    if (N == 0) return 0;
    if (!sigmas || !rgbs || !deltas || !rays || !nears || !weights_sum || !depth || !image) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_whole_rays, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, sigmas, rgbs, deltas, rays, nears, M, N,
                       T_thresh, weights_sum, depth, image);
    return sdn_launch_status();
}

int sdn_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image, const float *sigmas, const float *rgbs,
                                      const float *deltas, const int32_t *rays, const float *weights_sum, const float *image,
                                      uint32_t M, uint32_t N, float T_thresh, float *grad_sigmas, float *grad_rgbs, void *stream) {
    if (N == 0) return 0;
    if (M == 0) return 0;       // no sample, no gradient entry to write
    if (!grad_weights_sum || !grad_image || !sigmas || !rgbs || !deltas || !rays || !weights_sum || !image || !grad_sigmas || !grad_rgbs)
        return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_train_bwd, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, grad_weights_sum, grad_image,
                       sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh, grad_sigmas, grad_rgbs);
    return sdn_launch_status();
}

static int launch_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                             const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                             const uint8_t *grid, const float *fars, float *xyzs, float *dirs, float *deltas, const float *noises,
                             uint32_t M_pad, const uint32_t *cull, uint32_t *live_idx, uint32_t *live_count, hipStream_t st) {
    if (n_alive == 0 || n_step == 0) {
        // no sample slots: the M_pad padding slots are still the caller's to read -- the reference hands out zero-filled buffers
        // (raymarching.py:333-335), and no kernel runs here that would clear them
        if (M_pad && xyzs && dirs && deltas) {
            if (hipMemsetAsync(xyzs, 0, (size_t)M_pad * 12, st) != hipSuccess || hipMemsetAsync(dirs, 0, (size_t)M_pad * 12, st) != hipSuccess ||
                hipMemsetAsync(deltas, 0, (size_t)M_pad * 8, st) != hipSuccess)
                return sdn_launch_status();
        }
        return 0;
    }
    if (!rays_alive || !rays_t || !rays_o || !rays_d || !grid || !fars || !xyzs || !dirs || !deltas) return SDN_E_BADARG;
    if (C == 0 || C > 16 || H == 0 || max_steps == 0) return SDN_E_BADARG;
    if ((live_idx == nullptr) != (live_count == nullptr)) return SDN_E_BADARG;
    const uint32_t base = n_alive * n_step;
    if (M_pad < base) M_pad = base;
    MarchRays m;
    m.threads = n_alive + (M_pad - base);  // one lane per alive ray + one per tail slot
    m.n_alive = n_alive; m.n_step = n_step; m.rays_alive = rays_alive; m.rays_t = rays_t; m.rays_o = rays_o; m.rays_d = rays_d;
    m.bound = bound; m.dt_gamma = dt_gamma; m.max_steps = max_steps; m.C = C; m.H = H; m.grid = grid; m.fars = fars;
    m.xyzs = xyzs; m.dirs = dirs; m.deltas = deltas; m.noises = noises; m.M_pad = M_pad; m.cull = cull; m.live_idx = live_idx; m.live_count = live_count;
    return launch_k_march_rays(m, st);
}

int sdn_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                   const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                   const uint8_t *grid, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                   const float *noises, void *stream) {
    (void)nears;  // unused by the reference kernel as well (raymarching.cu:737)
    return launch_march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, fars, xyzs, dirs,
                             deltas, noises, 0, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int sdn_march_rays_ex(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                      const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                      const uint8_t *grid, const float *fars, float *xyzs, float *dirs, float *deltas, const float *noises,
                      uint32_t M_pad, const uint8_t *cull_grid, uint32_t *live_idx, uint32_t *live_count, void *stream) {
    return launch_march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, fars, xyzs, dirs,
                             deltas, noises, M_pad, (const uint32_t *)cull_grid, live_idx, live_count, (hipStream_t)stream);
}

uint32_t sdn_cull_grid_bytes(void) { return kCullImageWord * 4 + kFineCacheCells * 8; }  // marks + bounding-box record + packed fine bits

int sdn_build_cull_grid(const uint8_t *bitfield, uint32_t H, uint8_t *cull_grid, void *stream) {
    if (!bitfield || !cull_grid) return SDN_E_BADARG;
    if (H != 128) return SDN_E_UNSUPPORTED;
    if (((uintptr_t)bitfield & 7u) != 0 || ((uintptr_t)cull_grid & 15u) != 0) return SDN_E_BADARG;
    return sdn_int::build_cull(bitfield, (uint32_t *)cull_grid, (hipStream_t)stream);
}

int sdn_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t, const float *sigmas,
                       const float *rgbs, const float *deltas, float *weights_sum, float *depth, float *image, void *stream) {
    if (n_alive == 0 || n_step == 0) return 0;
    if (!rays_alive || !rays_t || !sigmas || !rgbs || !deltas || !weights_sum || !depth || !image) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_rays, dim3(sdn_div_up(n_alive, 256u)), dim3(256), 0, (hipStream_t)stream, n_alive, n_step, T_thresh,
                       rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, (const int32_t *)nullptr, (int32_t *)nullptr,
                       (uint32_t *)nullptr);
    return sdn_launch_status();
}

uint64_t sdn_compact_alive_scratch_bytes(uint32_t n) { return (uint64_t)sdn_div_up(n, kScanBlock) * sizeof(uint32_t); }

int sdn_compact_alive(const int32_t *in, uint32_t n, int32_t *out, int32_t *n_out, void *scratch, void *stream) {
    if (!n_out) return SDN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return (int)hipMemsetAsync(n_out, 0, sizeof(int32_t), st);
    if (!in || !out || !scratch) return SDN_E_BADARG;
    const uint32_t nb = sdn_div_up(n, kScanBlock);
    hipLaunchKernelGGL(k_compact_count, dim3(nb), dim3(kScanBlock), 0, st, in, n, (uint32_t *)scratch, (const int32_t *)nullptr,
                       (const int32_t *)nullptr);
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kScanBlock), 0, st, in, n, (const uint32_t *)scratch, out, n_out,
                       (const int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, 1u);
    return sdn_launch_status();
}

}  // extern "C"
