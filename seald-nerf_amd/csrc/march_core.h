// Device code the marching translation units share: the DDA stepper MarcherT, the cull-grid layout and the exact cull test, the LDS
// occupancy caches, the closed form of the constant-step lattice, and the two host rules that pick a marcher's configuration.
// Included by raymarching.hip (utilities, cull-grid build), march_train.hip (training marcher) and render_loop.hip (inference marcher,
// device-driven loop).  No kernel lives here: everything is internal to the including unit, which instantiates only what it uses.
//
// Behavioural contract: raymarching/src/raymarching.cu of the reference (line ranges cited per function).  Arithmetic contract: the
// including units are built with -ffp-contract=off so that every float operation rounds on its own, in the order the reference
// source writes it -- which is what oracle/sdn_oracle.c evaluates on the CPU.
#pragma once
#include "sdn_common.h"
#include "sdn_internal.h"

namespace {
using sdn_int::FrameSel;

constexpr float kSqrt3 = 1.7320508075688772f;

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
// The DDA stepper shared by the training count pass (both forms), the training emit pass, the inference marcher, the steady loop's
// composite+march kernel and the culled start (raymarching.cu:359-400 == 427-479 == 750-804).
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

static inline bool fast_config(float bound, uint32_t C, uint32_t H) {
    return C == 1 && bound == 1.0f && H >= 2 && H <= 256 && (H & (H - 1)) == 0;
}
// the cull grid is built for the 128^3 grid of the FAST configuration only: a marcher of any other configuration is handed none
static inline bool cull_grid_applies(float bound, uint32_t C, uint32_t H) { return H == 128 && fast_config(bound, C, H); }

// ---------------------------------------------------------------------------
// Exact early-out for rays that cannot produce a sample ("cull grid").
// cull[32^3] (x fastest) marks coarse cells (4^3 fine voxels of the 128^3 grid) whose 3x3x3 coarse neighbourhood
// holds any occupied voxel.  A ray whose remaining segment [t, far], tested every cell width, only sees unmarked
// cells stays >= half a coarse cell (2 fine voxels) away from every occupied voxel, so the reference's marcher --
// whose probe points lie on that segment up to float rounding -- emits nothing for it: returning "no samples"
// is exact, not an approximation.  Rays that may hit take the full reference chain from their own t.
// (The grid is built by k_build_cull_grid / k_build_fine_image, raymarching.hip.)
// ---------------------------------------------------------------------------

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

// The bound t_end found by ray_may_hit -- beyond it the ray meets no marked cell -- is a property of the ray, not of where the scan
// started, so the device loop keeps it per ray (kTendUnset: not computed yet; kTendDead: the ray cannot produce a sample).
constexpr float kTendUnset = -2.0f, kTendDead = -1.0f;

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

}  // namespace
