// The network of the two fp16 fused field kernels, written once: the stages of NeRFNetwork.forward under `-O` (the behavioural contract
// at the top of field.hip) as functions over plain values and register arrays.  k_field_f16 (field.hip: one tile per workgroup) and
// k_field_pp_f16 (field_pp.inc: persistent, two sets) call them and keep only what is theirs -- the weight staging, the wide layers'
// MFMA order, barriers, priorities, scheduling pins and the batching of the gathers.  A stage holds arithmetic and operand order, no
// schedule: where a kernel must pin a stage's result in registers it does so at the call.
//
// Lane layout: a wave owns 32 points, lane-half h = lane / 32 holds point n = lane % 32.  A 32 x 32 x 16 MFMA leaves row
// 8 (r / 4) + 4 h + r % 4 of its output tile in accumulator register r, and that order is the k-order of the next layer's operand
// (baked into the weight packing, dnerf_amd/fused.py), so an accumulator converts in place into operand fragments.
#pragma once
#include <stdint.h>

#include "sdn_common.h"
#include "sdn_internal.h"
#include "sh_eval.h"

namespace sdn_f16 {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// fragment (1 KiB block) indices inside the packed weight buffer
constexpr int kBlkD0 = 0;                 // 4 Mt x 4 ks
constexpr int kBlkD1 = kBlkD0 + 16;       // 6 layers x (4 Mt x 8 ks)
constexpr int kBlkD7 = kBlkD1 + 6 * 32;   // 1 Mt x 8 ks
constexpr int kBlkS0 = kBlkD7 + 8;        // 2 Mt x 2 ks
constexpr int kBlkS1 = kBlkS0 + 4;        // 1 Mt x 4 ks
constexpr int kBlkC0 = kBlkS1 + 4;        // 2 Mt x 2 ks
constexpr int kBlkC1 = kBlkC0 + 4;        // 2 Mt x 4 ks
constexpr int kBlkC2 = kBlkC1 + 8;        // 1 Mt x 4 ks
constexpr int kBlkTotal = kBlkC2 + 4;     // 240
static_assert(kBlkTotal - kBlkD7 == 32, "the tail stage must be exactly one 32 KiB buffer");
// the small layers inside the tail stage (D7 | S0 | S1 | C0 | C1 | C2)
constexpr int tD7 = 0, tS0 = kBlkS0 - kBlkD7, tS1 = kBlkS1 - kBlkD7, tC0 = kBlkC0 - kBlkD7, tC1 = kBlkC1 - kBlkD7, tC2 = kBlkC2 - kBlkD7;

// tiled-grid level constants (D = 3, align_corners = false), host-precomputed: gridencoder.cu:66-84,138-139
struct TiledLevels {
    uint32_t offset[16];  // first row of the level
    uint32_t s1[16];      // row stride of +1 in y (0 if the dimension is dropped: stride > rows)
    uint32_t s2[16];      // row stride of +1 in z (0 if dropped)
    uint32_t hsize[16];   // rows in the level
    uint32_t mask[16];    // hsize - 1 if hsize is a power of two (wrapping level), else 0xFFFFFFFF (dense level)
    float scale[16];
};

struct FieldArgs {
    const float *xyzs;        // [M,3]
    const float *dirs;        // [M,3]
    const uint32_t *live_idx; // [<=M] slot indices to evaluate, or nullptr = all M slots
    const uint32_t *live_count;
    const int32_t *state;     // device-driven loop: the count is live_count[SdnLoopRecord::iteration] (one counter per iteration), else nullptr
    uint32_t M;
    const unsigned char *weights;  // kBlkTotal KiB, fragment order
    const float *bias0;       // [128] time-encoding contribution to the first deform layer
    const __half *table;      // grid embeddings, fp16 [rows, 2]
    float *sigmas;            // [M]
    float *rgbs;              // [M,3]
    float bound;
    float inv_2bound;         // 1 / (2 bound) if that is a power of two (the division is then an exact multiplication), else 0
    float density_scale;
    int zero_deform;          // bit f: frame f is at t == 0, the canonical frame (dnerf/network.py:140-141); a single frame uses bit 0
    const uint8_t *slot_frame;  // frame group: frame of every sample slot (selects bias0 + 128 f and bit f of zero_deform), or nullptr
    // density-grid query (CELLS variant): the points are jittered centres of occupancy-grid cells, built in the kernel
    const float *cell_noise;  // [count,3] uniform [0,1) by list position, or nullptr = counter-based generator on cell_seed
    uint32_t cell_seed;
    float cell_inv;           // 1 / (grid_size - 1) in fp32: torch divides a tensor by a host scalar as a multiplication by its reciprocal
    float cell_span;          // bound_cas - half_grid   (dnerf/renderer.py:484-488)
    float cell_half;          // half_grid = bound_cas / grid_size
    uint32_t n_frames;        // rows of bias0 (frames of a frame group; 1 without slot_frame)
    uint32_t pp_soft;         // persistent kernel: the workgroup count to stay within unless more workgroups save a whole round (0 = gridDim.x)
};

__device__ __forceinline__ f32x16 mfma(half8 a, half8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

__device__ __forceinline__ f32x16 zero_tile() {
    f32x16 z;
    #pragma unroll
    for (int r = 0; r < 16; r++) z[r] = 0.0f;
    return z;
}

// accumulator tile -> the two B fragments (k-steps) it provides to the next layer
// (the reference rounds the Linear output to fp16 and applies ReLU on the fp16 tensor: round first, then a packed max)
template <bool RELU>
__device__ __forceinline__ void acc_to_frags(const f32x16 &acc, half8 &f0, half8 &f1) {
    #pragma unroll
    for (int j = 0; j < 8; j++) {
        f0[j] = (_Float16)acc[j];
        f1[j] = (_Float16)acc[8 + j];
    }
    if (RELU) {
        const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
        f0 = __builtin_elementwise_max(f0, zero);
        f1 = __builtin_elementwise_max(f1, zero);
    }
}

__device__ __forceinline__ float round_h(float v) { return (float)(_Float16)v; }

// fp32 multiply with one operand taken straight from the low / high half of a packed fp16 pair (v_fma_mix_f32):
//   mix_mul_*(w, h2) = w * float(h2.half)        as fma(w, half, -0)  -- identical to the rounded product for every input
__device__ __forceinline__ float mix_mul_lo(float w, uint32_t h2) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(r) : "v"(w), "v"(h2), "s"(-0.0f));
    return r;
}
__device__ __forceinline__ float mix_mul_hi(float w, uint32_t h2) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(r) : "v"(w), "v"(h2), "s"(-0.0f));
    return r;
}
// sin(a) and cos(a) with one shared 3-term Cody-Waite reduction by pi (explicit FMAs: this file is built with -ffp-contract=off):
// r = a - k pi in [-pi/2, pi/2], sin(a) = (-1)^k sin(r), cos(a) = (-1)^k cos(r); odd degree-9 / even degree-10 polynomials,
// ~1.3e-7 absolute for |a| < ~1e4.  The standalone freq_encode kernel uses OCML sinf (<= 1 ulp); the two agree to ~1e-7, far below
// the fp16 rounding the features get as MFMA operands.
__device__ __forceinline__ void fast_sincos(float a, float &sn, float &cs) {
    const float k = rintf(a * 0.31830988618379067f);
    float r = __builtin_fmaf(-k, 3.140625f, a);
    r = __builtin_fmaf(-k, 9.67502593994140625e-4f, r);
    r = __builtin_fmaf(-k, 1.509957990978376e-7f, r);
    const float r2 = r * r;
    float p = __builtin_fmaf(r2, 2.6083159809786593e-6f, -1.9810690719168633e-4f);
    p = __builtin_fmaf(p, r2, 8.3330785855650902e-3f);
    p = __builtin_fmaf(p, r2, -1.6666659712791443e-1f);
    const float s = __builtin_fmaf(r * r2, p, r);
    float q = __builtin_fmaf(r2, -2.6051615e-07f, 2.4760495e-05f);
    q = __builtin_fmaf(q, r2, -1.3888378e-03f);
    q = __builtin_fmaf(q, r2, 4.1666638e-02f);
    q = __builtin_fmaf(q, r2, -0.5f);
    const float c = __builtin_fmaf(q, r2, 1.0f);
    const int sign = ((int)k & 1) << 31;
    sn = __int_as_float(__float_as_int(s) ^ sign);
    cs = __int_as_float(__float_as_int(c) ^ sign);
}

__device__ __forceinline__ half8 lds_frag(const unsigned char *buf, int blk, uint32_t lane) {
    return *reinterpret_cast<const half8 *>(buf + (size_t)blk * 1024 + lane * 16);
}

// per grid level in LDS: {offset, s1, s2, hsize}, {mask, scale, -, -} (two 16-byte reads per level instead of six per-lane selects
// between kernarg values, which the compiler turns into six per-lane global loads); visible after the caller's next barrier
__device__ __forceinline__ void levels_to_lds(uint4 (*s_lv)[2], const TiledLevels &lv) {
    if (threadIdx.x < 16) {
        const uint32_t l = threadIdx.x;
        s_lv[l][0] = make_uint4(lv.offset[l], lv.s1[l], lv.s2[l], lv.hsize[l]);
        s_lv[l][1] = make_uint4(lv.mask[l], __float_as_uint(lv.scale[l]), 0u, 0u);
    }
}

// points of the launch: the device loop's counter of this iteration, a live list's count, or every slot
__device__ __forceinline__ uint32_t live_points(const FieldArgs &P) {
    return P.state ? P.live_count[sdn_loop(P.state)->iteration] : (P.live_idx ? *P.live_count : P.M);
}

// ---------------- deform layer 0: freq features as B fragments ----------------
// lane-half h owns (freq, dim) pairs 15h .. 15h+14 (sin and cos) plus x0,x1 (h = 0) / x2,pad (h = 1), i.e. the five octaves
// 2^(5h) .. 2^(5h+4) of every coordinate.  One sine / cosine pair per coordinate at the lane-half's base octave (shared range
// reduction, two short polynomials), the four higher octaves by angle doubling in fp32:  s' = 2 s c,  c' = 1 - 2 s^2  -- 6
// polynomial evaluations + 48 multiply-adds per lane instead of 30 sine evaluations.  The doubling error (<= 2^4 x 1e-7) is two
// orders of magnitude below the fp16 rounding the features get as MFMA operands; kernel_freq (freqencoder.cu:52-56) evaluates
// cos as sin(x 2^f + float(pi/2)), which is itself off by up to 3e-5 at 2^9 -- the values here are the closer to the exact ones.
// (v_sin_f32 / v_cos_f32 on revolutions measured no faster and leave 1.6 % of the fp16 features off the exactly rounded value against
//  0.14 % for this pair and 0.40 % for the reference's own float form: profiles/r04_field_valu_diet.txt)
__device__ __forceinline__ void freq_base(float x0, float x1, float x2, uint32_t h, float (&sv0)[3], float (&cv0)[3]) {
    const float xs[3] = {x0, x1, x2};
    const float fscale = h ? 32.0f : 1.0f;
    #pragma unroll
    for (int dd = 0; dd < 3; dd++) fast_sincos(xs[dd] * fscale, sv0[dd], cv0[dd]);
}
// the four doublings and the 32 slots of the lane-half (4 k-steps of D0) into bf[0..3]
__device__ __forceinline__ void freq_operand(float x0, float x1, float x2, uint32_t h, const float (&sv0)[3], const float (&cv0)[3], half8 (&bf)[8]) {
    float sv[5][3], cv[5][3];
    #pragma unroll
    for (int dd = 0; dd < 3; dd++) {
        sv[0][dd] = sv0[dd]; cv[0][dd] = cv0[dd];
        #pragma unroll
        for (int f = 1; f < 5; f++) {
            const float sp = sv[f - 1][dd], cp = cv[f - 1][dd];
            const float s2 = sp + sp;                         // (2 s) c and 1 - (2 s) s: the same roundings as 2 (s c) and 1 - 2 s^2
            sv[f][dd] = s2 * cp;
            cv[f][dd] = __builtin_fmaf(-s2, sp, 1.0f);
        }
    }
    #pragma unroll
    for (int s = 0; s < 4; s++) {
        #pragma unroll
        for (int j = 0; j < 8; j++) {
            const int q = s * 8 + j;
            float v;
            if (q < 30) {
                const int pr = q >> 1, f = pr / 3, dd = pr % 3;
                v = (q & 1) ? cv[f][dd] : sv[f][dd];
            } else if (q == 30) {
                v = h ? x2 : x0;
            } else {
                v = h ? 0.0f : x1;
            }
            bf[s][j] = (_Float16)v;
        }
    }
}

// D0's initial accumulators: the time encoding's bias row of the point's frame (global memory or LDS), register r of output tile mt <->
// feature 32 mt + 8 (r >> 2) + 4 h + (r & 3)
__device__ __forceinline__ void bias_rows(const float *b0_row, uint32_t h, f32x16 (&acc)[4]) {
    #pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        #pragma unroll
        for (int r = 0; r < 16; r++) acc[mt][r] = b0_row[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h];
    }
}

// One small layer of the tail stage: MT output tiles of KS k-steps each, A fragments blk + mt KS + ks of `tail`, from zero.
template <int MT, int KS>
__device__ __forceinline__ void small_layer(const unsigned char *tail, int blk, const half8 *in, f32x16 *acc, uint32_t lane) {
    #pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        acc[mt] = zero_tile();
        #pragma unroll
        for (int ks = 0; ks < KS; ks++) acc[mt] = mfma(lds_frag(tail, blk + mt * KS + ks, lane), in[ks], acc[mt]);
    }
}
// two accumulator tiles (64 features) -> the four operand fragments of the next layer, ReLU
__device__ __forceinline__ void relu_frags(const f32x16 (&acc)[2], half8 (&f)[4]) {
    acc_to_frags<true>(acc[0], f[0], f[1]);
    acc_to_frags<true>(acc[1], f[2], f[3]);
}

// A stage ends where its MFMAs end (deform_d7, colour_hidden) or holds none (grid_coords, grid_operand): the persistent kernel raises
// its priority around exactly the MFMAs.
// ---------------- deform layer 7 (128 -> 3); deformation and grid coordinates ----------------
__device__ __forceinline__ f32x16 deform_d7(const unsigned char *tail, const half8 (&in)[8], uint32_t lane) {
    f32x16 o;
    small_layer<1, 8>(tail, tD7, in, &o, lane);
    return o;
}
// rows 0..2 of D7 = registers 0..2 of lane-half 0, broadcast to both halves; `canonical`: the frame is at t == 0 and deforms nothing
// (dnerf/network.py:139-141); GridEncoder.forward (grid.py:149): (x + bound) / (2 bound) -- for 2 bound a power of two the quotient is
// the exact product
__device__ __forceinline__ void grid_coords(const f32x16 &o, uint32_t lane, float x0, float x1, float x2, bool canonical, const FieldArgs &P,
                                            float (&u)[3]) {
    float df[3];
    #pragma unroll
    for (int c = 0; c < 3; c++) df[c] = __shfl(round_h(o[c]), (int)(lane & 31u), 64);
    const float xs[3] = {x0, x1, x2};
    #pragma unroll
    for (int c = 0; c < 3; c++) {
        const float xd = canonical ? xs[c] : xs[c] + df[c];
        u[c] = P.inv_2bound != 0.0f ? (xd + P.bound) * P.inv_2bound : (xd + P.bound) / (2 * P.bound);
    }
}
// a point outside [0, 1]^3 gets zero features (kernel_grid's early out)
__device__ __forceinline__ bool out_of_grid(const float (&u)[3]) {
    return (u[0] < 0) | (u[0] > 1) | (u[1] < 0) | (u[1] > 1) | (u[2] < 0) | (u[2] > 1);
}

// ---------------- grid encode ----------------
// One level's cell: fractions fr and the (unwrapped) row of the cell's low corner; k0 = {offset, s1, s2, hsize}, k1 = {mask, scale}.
//   pos = u scale + 0.5 >= 0.5 for every point that is not zeroed as out of range: the truncating conversion IS floor, and
//   v_fract_f32 returns pos - floor(pos), which is exact in fp32 -- the reference's `pos -= (float)pos_grid` (gridencoder.cu:147-151);
//   rows: cell coordinates <= 2049 and strides <= 2049^2 < 2^24: the low 32 bits of the 24 x 24-bit products are the uint32
//   products of get_grid_index (gridencoder.cu:66-84), wrap-around included (v_mad_u32_u24, not the quarter-rate v_mul_lo_u32);
//   `index % hashmap_size` without a division (the caller's AND with k1.x): capped levels have a power-of-two row count; dense levels
//   hold every (res+1)^3 corner, so an in-range point never wraps.
// `outside`: the caller wants row 0 for a point outside the grid (written as the parent of the row arithmetic, which the compiler then
// skips for such lanes; the persistent kernel passes false and masks the row instead).
__device__ __forceinline__ uint32_t level_cell(const uint4 &k0, const uint4 &k1, const float (&u)[3], float (&fr)[3], bool outside) {
    const float scale = __uint_as_float(k1.y);
    uint32_t pg[3];
    #pragma unroll
    for (int d = 0; d < 3; d++) {
        const float q = u[d] * scale + 0.5f;
        pg[d] = (uint32_t)q;
        fr[d] = __builtin_amdgcn_fractf(q);
    }
    return outside ? 0u : pg[0] + __umul24(pg[1], k0.y) + __umul24(pg[2], k0.z);
}
// kernel_grid (gridencoder.cu:187-189), scalar_t = at::Half:  results[ch] += w * grid[index + ch]  is
//   t = Half(w * float(val));  results = Half(float(results) + float(t))
// -- the float product is converted to Half first (the only `Half += x` takes a Half).  The products come from
// v_fma_mix_f32 reading the fp16 halves of the gathered word in place (w * val as fma(w, val, -0): the individually
// rounded fp32 product), one v_cvt_pk_f16_f32 rounds both channels, and the Half + Half sum is ONE v_pk_add_f16:
// for two fp16 operands the fp16-rounded exact sum equals Half(fp32 sum) (24 >= 2 * 11 + 2 bits: no double-rounding
// case exists).  4 VALU instructions per corner for both channels.  `corner_bits(idx)` = the half2 of corner idx (bit d set:
// +1 along dimension d), in the reference's corner order.  Returns the level's two features as a packed pair (the caller zeroes them
// for a point outside the grid).
template <typename Corner>
__device__ __forceinline__ uint32_t interp_corners(const float (&fr)[3], Corner corner_bits) {
    half2v accv = {(_Float16)0.0f, (_Float16)0.0f};
    #pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) {
        float w = 1;
        #pragma unroll
        for (uint32_t d = 0; d < 3; d++) w *= (idx & (1u << d)) ? fr[d] : 1 - fr[d];
        const uint32_t bits = corner_bits(idx);
        const half2v t = {(_Float16)mix_mul_lo(w, bits), (_Float16)mix_mul_hi(w, bits)};
        accv = accv + t;
    }
    return __builtin_bit_cast(uint32_t, accv);
}
// corner idx of a cell from its two QUAD blocks (z and z + 1: each the four (x, y) corners)
__device__ __forceinline__ uint32_t quad_corner(const uint4 (&quads)[2], uint32_t idx) {
    const uint4 &q = quads[idx >> 2];
    return (idx & 3u) == 0u ? q.x : ((idx & 3u) == 1u ? q.y : ((idx & 3u) == 2u ? q.z : q.w));
}

// The fp16 table's layouts (field.hip describes them at k_field_f16; the host recognises one from the offsets it comes with).
constexpr int kLayoutRef = 0, kLayoutPad = 1, kLayoutQuad = 2;

// the lane-half's 8 levels x 2 features (packed pairs) as the sigma net's operand
__device__ __forceinline__ void grid_operand(const uint32_t (&gfw)[2][4], half8 (&gf)[2]) {
    #pragma unroll
    for (int q = 0; q < 2; q++) gf[q] = __builtin_bit_cast(half8, (u32x4){gfw[q][0], gfw[q][1], gfw[q][2], gfw[q][3]});
}
// ---------------- sigma net: 32 -> 64 (ReLU) -> 16 ----------------
__device__ __forceinline__ f32x16 sigma_net(const unsigned char *tail, const half8 (&gf)[2], uint32_t lane) {
    f32x16 s0[2], hv;
    small_layer<2, 2>(tail, tS0, gf, s0, lane);
    half8 sf[4];
    relu_frags(s0, sf);
    small_layer<1, 4>(tail, tS1, sf, &hv, lane);
    return hv;
}
// h[0] (lane-half 0, register 0) is the density logit; trunc_exp = exp in fp32 of the fp16 value
// (v_exp_f32 on h log2(e): 1 ulp of the hardware exponential plus |h| 2^-24 from the product -- the reference's own operators use the
//  fast intrinsics of their platform here (__expf), and sigma feeds a compositing sum that is compared at 1e-4 / fp16 distance)
__device__ __forceinline__ float density_of_logit(float logit, float density_scale) {   // logit: an fp16 value
    return density_scale * __builtin_amdgcn_exp2f(logit * 1.4426950408889634f);
}
__device__ __forceinline__ float density(const f32x16 &hv, float density_scale) { return density_of_logit(round_h(hv[0]), density_scale); }

// ---------------- colour net: [geo_feat(15) ++ SH(16)] -> 64 -> 64 -> 3 ----------------
// k-step 0 of its first layer: registers 0..7 of every lane = h[0..15], raw; the column of h[0] is zero in the packed weights
__device__ __forceinline__ half8 geo_operand(const f32x16 &hv) {
    half8 geo, dummy;
    acc_to_frags<false>(hv, geo, dummy);
    return geo;
}
// k-step 1: SH coefficient 8 h + j of the direction
__device__ __forceinline__ half8 sh_operand(float d0, float d1, float d2, uint32_t h) {
    float sh[16];
    float *nul = nullptr;
    sdn_sh::sh_eval<4, false>(d0, d1, d2, sh, nul, nul, nul);
    half8 f;
    #pragma unroll
    for (int j = 0; j < 8; j++) {
        float lo = sh[j], hi = sh[8 + j];
        // pin both candidates in VGPRs: otherwise the select of two array elements becomes one dynamically indexed
        // load and the whole array is demoted to LDS
        asm volatile("" : "+v"(lo), "+v"(hi));
        f[j] = (_Float16)(h ? hi : lo);
    }
    return f;
}
// its two hidden layers; the caller's relu_frags(c1, ..) gives the last layer's operand
__device__ __forceinline__ void colour_hidden(const unsigned char *tail, const half8 (&cf)[2], uint32_t lane, f32x16 (&c1)[2]) {
    f32x16 c0[2];
    small_layer<2, 2>(tail, tC0, cf, c0, lane);
    half8 c1f[4];
    relu_frags(c0, c1f);
    small_layer<2, 4>(tail, tC1, c1f, c1, lane);
}
__device__ __forceinline__ f32x16 colour_out(const unsigned char *tail, const half8 (&c2f)[4], uint32_t lane) {
    f32x16 co;
    small_layer<1, 4>(tail, tC2, c2f, &co, lane);
    return co;
}
// torch.sigmoid on an fp16 logit: fp32 math, fp16 result
__device__ __forceinline__ float rgb_of_logit(float logit) {
    return round_h(__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(logit * -1.4426950408889634f)));
}
// rows 0..2 of `co` are the colour logits
__device__ __forceinline__ void store_sigma_rgb(const FieldArgs &P, uint32_t p, float sigma, const f32x16 &co) {
    P.sigmas[p] = sigma;
    #pragma unroll
    for (int c = 0; c < 3; c++) P.rgbs[(size_t)p * 3 + c] = rgb_of_logit(round_h(co[c]));
}

}  // namespace sdn_f16

// Host side, shared by the launchers of the kernels built from these stages (defined in field.hip): the kernels' argument records of
// one call (cell fields zero), and the layout (kLayout*) a table's offsets announce.  For a kernel with a grid of its own dimension
// (field_hyper.hip: D = 4): the argument record without the levels, and the levels of a D-dimensional tiled grid -- the 3-D record plus
// the fourth coordinate's stride s3 [16] (0 where a level's index drops it).
namespace sdn_int {
int fill_field_args(sdn_f16::FieldArgs &a, sdn_f16::TiledLevels &lv, const FieldCall &f);
void fill_field_record(sdn_f16::FieldArgs &a, const FieldCall &f);
int fill_tiled_levels_nd(sdn_f16::TiledLevels &lv, uint32_t (*s3)[16], uint32_t D, const int32_t *offsets_host, float S, uint32_t H);
int field_table_layout(const int32_t *offsets_host);
}  // namespace sdn_int
