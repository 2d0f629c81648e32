// The stages the temporal-basis field (dnerf/network_basis.py under `-O`) adds to those of field_f16_net.h, over the same lane layout:
// a wave owns 32 points, lane-half h = lane / 32 holds point n = lane % 32, and register r of an accumulator tile mt holds output
// feature 32 mt + 8 (r / 4) + 4 h + r % 4.  The model has no deformation network: a static tiled grid feeds a sigma net that emits 32
// density coefficients and 32 geo_feat, a colour net emits 3 x 8 colour coefficients, and the frame's basis row -- 32 + 8 weights, the
// output of a 5-layer MLP of the time stamp alone, computed on the host -- contracts them.
#pragma once
#include "field_f16_net.h"

namespace sdn_basis {

using namespace sdn_f16;

// fragment (1 KiB block) indices inside the packed weight buffer (dnerf_amd/fused_basis.py); all of it stays resident in LDS
constexpr int kBlkS0 = 0;              // 32 -> 64: 2 Mt x 2 ks
constexpr int kBlkS1 = kBlkS0 + 4;     // 64 -> 64 (32 density coefficients | 32 geo_feat): 2 Mt x 4 ks
constexpr int kBlkC0 = kBlkS1 + 8;     // [SH(16) ++ geo_feat(32)] -> 64: 2 Mt x 3 ks
constexpr int kBlkC1 = kBlkC0 + 6;     // 64 -> 64: 2 Mt x 4 ks
constexpr int kBlkC2 = kBlkC1 + 8;     // 64 -> 24 (rows 24..31 of the tile are zero): 1 Mt x 4 ks
constexpr int kBlkTotal = kBlkC2 + 4;  // 30
// the basis row: [128] fp32 holding fp16 values -- sigma_basis in 0..31, color_basis in 32..39, the rest zero
constexpr int kRowColour = 32;

// ---------------- grid encode: lane-half h evaluates levels 8h .. 8h+7 ----------------
// This kernel's batching of the gathers around the shared per-level stages (level_cell, interp_corners, quad_corner), for the two
// derived table layouts (field.hip, kLayoutQuad / kLayoutPad: no clamp, no wrap bookkeeping): the gathers of kGridBatch levels are
// issued back to back before any is consumed.  s_lv: the levels' LDS copy (levels_to_lds).  Leaves the 8 x 2 features as packed pairs
// in gfw, zeros for a point outside the grid.
template <int LAYOUT, int kGridBatch>
__device__ __forceinline__ void grid_encode(const uint4 (&s_lv)[16][2], const unsigned char *__restrict__ table_bytes, const float (&u)[3], uint32_t h,
                                            uint32_t (&gfw)[2][4]) {
    static_assert(LAYOUT == kLayoutQuad || LAYOUT == kLayoutPad, "built for the derived layouts");
    const bool oob = out_of_grid(u);
    #pragma unroll
    for (int lb = 0; lb < 8 / kGridBatch; lb++) {
        float pos[kGridBatch][3];
        uint4 got[kGridBatch][2];   // QUAD: the cell's two blocks (z, z + 1); PAD: its four (x, x + 1) row pairs as .xy / .zw
        #pragma unroll
        for (int lq = 0; lq < kGridBatch; lq++) {
            const uint4 k0 = s_lv[8 * h + lb * kGridBatch + lq][0], k1 = s_lv[8 * h + lb * kGridBatch + lq][1];
            const uint32_t base = level_cell(k0, k1, u, pos[lq], oob);
            if constexpr (LAYOUT == kLayoutQuad) {
                // (uniform 64-bit base + 32-bit byte offset: the host refuses tables of 2^28 blocks or more)
                __builtin_memcpy(&got[lq][0], table_bytes + ((k0.x + (base & k1.x)) << 4), 16);
                __builtin_memcpy(&got[lq][1], table_bytes + ((k0.x + ((base + k0.z) & k1.x)) << 4), 16);
            } else {
                #pragma unroll
                for (uint32_t c = 0; c < 4; c++) {
                    const uint32_t row = (base + ((c & 1u) ? k0.y : 0u) + ((c & 2u) ? k0.z : 0u)) & k1.x;
                    uint2 pair;
                    __builtin_memcpy(&pair, table_bytes + ((k0.x + row) << 2), 8);   // 4-byte aligned 8-byte gather: rows (row, row + 1)
                    if (c & 1u) { got[lq][c >> 1].z = pair.x; got[lq][c >> 1].w = pair.y; }
                    else { got[lq][c >> 1].x = pair.x; got[lq][c >> 1].y = pair.y; }
                }
            }
        }
        #pragma unroll
        for (int lq = 0; lq < kGridBatch; lq++) {
            const int li = lb * kGridBatch + lq;
            // either way got[lq][z] = {(x, y), (x+1, y), (x, y+1), (x+1, y+1)}: the QUAD block's own order
            const uint32_t feat = interp_corners(pos[lq], [&](uint32_t idx) { return quad_corner(got[lq], idx); });
            gfw[li >> 2][li & 3] = oob ? 0u : feat;
        }
        // keep the batches apart (the next batch's gathers above this batch's interpolation would double the live registers)
        if (lb + 1 < 8 / kGridBatch) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---------------- sigma net: 32 -> 64 (ReLU) -> 64, no bias; hv[0] = the density coefficients, hv[1] = geo_feat ----------------
// GEO = false (the density-grid query, which has no consumer for geo_feat): output tile 1 of the last layer is not computed
template <bool GEO = true>
__device__ __forceinline__ void sigma_net(const unsigned char *w, const half8 (&gf)[2], uint32_t lane, f32x16 (&hv)[2]) {
    f32x16 s0[2];
    small_layer<2, 2>(w, kBlkS0, gf, s0, lane);
    half8 sf[4];
    relu_frags(s0, sf);
    small_layer<GEO ? 2 : 1, 4>(w, kBlkS1, sf, hv, lane);
}

// `h[:, lo : lo + 8 n] @ basis` as autocast runs it: an fp16 matrix-vector product -- fp16 operands (the Linear's output rounded to
// fp16, the basis row's fp16 values), exact products, fp32 accumulation, the result rounded to fp16.  The lane holds n groups of four
// consecutive features of every eight (registers r0 .. r0 + 4 n - 1); its lane-half partner holds the others.
template <int N>
__device__ __forceinline__ float basis_dot(const f32x16 &t, int r0, const float *basis, uint32_t h) {
    float s = 0.0f;
    #pragma unroll
    for (int r = 0; r < 4 * N; r++) s = __builtin_fmaf(round_h(t[r0 + r]), basis[8 * (r >> 2) + 4 * h + (r & 3)], s);
    s += __shfl_xor(s, 32, 64);
    return round_h(s);
}

// ---------------- density: trunc_exp(h[:, :32] @ sigma_basis) ----------------
__device__ __forceinline__ float density(const f32x16 &coef, const float *row, uint32_t h, float density_scale) {
    return density_of_logit(basis_dot<4>(coef, 0, row, h), density_scale);
}

// ---------------- colour net: [SH(16) ++ geo_feat(32)] -> 64 -> 64 -> 24, no bias ----------------
// k-step 0 of its first layer is the SH operand, k-steps 1 and 2 are geo_feat, raw, in accumulator order
__device__ __forceinline__ f32x16 colour_net(const unsigned char *w, half8 sh, const f32x16 &geo, uint32_t lane) {
    half8 cf[3] = {sh};
    acc_to_frags<false>(geo, cf[1], cf[2]);
    f32x16 c0[2], c1[2], co;
    small_layer<2, 3>(w, kBlkC0, cf, c0, lane);
    half8 f[4];
    relu_frags(c0, f);
    small_layer<2, 4>(w, kBlkC1, f, c1, lane);
    relu_frags(c1, f);
    small_layer<1, 4>(w, kBlkC2, f, &co, lane);
    return co;
}
// sigmoid(h.view(-1, 3, 8) @ color_basis): coefficient k of colour c is output row 8 c + k = register 4 c + k % 4 of lane-half k / 4
__device__ __forceinline__ void store_sigma_rgb(const FieldArgs &P, uint32_t p, float sigma, const f32x16 &co, const float *row, uint32_t h, bool store) {
    float rgb[3];
    #pragma unroll
    for (int c = 0; c < 3; c++) rgb[c] = rgb_of_logit(basis_dot<1>(co, 4 * c, row + kRowColour, h));
    if (!store) return;
    P.sigmas[p] = sigma;
    #pragma unroll
    for (int c = 0; c < 3; c++) P.rgbs[(size_t)p * 3 + c] = rgb[c];
}

}  // namespace sdn_basis
