// The stages the ambient-dimension field (dnerf/network_hyper.py under `-O`) adds to those of field_f16_net.h, over the same lane layout:
// a wave owns 32 points, lane-half h = lane / 32 holds point n = lane % 32, and register r of an accumulator tile mt holds output
// feature 32 mt + 8 (r / 4) + 4 h + r % 4.  The model has no deformation network: a 4-D tiled grid over (x, y, z, ambient(t)) feeds a
// sigma net that emits the density logit and 32 geo_feat, and a colour net emits the three colour logits.  The ambient coordinate -- the
// output of a 5-layer MLP of the time stamp alone, computed on the host -- is entry 0 of the frame's constants row.
#pragma once
#include "field_f16_net.h"

namespace sdn_hyper {

using namespace sdn_f16;

// fragment (1 KiB block) indices inside the packed weight buffer (dnerf_amd/fused_hyper.py); all of it stays resident in LDS
constexpr int kBlkS0 = 0;              // 32 -> 64: 2 Mt x 2 ks
constexpr int kBlkS1 = kBlkS0 + 4;     // 64 -> 33, rows permuted by the packer (tile 0 = geo_feat, row 0 of tile 1 = the density logit): 2 Mt x 4 ks
constexpr int kBlkC0 = kBlkS1 + 8;     // [SH(16) ++ geo_feat(32)] -> 64: 2 Mt x 3 ks
constexpr int kBlkC1 = kBlkC0 + 6;     // 64 -> 64: 2 Mt x 4 ks
constexpr int kBlkC2 = kBlkC1 + 8;     // 64 -> 3 (rows 3..31 of the tile are zero): 1 Mt x 4 ks
constexpr int kBlkTotal = kBlkC2 + 4;  // 30
// the density-grid query's LDS copy holds S0 and, right behind it, the logit tile of S1 (source blocks kBlkS1 + 4 .. kBlkS1 + 7)
constexpr int kBlkS1Logit = kBlkS0 + 4;
constexpr int kBlkCellsTotal = kBlkS1Logit + 4;  // 8

// tiled-grid level constants for D = 4: the 3-D kernels' record (their view of it is unchanged) and the row stride of +1 along the
// fourth coordinate (0 if the level's index drops it: gridencoder.cu:72)
struct HyperLevels {
    TiledLevels lv;
    uint32_t s3[16];
};

// per grid level in LDS: {offset, s1, s2, hsize}, {mask, scale, s3, -}; visible after the caller's next barrier
__device__ __forceinline__ void levels_to_lds(uint4 (*s_lv)[2], const HyperLevels &hl) {
    if (threadIdx.x < 16) {
        const uint32_t l = threadIdx.x;
        s_lv[l][0] = make_uint4(hl.lv.offset[l], hl.lv.s1[l], hl.lv.s2[l], hl.lv.hsize[l]);
        s_lv[l][1] = make_uint4(hl.lv.mask[l], __float_as_uint(hl.lv.scale[l]), hl.s3[l], 0u);
    }
}

// GridEncoder.forward (grid.py:149) on one coordinate: (x + bound) / (2 bound), grid_coords' expression
__device__ __forceinline__ float unit_coord(float x, const FieldArgs &P) {
    return P.inv_2bound != 0.0f ? (x + P.bound) * P.inv_2bound : (x + P.bound) / (2 * P.bound);
}

// The fourth coordinate is the same for every point of a frame: thread 16 f + l works out level l of frame f once per workgroup --
// {pos_grid[3] * s3 (the coordinate's share of the row index; 0 where the level drops it), the fraction's bits} -- with level_cell's
// expressions (cell <= 2049 and stride <= the level's rows <= 2^24, which the host checks: the 24-bit product is the uint32 one).
// A frame whose ambient coordinate lies outside the grid gets {0, 0}: its points are zeroed by the range test.
__device__ __forceinline__ void ambient_to_lds(uint2 (*s_w)[16], const HyperLevels &hl, const FieldArgs &P) {
    if (threadIdx.x < 16u * P.n_frames) {
        const uint32_t f = threadIdx.x >> 4, l = threadIdx.x & 15u;
        const float u3 = unit_coord(P.bias0[128u * f], P);
        const float q = u3 * hl.lv.scale[l] + 0.5f;
        const bool out = (u3 < 0) | (u3 > 1);
        s_w[f][l] = out ? make_uint2(0u, 0u) : make_uint2(__umul24((uint32_t)q, hl.s3[l]), __float_as_uint(__builtin_amdgcn_fractf(q)));
    }
}

// kernel_grid's interpolation for D = 4 (gridencoder.cu:166-189, scalar_t = at::Half): the 16 corners in the reference's order -- bit d
// of idx selects coordinate d, the fourth coordinate is bit 3 -- the weight the product of four factors in coordinate order, each
// corner's product rounded to half and each partial sum rounded to half (interp_corners of field_f16_net.h, one dimension more).
template <typename Corner>
__device__ __forceinline__ uint32_t interp_corners4(const float (&fr)[4], Corner corner_bits) {
    half2v accv = {(_Float16)0.0f, (_Float16)0.0f};
    #pragma unroll
    for (uint32_t idx = 0; idx < 16; idx++) {
        float w = 1;
        #pragma unroll
        for (uint32_t d = 0; d < 4; d++) w *= (idx & (1u << d)) ? fr[d] : 1 - fr[d];
        const uint32_t bits = corner_bits(idx);
        const half2v t = {(_Float16)mix_mul_lo(w, bits), (_Float16)mix_mul_hi(w, bits)};
        accv = accv + t;
    }
    return __builtin_bit_cast(uint32_t, accv);
}

// ---------------- grid encode: lane-half h evaluates levels 8h .. 8h+7 ----------------
// This kernel's batching of the gathers, for the two derived table layouts: the gathers of kGridBatch levels are issued back to back
// before any is consumed.  A level's cell is four QUAD blocks -- (z, w), (z + 1, w), (z, w + 1), (z + 1, w + 1), each the four (x, y)
// corners -- or, in PAD, sixteen (x, x + 1) row pairs.  Where the level's index drops the fourth coordinate (s3 == 0) corners idx and
// idx + 8 are the same row: the w + 1 half is not gathered, its corners read the w half, and all sixteen rounded accumulations remain.
// s_lv: the levels' LDS copy; s_wf: the fourth coordinate's per-level record of the point's frame (ambient_to_lds).  Leaves the 8 x 2
// features as packed pairs in gfw, zeros for a point outside the grid.
template <int LAYOUT, int kGridBatch>
__device__ __forceinline__ void grid_encode(const uint4 (&s_lv)[16][2], const uint2 *s_wf, const unsigned char *__restrict__ table_bytes,
                                            const float (&u)[3], bool oob, uint32_t h, uint32_t (&gfw)[2][4]) {
    static_assert(LAYOUT == kLayoutQuad || LAYOUT == kLayoutPad, "built for the derived layouts");
    #pragma unroll
    for (int lb = 0; lb < 8 / kGridBatch; lb++) {
        float pos[kGridBatch][4];
        uint4 got[kGridBatch][4];   // block zw = {(x, y), (x+1, y), (x, y+1), (x+1, y+1)} at (z + (zw & 1), w + (zw >> 1))
        bool four[kGridBatch];
        #pragma unroll
        for (int lq = 0; lq < kGridBatch; lq++) {
            const uint32_t l = 8 * h + lb * kGridBatch + lq;
            const uint4 k0 = s_lv[l][0], k1 = s_lv[l][1];
            const uint2 kw = s_wf[l];
            float p3[3];
            const uint32_t base = level_cell(k0, k1, u, p3, oob) + (oob ? 0u : kw.x);
            pos[lq][0] = p3[0]; pos[lq][1] = p3[1]; pos[lq][2] = p3[2]; pos[lq][3] = __uint_as_float(kw.y);
            four[lq] = k1.z != 0u;
            auto block = [&](uint32_t zw) {
                const uint32_t first = base + ((zw & 1u) ? k0.z : 0u) + ((zw & 2u) ? k1.z : 0u);
                uint4 g;
                if constexpr (LAYOUT == kLayoutQuad) {
                    // (uniform 64-bit base + 32-bit byte offset: the host refuses tables of 2^28 blocks or more)
                    __builtin_memcpy(&g, table_bytes + ((k0.x + (first & k1.x)) << 4), 16);
                } else {
                    uint2 lo, hi;   // 4-byte aligned 8-byte gathers: rows (row, row + 1)
                    __builtin_memcpy(&lo, table_bytes + ((k0.x + (first & k1.x)) << 2), 8);
                    __builtin_memcpy(&hi, table_bytes + ((k0.x + ((first + k0.y) & k1.x)) << 2), 8);
                    g = make_uint4(lo.x, lo.y, hi.x, hi.y);
                }
                return g;
            };
            got[lq][0] = block(0);
            got[lq][1] = block(1);
            got[lq][2] = got[lq][3] = make_uint4(0u, 0u, 0u, 0u);
            if (four[lq]) {
                got[lq][2] = block(2);
                got[lq][3] = block(3);
            }
        }
        #pragma unroll
        for (int lq = 0; lq < kGridBatch; lq++) {
            const int li = lb * kGridBatch + lq;
            // the w + 1 half: gathered, or the w half again (both candidates pinned in VGPRs: otherwise the select of two array
            // elements becomes one dynamically indexed load and the gathered blocks are demoted to scratch)
            uint32_t up[2][4];
            #pragma unroll
            for (int z = 0; z < 2; z++) {
                const uint32_t lo[4] = {got[lq][z].x, got[lq][z].y, got[lq][z].z, got[lq][z].w};
                const uint32_t hi[4] = {got[lq][2 + z].x, got[lq][2 + z].y, got[lq][2 + z].z, got[lq][2 + z].w};
                #pragma unroll
                for (int c = 0; c < 4; c++) {
                    uint32_t a = lo[c], b = hi[c];
                    asm volatile("" : "+v"(a), "+v"(b));
                    up[z][c] = four[lq] ? b : a;
                }
            }
            const uint4 (&g)[4] = got[lq];
            const uint32_t feat = interp_corners4(pos[lq], [&](uint32_t idx) {
                const uint32_t c = idx & 3u, zw = idx >> 2;
                if (zw >= 2u) return up[zw - 2u][c];
                const uint4 &q = g[zw];
                return c == 0u ? q.x : (c == 1u ? q.y : (c == 2u ? q.z : q.w));
            });
            gfw[li >> 2][li & 3] = oob ? 0u : feat;
        }
        // keep the batches apart (the next batch's gathers above this batch's interpolation would double the live registers)
        if (lb + 1 < 8 / kGridBatch) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---------------- sigma net: 32 -> 64 (ReLU) -> 33, no bias; hv[0] = geo_feat, row 0 of hv[1] = the density logit ----------------
// GEO = false (the density-grid query, which has no consumer for geo_feat): output tile 0 of the last layer is not computed, hv[0] is
// left unset, and `w` is the query's short copy, where the logit tile's fragments start at kBlkS1Logit
template <bool GEO = true>
__device__ __forceinline__ void sigma_net(const unsigned char *w, const half8 (&gf)[2], uint32_t lane, f32x16 (&hv)[2]) {
    f32x16 s0[2];
    small_layer<2, 2>(w, kBlkS0, gf, s0, lane);
    half8 sf[4];
    relu_frags(s0, sf);
    if constexpr (GEO) small_layer<2, 4>(w, kBlkS1, sf, hv, lane);
    else small_layer<1, 4>(w, kBlkS1Logit, sf, &hv[1], lane);
}

// ---------------- colour net: [SH(16) ++ geo_feat(32)] -> 64 -> 64 -> 3, no bias ----------------
// k-step 0 of its first layer is the SH operand, k-steps 1 and 2 are geo_feat, raw, in accumulator order; rows 0..2 of the result are
// the colour logits (store_sigma_rgb of field_f16_net.h reads them)
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

}  // namespace sdn_hyper
