// The network of the temporal-basis model's fp32 fused field kernel (field_basis_f32.hip) over the lane layout and the operand policy
// of the fp32 kernels (field_f32_net.h, field_f32_mfma.h): a wave owns 32 points, both lane halves h = lane / 32 hold point
// n = lane % 32, accumulator register v of output tile mt holds row 32 mt + 8 (v / 4) + 4 h + v % 4.
//
// Weights: ONE resident stage of floats, [pair][lane][m-tile] blocks in the order S0 | S1 | C0 | C1 | C2 (dnerf_amd/fused_basis.py:
// pack_weights_f32):
//   S0  16 pairs x 2 tiles   pair l = the two channels of grid level l
//   S1  32 pairs x 2 tiles   accumulator pairs; output tile 0 = the 32 density coefficients, tile 1 = geo_feat (raw)
//   C0  24 pairs x 2 tiles   pairs 0..7 = SH coefficients (2p, 2p + 1), pairs 8..23 = registers 0..15 of S1's output tile 1
//   C1  32 pairs x 2 tiles   accumulator pairs
//   C2  32 pairs x 1 tile    accumulator pairs; rows 24..31 zero
#pragma once
#include "field_f32_mfma.h"

namespace sdn_basis_f32 {

using namespace sdn_f32;

constexpr int kS0 = 0, kS1 = kS0 + 16 * 64 * 2, kC0 = kS1 + 32 * 64 * 2, kC1 = kC0 + 24 * 64 * 2, kC2 = kC1 + 32 * 64 * 2;
constexpr int kTotalFloats = kC2 + 32 * 64;        // 15 360 floats = 60 KiB
static_assert(kTotalFloats <= kStageFloats, "one resident stage");
constexpr int kRowColour = 32;                     // the basis row: sigma_basis in 0..31, color_basis in 32..39
// floats a launch keeps in LDS: the density query reads the sigma net only
constexpr int resident_floats(bool cells) { return cells ? kC0 : kTotalFloats; }

// `coefficients . basis` over the rows of one output tile: register r0 + r of lane half h holds row 8 (r / 4) + 4 h + r % 4 of the
// N groups of eight rows that start at register r0; a per-lane partial sum in register order, then the other half's partial.  (The
// reference's fp32 GEMV has no defined summation order; this one is fixed, and the same in both kernels.)
template <int N>
__device__ __forceinline__ float basis_dot(const float16_t &t, int r0, const float *basis, uint32_t h) {
    float s = 0.0f;
    #pragma unroll
    for (int r = 0; r < 4 * N; r++) s = __builtin_fmaf(t[r0 + r], basis[8 * (r >> 2) + 4 * h + (r & 3)], s);
    return s + __shfl_xor(s, 32, 64);
}

// CELLS: the density-grid query (dnerf/renderer.py:453-555) without -O, as field_f32_net.h's: slot p is a Morton cell index, the point
// is the cell's jittered centre, the kernel stops behind the density contraction and writes sigma * density_scale only; the colour net,
// SH and geo_feat (S1's output tile 1: its MFMAs have no consumer) are compiled out, tile 0's instruction sequence is the forward's.
// s_w: resident_floats(CELLS) floats; s_bias: the frames' basis rows (kMaxFrames * 128).
template <class Ops, bool CELLS>
__device__ __forceinline__ void field_net(const F32Args &P, const LevelParams &lp, float *s_w, float *s_bias) {
    constexpr int kResident = resident_floats(CELLS);
    Point pt;
    if (!load_point<CELLS>(P, pt)) return;                           // workgroup-uniform, before any barrier
    const uint32_t lane = pt.lane, h = pt.h, slot = pt.slot;
    const bool valid = pt.valid;
    const Pre pre = stage_prefetch<kResident>(P.weights);            // all weights: in flight under the grid gathers
    for (uint32_t k = threadIdx.x; k < P.n_frames * 128u; k += 64 * kWaves) s_bias[k] = P.bias0[k];

    // ---- sigma network: grid(x) -> 64 -> 32 coefficients ++ 32 geo_feat (nothing deforms) ----
    float b16[16];
    {
        float in[3];
        bool oob = false;
        #pragma unroll
        for (int k = 0; k < 3; k++) {
            in[k] = (pt.x[k] + P.bound) / (2 * P.bound);        // grid.py:149
            if (in[k] < 0 || in[k] > 1) oob = true;
        }
        Ops::deal_grid(P.table, lp, in, oob, h, b16);
    }
    stage_commit<kResident>(s_w, pre);                               // the workgroup's only barrier pair (it covers s_bias too)
    const float *row = s_bias + pt.fr * 128u;
    float16_t a2[2];
    zero(a2);
    Ops::template layer<16, 2>(s_w + kS0, b16, a2, lane);
    float b32[32];
    Ops::template next<2>(a2, b32);
    zero(a2);
    Ops::template layer<32, 2>(s_w + kS1, b32, a2, lane);
    const float sigma = expf(basis_dot<4>(a2[0], 0, row, h)) * P.density_scale;      // trunc_exp's forward is exp
    if constexpr (CELLS) {
        if (valid && h == 0) P.sigmas[slot] = sigma;
        return;
    } else {
        // ---- colour network: SH(d, 4) ++ geo_feat (raw) -> 64 -> 64 -> 3 x 8 coefficients ----
        float b24[24];
        {
            float sh[16], bsh[16], *nul = nullptr;
            sdn_sh::sh_eval<4, false>(pt.d[0], pt.d[1], pt.d[2], sh, nul, nul, nul);
            Ops::deal_sh(sh, h, bsh);
            #pragma unroll
            for (int p = 0; p < 8; p++) b24[p] = bsh[p];
            #pragma unroll
            for (int v = 0; v < 16; v++) b24[8 + v] = a2[1][v];      // pairs of geo_feat (g, g + 4), g = 8 (v / 4) + v % 4
        }
        zero(a2);
        Ops::template layer<24, 2>(s_w + kC0, b24, a2, lane);
        Ops::template next<2>(a2, b32);
        zero(a2);
        Ops::template layer<32, 2>(s_w + kC1, b32, a2, lane);
        Ops::template next<2>(a2, b32);
        float16_t a1[1];
        zero(a1);
        Ops::template layer<32, 1>(s_w + kC2, b32, a1, lane);
        // coefficient j of colour c is output row 8 c + j = register 4 c + j % 4 of lane half j / 4
        float rgb[3];
        #pragma unroll
        for (int c = 0; c < 3; c++) rgb[c] = 1.0f / (1.0f + expf(-basis_dot<1>(a1[0], 4 * c, row + kRowColour, h)));
        if (valid && h == 0) {
            P.sigmas[slot] = sigma;
            #pragma unroll
            for (int c = 0; c < 3; c++) P.rgbs[(size_t)slot * 3 + c] = rgb[c];
        }
    }
}

}  // namespace sdn_basis_f32
