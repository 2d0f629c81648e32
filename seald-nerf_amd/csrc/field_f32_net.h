// The network of the two fp32 fused field kernels, written once: sigma and rgb of sample points in one launch (the reference WITHOUT
// `-O`: dnerf/network.py:123-169 in float32), fp32 weights, fp32 table, activations on chip, the encoders the fp32 operators' own
// expressions (freqencoder.cu:30-58 with its phase-shifted sine, gridencoder.cu:87-245, shencoder.cu:49-121 through sh_eval.h).
// field_f32.hip (Fp32Mfma: fp32 MFMAs) and field_f32x3.hip (SplitF16: fp32 operands as hi + lo fp16 pairs) give it an operand policy.
//
// Mapping.  A workgroup is 4 waves (two workgroups per CU, out of step with each other: one encodes while the other multiplies; 8 waves
// in one workgroup measured 3 % slower), a wave owns 32 points (N of the MFMA) from its encodings to its outputs and never talks to another
// wave; the workgroup shares the WEIGHTS: each layer's A operands are staged once in LDS (64 KiB for a 128 x 128 layer) and read by
// all its waves, the next stage travelling under the layer (field_f32_common.h).  Both lane halves h = lane / 32 hold point
// n = lane % 32.  A 32 x 32 MFMA leaves C[row = 8 (v / 4) + 4 h + v % 4][n] in accumulator register v, and the policy's k-order makes
// the accumulator registers of one layer the B operands of the next: activations never leave the register file and are never permuted;
// that k-order is baked into the weight packing, and the policy deals the three encodings to the lanes in it.
//
// An operand policy `Ops` holds what differs between the kernels:
//   Operand, kPerOperand         one register-resident piece of a B operand and the k positions it covers: N(K) = K / kPerOperand
//   kT_D7 .. kT_C2               offsets of the layers inside the tail stage
//   layer<N, MT>(s_w, b, acc, lane)      N operands against the staged A operands, MT output tiles of 32 rows
//   next<MT>(acc, b)             ReLU of MT accumulator tiles as the next layer's 32 MT inputs
//   deal_freq / deal_grid / deal_geo / deal_sh      the encodings in the packing's k-order (deal_grid gathers its levels with trilinear())
//   kScaled, kAccScale, kAccToOut        accumulators hold kAccScale times a layer's output, kAccToOut brings an output back; unused
//                                        (compiled out) when !kScaled
#pragma once
#include "field_f32_common.h"

namespace sdn_f32 {

template <int MT>
__device__ __forceinline__ void zero(float16_t (&acc)[MT]) {
    #pragma unroll
    for (int mt = 0; mt < MT; mt++)
        #pragma unroll
        for (int v = 0; v < 16; v++) acc[mt][v] = 0.0f;
}

// One level of the hash grid at normalised position `in`: the trilinear blend of its eight corners, channel h into r0 (BOTH: channels
// 0 and 1 into r0 and r1); zeros when the point lies outside the grid.
template <bool BOTH>
__device__ __forceinline__ void trilinear(const float *table, const LevelParams &lp, uint32_t level, const float (&in)[3], bool oob, uint32_t h,
                                          float &r0, float &r1) {
    const float *grid = table + (size_t)lp.offset[level] * 2;
    const uint32_t hashmap_size = lp.hashmap_size[level], resolution = lp.resolution[level];
    const float scale = lp.scale[level];
    float pos[3];
    uint32_t pg[3];
    #pragma unroll
    for (int k = 0; k < 3; k++) {
        pos[k] = in[k] * scale + 0.5f;
        pg[k] = (uint32_t)floorf(pos[k]);
        pos[k] -= (float)pg[k];
    }
    r0 = 0; r1 = 0;
    if (!oob) {
        std::conditional_t<BOTH, float2, float> vals[8];
        float ws[8];
        #pragma unroll
        for (uint32_t idx = 0; idx < 8; idx++) {
            float w = 1;
            uint32_t pgl[3];
            #pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                w *= (idx & (1u << k)) ? pos[k] : 1 - pos[k];
                pgl[k] = pg[k] + ((idx >> k) & 1u);
            }
            ws[idx] = w;
            const uint32_t at = sdn_grid::grid_index<3, 2>(1u, false, hashmap_size, resolution, pgl);      // tiled grid
            if constexpr (BOTH) vals[idx] = *reinterpret_cast<const float2 *>(grid + at);
            else vals[idx] = grid[at + h];
        }
        #pragma unroll
        for (uint32_t idx = 0; idx < 8; idx++) {
            if constexpr (BOTH) { r0 = r0 + ws[idx] * vals[idx].x; r1 = r1 + ws[idx] * vals[idx].y; }
            else r0 = r0 + ws[idx] * vals[idx];
        }
    }
}

// an accumulator register as the layer's output
template <class Ops>
__device__ __forceinline__ float acc_out(float a) {
    if constexpr (Ops::kScaled) return a * Ops::kAccToOut;
    else return a;
}

// CELLS: the density-grid query of update_extra_state (dnerf/renderer.py:453-555) without -O: slot p is a Morton cell index, the point is
// the cell's jittered centre (cell_points.h), the kernel stops behind the sigma network and writes sigma * density_scale only.
// s_w: one stage of weights (kStageFloats); s_bias: the frames' time-encoding bias rows (D0's initial accumulators, kMaxFrames * 128).
template <class Ops, bool CELLS>
__device__ __forceinline__ void field_net(const F32Args &P, const LevelParams &lp, float *s_w, float *s_bias) {
    using Operand = typename Ops::Operand;
    constexpr int N128 = 128 / Ops::kPerOperand, N64 = 64 / Ops::kPerOperand, N32 = 32 / Ops::kPerOperand;
    Point pt;
    if (!load_point<CELLS>(P, pt)) return;                           // workgroup-uniform, before any barrier
    const uint32_t lane = pt.lane, h = pt.h, n = pt.n, slot = pt.slot, fr = pt.fr;
    const bool valid = pt.valid, canonical = pt.canonical;
    float x[3] = {pt.x[0], pt.x[1], pt.x[2]}, d[3] = {pt.d[0], pt.d[1], pt.d[2]};
    Pre pre = stage_prefetch<kD0Floats>(P.weights + kD0);            // (see field_f32_common.h: the next stage travels under the layer)
    for (uint32_t k = threadIdx.x; k < P.n_frames * 128u; k += 64 * kWaves) s_bias[k] = P.bias0[k];

    // ---- deformation network: freq(x, 10) (time part folded into bias0) -> 128 x 7 -> 3 ----
    Operand b128[N128];
    Ops::deal_freq(x, h, b128);                                      // (the 64 inputs: its first N64 operands)
    float16_t acc[4];
    stage_commit<kD0Floats>(s_w, pre);
    pre = stage_prefetch<kStageFloats>(P.weights + kD1);
    #pragma unroll
    for (int mt = 0; mt < 4; mt++)
        #pragma unroll
        for (int v = 0; v < 16; v++) {
            const float b = s_bias[fr * 128u + mt * 32 + (v >> 2) * 8 + h * 4 + (v & 3)];
            if constexpr (Ops::kScaled) acc[mt][v] = b * Ops::kAccScale;
            else acc[mt][v] = b;
        }
    {
        Operand b0[N64];
        #pragma unroll
        for (int p = 0; p < N64; p++) b0[p] = b128[p];
        Ops::template layer<N64, 4>(s_w, b0, acc, lane);
    }
    #pragma unroll 1
    for (int l = 0; l < 6; l++) {
        Ops::template next<4>(acc, b128);
        stage_commit<kStageFloats>(s_w, pre);                                                     // D(l+1), fetched under the previous layer
        pre = stage_prefetch<kStageFloats>(P.weights + kD1 + (size_t)(l + 1) * kStageFloats);      // D(l+2); after D6 the tail stage (kTail follows D6)
        zero(acc);
        Ops::template layer<N128, 4>(s_w, b128, acc, lane);
    }
    Ops::template next<4>(acc, b128);
    stage_commit<kStageFloats>(s_w, pre);
    float16_t a1[1];
    zero(a1);
    Ops::template layer<N128, 1>(s_w + Ops::kT_D7, b128, a1, lane);
    // rows 0..2 of the output live in registers 0..2 of the lower lane half; the upper half evaluates the same point
    if (P.deform && valid && h == 0) {      // dnerf/network.py:139-141: `deform = zeros` on the canonical frame
        #pragma unroll
        for (int k = 0; k < 3; k++) P.deform[(size_t)slot * 3 + k] = canonical ? 0.0f : acc_out<Ops>(a1[0][k]);
    }
    #pragma unroll
    for (int k = 0; k < 3; k++) {
        const float dk = acc_out<Ops>(__shfl(a1[0][k], (int)n, 64));
        if (!canonical) x[k] = x[k] + dk;
    }

    // ---- sigma network: grid(x') -> 64 -> 16 ----
    Operand b32[N32];
    {
        float in[3];
        bool oob = false;
        #pragma unroll
        for (int k = 0; k < 3; k++) {
            in[k] = (x[k] + P.bound) / (2 * P.bound);            // grid.py:149
            if (in[k] < 0 || in[k] > 1) oob = true;
        }
        Ops::deal_grid(P.table, lp, in, oob, h, b32);
    }
    float16_t a2[2];
    zero(a2);
    Ops::template layer<N32, 2>(s_w + Ops::kT_S0, b32, a2, lane);
    Operand b64[N64];
    Ops::template next<2>(a2, b64);
    zero(a1);
    Ops::template layer<N64, 1>(s_w + Ops::kT_S1, b64, a1, lane);
    const float sigma = expf(acc_out<Ops>(a1[0][0])) * P.density_scale;     // row 0 (lower half); trunc_exp's forward is exp
    if constexpr (CELLS) {                                    // (every barrier of the workgroup lies behind this wave)
        if (valid && h == 0) P.sigmas[slot] = sigma;
        return;
    }

    // ---- colour network: SH(d, 4) ++ geo_feat (the sigma net's rows 1..15, raw; row 0's weights are zero) -> 64 -> 64 -> 3 ----
    {
        float sh[16], *nul = nullptr;
        Ops::deal_geo(a1[0], b32);
        sdn_sh::sh_eval<4, false>(d[0], d[1], d[2], sh, nul, nul, nul);
        Ops::deal_sh(sh, h, b32);
    }
    zero(a2);
    Ops::template layer<N32, 2>(s_w + Ops::kT_C0, b32, a2, lane);
    Ops::template next<2>(a2, b64);
    zero(a2);
    Ops::template layer<N64, 2>(s_w + Ops::kT_C1, b64, a2, lane);
    Ops::template next<2>(a2, b64);
    zero(a1);
    Ops::template layer<N64, 1>(s_w + Ops::kT_C2, b64, a1, lane);
    if (valid && h == 0) {
        P.sigmas[slot] = sigma;
        #pragma unroll
        for (int k = 0; k < 3; k++) P.rgbs[(size_t)slot * 3 + k] = 1.0f / (1.0f + expf(acc_out<Ops>(-a1[0][k])));
    }
}

// The one host launcher: the kernel's arguments from the call (and, for a CELLS kernel, the cell -> point constants), the launch, its status.
template <class Kernel>
int launch_field(Kernel kernel, const sdn_int::FieldCall &f, const sdn_int::FieldCells *q, hipStream_t st) {
    LevelParams lp;
    F32Args a;
    int rc = fill_args(a, lp, f);
    if (rc) return rc;
    if (q) {
        a.cell_noise = q->noise; a.cell_seed = q->seed;
        const float half_grid = q->cas_bound / (float)q->grid_size;
        a.cell_inv = 1.0f / (float)(q->grid_size - 1); a.cell_span = q->cas_bound - half_grid; a.cell_half = half_grid;
    }
    hipLaunchKernelGGL(kernel, dim3(sdn_div_up(f.M, (uint32_t)kPointsPerWG)), dim3(64 * kWaves), 0, st, a, lp);
    return sdn_launch_status();
}

}  // namespace sdn_f32
