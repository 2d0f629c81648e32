// The fp32-MFMA operand policy of the fp32 fused field kernels (field_f32.hip: the deformation model; field_basis_f32.hip: the
// temporal-basis model): activations and weights as they are, one v_mfma_f32_32x32x2_f32 per k-pair and output tile.
//
// Operands.  v_mfma_f32_32x32x2_f32 takes A[m = lane % 32][k = lane / 32] and B[k = lane / 32][n = lane % 32] -- one register each.  So
// accumulator register v of output tile mt IS the B operand of the next layer for the k-pair (row, row + 4), row = 32 mt + 8 (v / 4)
// + v % 4; the packing (dnerf_amd/fused_f32.py: _pack_layer) is [pair][lane][m-tile], so that one LDS read feeds the MFMAs of a
// k-pair.  The encodings come in the same shape: lane half h of point n computes feature (pair, h) -- for the frequency encoding the
// pair is (sin, cos) of one angle, i.e. ONE sinf with the reference's phase shift h * pi/2; for the grid it is the two channels of a
// level; for SH consecutive coefficients.
#pragma once
#include "field_f32_net.h"

namespace {

using namespace sdn_f32;

struct Fp32Mfma {
    using Operand = float;                      // one k-pair: lane half h holds k = h of it
    static constexpr int kPerOperand = 2;
    static constexpr bool kScaled = false;
    // offsets inside the deformation model's tail stage (floats): [pair][lane][m-tile] blocks
    static constexpr int kT_D7 = 0, kT_S0 = kT_D7 + 64 * 64, kT_S1 = kT_S0 + 16 * 64 * 2, kT_C0 = kT_S1 + 32 * 64, kT_C1 = kT_C0 + 16 * 64 * 2,
                         kT_C2 = kT_C1 + 32 * 64 * 2;
    static_assert(kT_C2 + 32 * 64 == kTailFloats && 32 * 64 * 4 == kD0Floats, "stage sizes");

    // one layer: PAIRS k-pairs of B operands (registers) against the staged A operands, MT output tiles of 32 rows
    template <int PAIRS, int MT>
    static __device__ __forceinline__ void layer(const float *s_w, const float (&b)[PAIRS], float16_t (&acc)[MT], uint32_t lane) {
        #pragma unroll
        for (int p = 0; p < PAIRS; p++) {
            float a[MT];
            const float *src = s_w + ((size_t)p * 64 + lane) * MT;
            if constexpr (MT == 4) *reinterpret_cast<float4 *>(a) = *reinterpret_cast<const float4 *>(src);
            else if constexpr (MT == 2) *reinterpret_cast<float2 *>(a) = *reinterpret_cast<const float2 *>(src);
            else a[0] = src[0];
            #pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[p], acc[mt], 0, 0, 0);
        }
    }

    template <int MT>
    static __device__ __forceinline__ void next(const float16_t (&acc)[MT], float (&b)[16 * MT]) {
        #pragma unroll
        for (int mt = 0; mt < MT; mt++)
            #pragma unroll
            for (int v = 0; v < 16; v++) b[mt * 16 + v] = relu1(acc[mt][v]);
    }

    static __device__ __forceinline__ void deal_freq(const float (&x)[3], uint32_t h, float (&b)[64]) {
        const float phase = (float)h * (3.141592653589793f / 2);      // freqencoder.cu: the cosine is the sine shifted by pi/2 in fp32
        #pragma unroll
        for (int p = 0; p < 30; p++) b[p] = sinf(scalbnf(x[p % 3], p / 3) + phase);
        b[30] = h ? x[1] : x[0];
        b[31] = h ? 0.0f : x[2];
    }
    static __device__ __forceinline__ void deal_grid(const float *table, const LevelParams &lp, const float (&in)[3], bool oob, uint32_t h,
                                                     float (&b)[16]) {
        #pragma unroll
        for (int level = 0; level < 16; level++) {
            float unused;
            trilinear<false>(table, lp, level, in, oob, h, b[level], unused);
        }
    }
    static __device__ __forceinline__ void deal_geo(const float16_t &a, float (&b)[16]) {
        #pragma unroll
        for (int v = 0; v < 8; v++) b[8 + v] = a[v];       // pairs of rows (8 (v / 4) + v % 4, + 4)
    }
    static __device__ __forceinline__ void deal_sh(const float (&sh)[16], uint32_t h, float (&b)[16]) {
        #pragma unroll
        for (int p = 0; p < 8; p++) b[p] = h ? sh[2 * p + 1] : sh[2 * p];
    }
};

}  // namespace
