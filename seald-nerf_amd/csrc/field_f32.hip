// The fused field network on fp32 MFMAs (field_f32_net.h has the network and the mapping).  The fp16 kernel (field.hip) reproduces
// autocast's half roundings and cannot meet a 1e-4 bar against the fp32 network; this one can: every product and sum is fp32
// (v_mfma_f32_32x32x2_f32).  It is also the fp32 density-grid query (CELLS).
//
// Operands.  v_mfma_f32_32x32x2_f32 takes A[m = lane % 32][k = lane / 32] and B[k = lane / 32][n = lane % 32] -- one register each.  So
// accumulator register v of output tile mt IS the B operand of the next layer for the k-pair (row, row + 4), row = 32 mt + 8 (v / 4)
// + v % 4; the packing (dnerf_amd/fused_f32.py: pack_weights_f32) is [pair][lane][m-tile], so that one 16-byte LDS read feeds the four
// MFMAs of a k-pair.  The encodings come in the same shape: lane half h of point n computes feature (pair, h) -- for the frequency
// encoding the pair is (sin, cos) of one angle, i.e. ONE sinf with the reference's phase shift h * pi/2; for the grid it is the two
// channels of a level; for SH consecutive coefficients.
//
// Bound: 1 920 MFMAs of 64 cycles per 32 points = 123 K matrix-pipe cycles per wave-tile (fp32 MFMA peak 157 TFLOP/s dense on MI355X);
// 235 520 FLOP per point as in the fp16 kernel.
#include "field_f32_net.h"

namespace {

using namespace sdn_f32;

struct Fp32Mfma {
    using Operand = float;                      // one k-pair: lane half h holds k = h of it
    static constexpr int kPerOperand = 2;
    static constexpr bool kScaled = false;
    // offsets inside the tail stage (floats): [pair][lane][m-tile] blocks
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

template <bool CELLS>
__global__ void __launch_bounds__(64 * kWaves, 8 / kWaves) k_field_f32(F32Args P, LevelParams lp) {
    __shared__ __attribute__((aligned(16))) float s_w[kStageFloats];
    __shared__ float s_bias[kMaxFrames * 128];
    field_net<Fp32Mfma, CELLS>(P, lp, s_w, s_bias);
}

}  // namespace

namespace sdn_int {
int field_forward_f32(const FieldCall &f, hipStream_t st) { return sdn_f32::launch_field(k_field_f32<false>, f, nullptr, st); }

// sigma * density_scale of jittered occupancy-grid cell centres -> tmp_grid slice, fp32 network (the fp32 twin of field_cells_f16)
int field_cells_f32(const FieldCells &q, hipStream_t st) { return sdn_f32::launch_field(k_field_f32<true>, q.f, &q, st); }
}  // namespace sdn_int

extern "C" {

uint32_t sdn_field_weight_floats_f32(void) { return (uint32_t)sdn_f32::kTotalFloats; }

int sdn_field_forward_f32(const float *xyzs, const float *dirs, const uint32_t *live_idx, const uint32_t *live_count, uint32_t M,
                          const float *weights, const float *bias0, const float *table, const int32_t *offsets_host, float S, uint32_t H,
                          float bound, float density_scale, int zero_deform, float *sigmas, float *rgbs, float *deform, void *stream) {
    return sdn_int::field_forward_checked(1, {.xyzs = xyzs, .dirs = dirs, .live_idx = live_idx, .live_count = live_count, .M = M, .weights = weights,
                                              .bias0 = bias0, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                              .density_scale = density_scale, .zero_deform = zero_deform ? 1 : 0, .sigmas = sigmas, .rgbs = rgbs,
                                              .deform = deform},
                                          stream);
}

// The density-grid query of update_extra_state for a model trained WITHOUT -O: as sdn_density_query_cells_f16 with the fp32 network
// (weights of sdn_field_weight_floats_f32 floats, the model's fp32 embedding table in the reference layout).
int sdn_density_query_cells_f32(const int32_t *cells, const uint32_t *cell_count, uint32_t n, const float *noise, uint32_t seed,
                                uint32_t grid_size, float cas_bound, const float *weights, const float *bias0, const float *table,
                                const int32_t *offsets_host, float S, uint32_t H, float bound, float density_scale, int zero_deform,
                                float *tmp_slice, void *stream) {
    return sdn_int::field_cells_checked(1, {.f = {.live_idx = (const uint32_t *)cells, .live_count = cell_count, .M = n, .weights = weights, .bias0 = bias0,
                                                  .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                                  .density_scale = density_scale, .zero_deform = zero_deform ? 1 : 0, .sigmas = tmp_slice},
                                            .noise = noise, .seed = seed, .grid_size = grid_size, .cas_bound = cas_bound},
                                        stream);
}

}  // extern "C"
