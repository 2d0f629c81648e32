// The fused field network on fp32 MFMAs (field_f32_net.h has the network and the mapping).  The fp16 kernel (field.hip) reproduces
// autocast's half roundings and cannot meet a 1e-4 bar against the fp32 network; this one can: every product and sum is fp32
// (v_mfma_f32_32x32x2_f32).  It is also the fp32 density-grid query (CELLS).
// The operand policy (Fp32Mfma: operand layout, packing order, how the encodings are dealt to the lanes) is field_f32_mfma.h,
// shared with the temporal-basis model's fp32 kernel (field_basis_f32.hip).
//
// Bound: 1 920 MFMAs of 64 cycles per 32 points = 123 K matrix-pipe cycles per wave-tile (fp32 MFMA peak 157 TFLOP/s dense on MI355X);
// 235 520 FLOP per point as in the fp16 kernel.
#include "field_f32_mfma.h"

namespace {

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
