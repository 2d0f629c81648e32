// The temporal-basis model's fused field on fp32 MFMAs: the reference's dnerf/network_basis.py:123-161 WITHOUT `-O`, sigma and rgb of
// sample points in one launch, every product and sum in fp32 (v_mfma_f32_32x32x2_f32, the Fp32Mfma policy of field_f32_mfma.h).  The
// fp16 kernel (field_basis.hip) reproduces autocast's half roundings and can only be held at fp16 distance from the fp32 network; this
// one is held to 1e-4 of it.  It is also the fp32 density-grid query of that model (CELLS).
//
//   xyz --tiled grid (16 lv x 2, fp32 table in the reference layout)--> sigma MLP (64, 64) --> 32 density coefficients . sigma_basis(t) --exp--> sigma
//                                                                                         \--> 32 geo_feat
//   dir --SH(4)--> ++ geo_feat --> colour MLP (64, 64, 24) --> 3 x 8 colour coefficients . color_basis(t) --sigmoid--> rgb
//
// Mapping: that of k_field_f32 (field_f32_net.h) -- 4 waves per workgroup, a wave owns 32 points from its encoding to its outputs, both
// lane halves h = lane / 32 hold point n = lane % 32, the accumulator registers of a layer are the B operands of the next -- and the same
// live-list / loop-record / frame-group contract (load_point, slot_frame, row fr of bias0: here the frame's BASIS row, the output of
// the model's basis_net for the time stamp, computed on the host: sigma_basis in 0..31, color_basis in 32..39).  The difference: all
// weights are 15 360 floats (60 KiB), below the one 64-KiB stage of the deformation kernels, so there is no stage pipeline: they travel
// to registers in front of the grid gathers, to LDS behind them, and stay (one barrier pair per workgroup).
//
// Bound: 240 MFMAs of 64 cycles per 32 points = 15 K matrix-pipe cycles per wave-tile, against the same 128 fp32 gathers per lane as
// k_field_f32; two workgroups per CU (2 x 62 KiB of LDS).  What bounds the launch was not measured.
#include "field_basis_f32_net.h"

namespace {

template <bool CELLS>
__global__ void __launch_bounds__(64 * kWaves, 8 / kWaves) k_field_basis_f32(F32Args P, LevelParams lp) {
    __shared__ __attribute__((aligned(16))) float s_w[sdn_basis_f32::resident_floats(CELLS)];
    __shared__ float s_bias[kMaxFrames * 128];
    sdn_basis_f32::field_net<Fp32Mfma, CELLS>(P, lp, s_w, s_bias);
}

// the fp32 kernels read the model's own table: level sizes are the reference's multiples of 8 rows (grid.py:124), the fp16 kernels'
// derived layouts (== 1 / 2 mod 8) are not
bool reference_layout(const int32_t *offsets_host) {
    for (int l = 0; l < 16; l++)
        if ((offsets_host[l + 1] - offsets_host[l]) % 8 != 0) return false;
    return true;
}

}  // namespace

namespace sdn_int {

int field_forward_basis_f32(const FieldCall &f, hipStream_t st) {
    if (!reference_layout(f.offsets_host)) return SDN_E_UNSUPPORTED;
    return sdn_f32::launch_field(k_field_basis_f32<false>, f, nullptr, st);
}

// sigma * density_scale of jittered occupancy-grid cell centres -> tmp_grid slice; q.f.bias0: the basis row of the slice's (perturbed) time
int field_cells_basis_f32(const FieldCells &q, hipStream_t st) {
    if (!reference_layout(q.f.offsets_host)) return SDN_E_UNSUPPORTED;
    return sdn_f32::launch_field(k_field_basis_f32<true>, q.f, &q, st);
}

}  // namespace sdn_int

extern "C" {

uint32_t sdn_field_basis_weight_floats_f32(void) { return (uint32_t)sdn_basis_f32::kTotalFloats; }

int sdn_field_basis_forward_f32(const float *xyzs, const float *dirs, const uint32_t *live_idx, const uint32_t *live_count, uint32_t M,
                                const float *weights, const float *basis_row, const float *table, const int32_t *offsets_host, float S, uint32_t H,
                                float bound, float density_scale, float *sigmas, float *rgbs, void *stream) {
    return sdn_int::field_forward_checked(5, {.xyzs = xyzs, .dirs = dirs, .live_idx = live_idx, .live_count = live_count, .M = M, .weights = weights,
                                              .bias0 = basis_row, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                              .density_scale = density_scale, .sigmas = sigmas, .rgbs = rgbs},
                                          stream);
}

// The density-grid query of update_extra_state for a temporal-basis model trained WITHOUT -O: sdn_density_query_cells_basis_f16 with
// the fp32 network (weights of sdn_field_basis_weight_floats_f32 floats, the model's fp32 embedding table in the reference layout).
int sdn_density_query_cells_basis_f32(const int32_t *cells, const uint32_t *cell_count, uint32_t n, const float *noise, uint32_t seed,
                                      uint32_t grid_size, float cas_bound, const float *weights, const float *basis_row, const float *table,
                                      const int32_t *offsets_host, float S, uint32_t H, float bound, float density_scale, float *tmp_slice,
                                      void *stream) {
    return sdn_int::field_cells_checked(5, {.f = {.live_idx = (const uint32_t *)cells, .live_count = cell_count, .M = n, .weights = weights,
                                                  .bias0 = basis_row, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                                  .density_scale = density_scale, .sigmas = tmp_slice},
                                            .noise = noise, .seed = seed, .grid_size = grid_size, .cas_bound = cas_bound},
                                        stream);
}

}  // extern "C"
