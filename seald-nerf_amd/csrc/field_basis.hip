// Fused field evaluation of the temporal-basis model on MFMA for gfx950 (MI355X), inference.
//
//   xyz --tiled grid (16 lv x 2)--> sigma MLP (64, 64) --> 32 density coefficients . sigma_basis(t) --exp--> sigma
//                                                    \--> 32 geo_feat
//   dir --SH(4)--> ++ geo_feat --> colour MLP (64, 64, 24) --> 3 x 8 colour coefficients . color_basis(t) --sigmoid--> rgb
//
// Behavioural contract: NeRFNetwork.forward of the reference's dnerf/network_basis.py:123-161 under `-O` (torch autocast): every Linear
// and both contractions with the basis take fp16 operands, accumulate in fp32 and round their output to fp16; the encoders run in fp32;
// the grid table and its output are fp16 with the per-corner half rounding of kernel_grid; sigma = exp(fp32(logit)); rgb =
// fp16(sigmoid(.)).  The basis itself -- a 5-layer MLP of the time stamp alone -- is the same for every point: the host evaluates it
// once per time stamp (dnerf_amd/fused_basis.py) and hands it over as the frame's constants row, where the deformation model's kernels
// take the time encoding's bias row (FieldArgs::bias0, row slot_frame[p] in a frame group).  zero_deform is ignored: nothing deforms.
//
// Mapping: the one-tile-per-workgroup form of k_field_f16 (field.hip) -- 8 waves = 256 points, one wave = 32 points = the N dimension
// of v_mfma_f32_32x32x16_f16, weights the A operand, an accumulator converting in place into the next layer's B operand -- with two
// differences.  All weights are 30 fragments of 1 KiB: they are copied to LDS once, before the workgroup's one barrier, and stay there
// (no staging, no double buffer).  And there is no wide layer in front of the grid phase: per point 60 MFMAs stand against the same 32
// gathers (QUAD) as in the deformation model's 240, so the launch is expected to be bound by the gather-address rate and by vector
// issue, and the kernel is built for occupancy ("temporal-basis field").
#include "sdn_common.h"
#include "sdn_internal.h"
#include "cell_points.h"
#include "field_basis_net.h"

namespace {

using namespace sdn_f16;

constexpr int kWaves = 8;                 // waves per workgroup, 32 points each
constexpr int kPointsPerWG = 32 * kWaves;
constexpr int kOcc = 4;                   // waves per SIMD the kernel is compiled for: two workgroups per CU (<= 128 VGPRs, 2 x 31 KiB of LDS)
constexpr int kGridBatch = 4;             // grid levels (per lane-half) whose gathers are in flight together

// CELLS: the density-grid query of update_extra_state (dnerf/renderer.py:453-555), as k_field_f16's (field.hip): slot p is a Morton cell
//   index, the point is that cell's jittered centre (cell_points.h), no xyzs / dirs / rgbs buffer is touched, only the density is
//   evaluated -- the sigma net's geo_feat tile and the whole colour net are compiled out, and only the sigma net's 12 fragments are
//   copied to LDS -- and it is stored at sigmas[p] (a slice of tmp_grid).  One slice per launch: the basis row is row 0 of bias0.
template <int LAYOUT, bool CELLS>
__global__ void __launch_bounds__(64 * kWaves, kOcc) k_field_basis_f16(FieldArgs P, TiledLevels lv) {
    constexpr int kBlkResident = CELLS ? sdn_basis::kBlkC0 : sdn_basis::kBlkTotal;   // fragments the launch reads: S0 S1 (| C0 C1 C2)
    __shared__ __attribute__((aligned(16))) unsigned char s_w[kBlkResident * 1024];
    __shared__ __attribute__((aligned(4096))) uint4 s_lv[16][2];   // per grid level: {offset, s1, s2, hsize}, {mask, scale, -, -}
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    levels_to_lds(s_lv, lv);
    const uint32_t count = live_points(P);
    if (blockIdx.x * (uint32_t)kPointsPerWG >= count) return;  // workgroup-uniform: nothing to do, no barrier touched
    // the weights, 16 bytes per lane and step, in fragment order as they lie in memory (every workgroup reads the same 30 KiB: L2)
    for (uint32_t c = threadIdx.x; c < (uint32_t)kBlkResident * 64u; c += 64u * kWaves)
        reinterpret_cast<uint4 *>(s_w)[c] = reinterpret_cast<const uint4 *>(P.weights)[c];
    const uint32_t n = lane & 31u, h = lane >> 5;
    const uint32_t i = blockIdx.x * (uint32_t)kPointsPerWG + wave * 32u + n;
    const bool valid = i < count;
    const uint32_t ii = valid ? i : (count - 1);  // idle lanes recompute the last point and store nothing
    const uint32_t p = P.live_idx ? P.live_idx[ii] : ii;
    float x0, x1, x2, d0 = 0, d1 = 0, d2 = 0;
    const float *row = P.bias0;
    if constexpr (CELLS) {
        float xs[3];
        #pragma unroll
        for (int d = 0; d < 3; d++) {
            const float r = P.cell_noise ? P.cell_noise[(size_t)ii * 3 + d] : sdn_cells::cell_uniform(P.cell_seed, ii * 3u + (uint32_t)d);
            xs[d] = sdn_cells::cell_coord(p, d, r, P.cell_inv, P.cell_span, P.cell_half);
        }
        x0 = xs[0]; x1 = xs[1]; x2 = xs[2];
    } else {
        x0 = P.xyzs[(size_t)p * 3]; x1 = P.xyzs[(size_t)p * 3 + 1]; x2 = P.xyzs[(size_t)p * 3 + 2];
        d0 = P.dirs[(size_t)p * 3]; d1 = P.dirs[(size_t)p * 3 + 1]; d2 = P.dirs[(size_t)p * 3 + 2];
        row = P.bias0 + 128u * (P.slot_frame ? (uint32_t)P.slot_frame[p] : 0u);   // the basis row of the point's frame
    }
    float u[3];
    grid_coords(zero_tile(), lane, x0, x1, x2, true, P, u);   // canonical: the model has no deformation
    __syncthreads();  // the levels and the weights are in LDS
    uint32_t gfw[2][4];   // 8 levels x 2 features as packed pairs
    sdn_basis::grid_encode<LAYOUT, kGridBatch>(s_lv, reinterpret_cast<const unsigned char *>(P.table), u, h, gfw);
    half8 gf[2];
    grid_operand(gfw, gf);
    f32x16 hv[2];
    sdn_basis::sigma_net<!CELLS>(s_w, gf, lane, hv);
    const float sigma = sdn_basis::density(hv[0], row, h, P.density_scale);
    if constexpr (CELLS) {
        if (h == 0 && valid) P.sigmas[p] = sigma;   // duplicates in the list: any one of them wins, as with tmp_grid[indices] = sigmas
        return;
    }
    const f32x16 co = sdn_basis::colour_net(s_w, sh_operand(d0, d1, d2, h), hv[1], lane);
    sdn_basis::store_sigma_rgb(P, p, sigma, co, row, h, h == 0 && valid);
}

}  // namespace

namespace sdn_int {

// launch used by both the C entry point and the device-driven render loop (render.hip)
int field_forward_basis(const FieldCall &f, hipStream_t st) {
    TiledLevels lv;
    FieldArgs a;
    int rc = fill_field_args(a, lv, f);
    if (rc) return rc;
    const uint32_t wgs = sdn_div_up(f.M, (uint32_t)kPointsPerWG);
    const int layout = field_table_layout(f.offsets_host);
    if (layout == kLayoutQuad) hipLaunchKernelGGL((k_field_basis_f16<kLayoutQuad, false>), dim3(wgs), dim3(64 * kWaves), 0, st, a, lv);
    else if (layout == kLayoutPad) hipLaunchKernelGGL((k_field_basis_f16<kLayoutPad, false>), dim3(wgs), dim3(64 * kWaves), 0, st, a, lv);
    else return SDN_E_UNSUPPORTED;   // built for the derived layouts only (dnerf_amd/fused_basis.py binds one of them)
    return sdn_launch_status();
}

// density_scale * sigma of jittered occupancy-grid cell centres -> tmp_grid slice (density.hip's kernels do the rest of the update);
// q.f.bias0: the basis row of the slice's (perturbed) time
int field_cells_basis(const FieldCells &q, hipStream_t st) {
    TiledLevels lv;
    FieldArgs a;
    int rc = fill_field_args(a, lv, q.f);
    if (rc) return rc;
    a.cell_noise = q.noise; a.cell_seed = q.seed;
    const float half_grid = q.cas_bound / (float)q.grid_size;
    a.cell_inv = 1.0f / (float)(q.grid_size - 1); a.cell_span = q.cas_bound - half_grid; a.cell_half = half_grid;
    const uint32_t wgs = sdn_div_up(q.f.M, (uint32_t)kPointsPerWG);
    const int layout = field_table_layout(q.f.offsets_host);
    if (layout == kLayoutQuad) hipLaunchKernelGGL((k_field_basis_f16<kLayoutQuad, true>), dim3(wgs), dim3(64 * kWaves), 0, st, a, lv);
    else if (layout == kLayoutPad) hipLaunchKernelGGL((k_field_basis_f16<kLayoutPad, true>), dim3(wgs), dim3(64 * kWaves), 0, st, a, lv);
    else return SDN_E_UNSUPPORTED;   // as the forward
    return sdn_launch_status();
}

}  // namespace sdn_int

extern "C" {

uint32_t sdn_field_basis_weight_blocks(void) { return (uint32_t)sdn_basis::kBlkTotal; }

int sdn_field_basis_forward_f16(const float *xyzs, const float *dirs, const uint32_t *live_idx, const uint32_t *live_count, uint32_t M,
                                const void *weights, const float *basis_row, const void *table, const int32_t *offsets_host, float S, uint32_t H,
                                float bound, float density_scale, float *sigmas, float *rgbs, void *stream) {
    return sdn_int::field_forward_checked(3, {.xyzs = xyzs, .dirs = dirs, .live_idx = live_idx, .live_count = live_count, .M = M, .weights = weights,
                                              .bias0 = basis_row, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                              .density_scale = density_scale, .sigmas = sigmas, .rgbs = rgbs},
                                          stream);
}

// The density-grid query of update_extra_state for the temporal-basis model: sdn_density_query_cells_f16 with this model's packed
// weights and the basis row of the slice's (perturbed) time where that one takes bias0; nothing deforms, so there is no zero_deform.
int sdn_density_query_cells_basis_f16(const int32_t *cells, const uint32_t *cell_count, uint32_t n, const float *noise, uint32_t seed,
                                      uint32_t grid_size, float cas_bound, const void *weights, const float *basis_row, const void *table,
                                      const int32_t *offsets_host, float S, uint32_t H, float bound, float density_scale, float *tmp_slice,
                                      void *stream) {
    return sdn_int::field_cells_checked(3, {.f = {.live_idx = (const uint32_t *)cells, .live_count = cell_count, .M = n, .weights = weights,
                                                  .bias0 = basis_row, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                                  .density_scale = density_scale, .sigmas = tmp_slice},
                                            .noise = noise, .seed = seed, .grid_size = grid_size, .cas_bound = cas_bound},
                                        stream);
}

}  // extern "C"
