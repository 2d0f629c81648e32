// Fused field evaluation of the ambient-dimension model on MFMA for gfx950 (MI355X), inference.
//
//   (xyz, ambient(t)) --4-D tiled grid (16 lv x 2)--> sigma MLP (64, 33) --> density logit --exp--> sigma
//                                                                       \--> 32 geo_feat
//   dir --SH(4)--> ++ geo_feat --> colour MLP (64, 64, 3) --sigmoid--> rgb
//
// Behavioural contract: NeRFNetwork.forward of the reference's dnerf/network_hyper.py:121-161 under `-O` (torch autocast): every Linear
// takes fp16 operands, accumulates in fp32 and rounds its output to fp16; the encoders run in fp32; the grid table and its output are
// fp16 with the two half roundings per corner of kernel_grid; sigma = exp(fp32(logit)); rgb = fp16(sigmoid(.)).  The ambient coordinate
// -- tanh of a 5-layer MLP of the time stamp alone, times bound -- is the same for every point of a frame: the host evaluates it once
// per time stamp (dnerf_amd/fused_hyper.py) and hands it over as entry 0 of the frame's constants row, where the deformation model's
// kernels take the time encoding's bias row (FieldArgs::bias0, row slot_frame[p] in a frame group).  The kernel normalises it as it
// normalises x, y, z and applies the range test to all four coordinates.  zero_deform is ignored: nothing deforms.
//
// Mapping: the one-tile-per-workgroup form of k_field_basis_f16 (field_basis.hip) -- 8 waves = 256 points, one wave = 32 points = the N
// dimension of v_mfma_f32_32x32x16_f16, weights the A operand, all 30 KiB of them copied to LDS once before the workgroup's one
// barrier.  The grid phase is the new part: 16 corners per level, 4 QUAD gathers where the level's index keeps the fourth coordinate
// and 2 where it drops it; the fourth coordinate's cell, row share and fraction per level are worked out once per workgroup and frame
// and read from LDS (field_hyper_net.h), per-lane work stays with x, y, z.  ("ambient-dimension field".)
#include "sdn_common.h"
#include "sdn_internal.h"
#include "cell_points.h"
#include "field_hyper_net.h"

namespace {

using namespace sdn_f16;

constexpr int kWaves = 8;                 // waves per workgroup, 32 points each
constexpr int kPointsPerWG = 32 * kWaves;
// Waves per SIMD the kernel is compiled for: one workgroup per CU.  Within 128 VGPRs (two workgroups per CU) the compiler spills about
// 120 registers per lane to scratch at every batch depth tried (1, 2, 4): the 16-corner interpolation with its pinned candidates does
// not fit beside the gathered blocks.  At 2 waves per SIMD it takes 222 VGPRs and no scratch, and the deeper batch makes up for the
// missing second workgroup with gathers in flight: up to 16 QUAD blocks per lane.
constexpr int kOcc = 2;
// The density-grid query (CELLS) drops the colour net, but the grid phase is what sets the budget: compiled for 4 it spills 360 bytes
// per lane at batch depth 4, 452 at 2 and 500 at 1 (profiles/hyper_cells_isa.txt), so it stays at one workgroup per CU as well.
constexpr int kOccCells = 2;
constexpr int kGridBatch = 4;             // grid levels (per lane-half) whose gathers are in flight together

// CELLS: the density-grid query of update_extra_state (dnerf/renderer.py:453-555), as k_field_basis_f16's (field_basis.hip): slot p is a
//   Morton cell index, the point is that cell's jittered centre (cell_points.h), no xyzs / dirs / rgbs / slot_frame buffer is touched,
//   only the density is evaluated and stored at sigmas[p] (a slice of tmp_grid).  One slice per launch: the ambient coordinate is entry
//   0 of row 0 of bias0, and only frame 0's fourth-coordinate records are worked out (the launcher sets n_frames = 1).  The range test
//   is the forward's, on all four coordinates.  The colour net and the sigma net's geo_feat tile (tile 0 of S1: permute_s1) are
//   compiled out.  Weights in LDS: exactly the 8 fragments the launch reads -- S0 (blocks 0..3) and the logit tile of S1 (blocks 8..11)
//   -- packed back to back (sdn_hyper::kBlkS1Logit), not the contiguous prefix of 12.
template <int LAYOUT, bool CELLS>
__global__ void __launch_bounds__(64 * kWaves, CELLS ? kOccCells : kOcc) k_field_hyper_f16(FieldArgs P, sdn_hyper::HyperLevels hl) {
    constexpr int kBlkResident = CELLS ? sdn_hyper::kBlkCellsTotal : sdn_hyper::kBlkTotal;
    __shared__ __attribute__((aligned(16))) unsigned char s_w[kBlkResident * 1024];
    __shared__ __attribute__((aligned(512))) uint4 s_lv[16][2];   // per grid level: {offset, s1, s2, hsize}, {mask, scale, s3, -}
    __shared__ __attribute__((aligned(16))) uint2 s_amb[CELLS ? 1 : SDN_MAX_GROUP_FRAMES][16];   // per frame and level: the fourth coordinate's {row share, fraction}
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    sdn_hyper::levels_to_lds(s_lv, hl);
    sdn_hyper::ambient_to_lds(s_amb, hl, P);
    const uint32_t count = live_points(P);
    if (blockIdx.x * (uint32_t)kPointsPerWG >= count) return;  // workgroup-uniform: nothing to do, no barrier touched
    // the weights, 16 bytes per lane and step, in fragment order as they lie in memory (every workgroup reads the same 30 KiB: L2)
    if constexpr (CELLS) {
        for (uint32_t c = threadIdx.x; c < (uint32_t)kBlkResident * 64u; c += 64u * kWaves) {
            const uint32_t src = c < (uint32_t)sdn_hyper::kBlkS1 * 64u ? c : c + (uint32_t)(sdn_hyper::kBlkS1 + 4 - sdn_hyper::kBlkS1Logit) * 64u;
            reinterpret_cast<uint4 *>(s_w)[c] = reinterpret_cast<const uint4 *>(P.weights)[src];
        }
    } else {
        for (uint32_t c = threadIdx.x; c < (uint32_t)sdn_hyper::kBlkTotal * 64u; c += 64u * kWaves)
            reinterpret_cast<uint4 *>(s_w)[c] = reinterpret_cast<const uint4 *>(P.weights)[c];
    }
    const uint32_t n = lane & 31u, h = lane >> 5;
    const uint32_t i = blockIdx.x * (uint32_t)kPointsPerWG + wave * 32u + n;
    const bool valid = i < count;
    const uint32_t ii = valid ? i : (count - 1);  // idle lanes recompute the last point and store nothing
    const uint32_t p = P.live_idx ? P.live_idx[ii] : ii;
    float x0, x1, x2, d0 = 0, d1 = 0, d2 = 0;
    uint32_t frame = 0u;
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
        frame = P.slot_frame ? (uint32_t)P.slot_frame[p] : 0u;   // the constants row of the point's frame
        if (frame >= P.n_frames) frame = P.n_frames - 1u;
    }
    const float u3 = sdn_hyper::unit_coord(P.bias0[128u * frame], P);
    float u[3];
    grid_coords(zero_tile(), lane, x0, x1, x2, true, P, u);   // canonical: the model has no deformation
    const bool oob = out_of_grid(u) | (u3 < 0) | (u3 > 1);
    __syncthreads();  // the levels, the fourth coordinate's records and the weights are in LDS
    uint32_t gfw[2][4];   // 8 levels x 2 features as packed pairs
    sdn_hyper::grid_encode<LAYOUT, kGridBatch>(s_lv, s_amb[frame], reinterpret_cast<const unsigned char *>(P.table), u, oob, h, gfw);
    half8 gf[2];
    grid_operand(gfw, gf);
    f32x16 hv[2];
    sdn_hyper::sigma_net<!CELLS>(s_w, gf, lane, hv);
    const float sigma = density(hv[1], P.density_scale);   // row 0 of tile 1: register 0 of lane-half 0
    if constexpr (CELLS) {
        if (h == 0 && valid) P.sigmas[p] = sigma;   // duplicates in the list: any one of them wins, as with tmp_grid[indices] = sigmas
        return;
    }
    const f32x16 co = sdn_hyper::colour_net(s_w, sh_operand(d0, d1, d2, h), hv[0], lane);
    if (h == 0 && valid) store_sigma_rgb(P, p, sigma, co);
}

}  // namespace

namespace sdn_int {

// launch used by both the C entry point and the device-driven render loop (render.hip)
int field_forward_hyper(const FieldCall &f, hipStream_t st) {
    sdn_hyper::HyperLevels hl;
    FieldArgs a;
    int rc = fill_tiled_levels_nd(hl.lv, &hl.s3, 4, f.offsets_host, f.S, f.H);
    if (rc) return rc;
    fill_field_record(a, f);
    const uint32_t wgs = sdn_div_up(f.M, (uint32_t)kPointsPerWG);
    const int layout = field_table_layout(f.offsets_host);
    if (layout == kLayoutQuad) hipLaunchKernelGGL((k_field_hyper_f16<kLayoutQuad, false>), dim3(wgs), dim3(64 * kWaves), 0, st, a, hl);
    else if (layout == kLayoutPad) hipLaunchKernelGGL((k_field_hyper_f16<kLayoutPad, false>), dim3(wgs), dim3(64 * kWaves), 0, st, a, hl);
    else return SDN_E_UNSUPPORTED;   // built for the derived layouts only (dnerf_amd/fused_hyper.py binds one of them)
    return sdn_launch_status();
}

// density_scale * sigma of jittered occupancy-grid cell centres -> tmp_grid slice (density.hip's kernels do the rest of the update);
// q.f.bias0: the ambient row of the slice's (perturbed) time.  One row: whatever the caller set, the kernel sees a single frame.
int field_cells_hyper(const FieldCells &q, hipStream_t st) {
    sdn_hyper::HyperLevels hl;
    FieldArgs a;
    int rc = fill_tiled_levels_nd(hl.lv, &hl.s3, 4, q.f.offsets_host, q.f.S, q.f.H);
    if (rc) return rc;
    fill_field_record(a, q.f);
    a.slot_frame = nullptr; a.n_frames = 1;
    a.cell_noise = q.noise; a.cell_seed = q.seed;
    const float half_grid = q.cas_bound / (float)q.grid_size;
    a.cell_inv = 1.0f / (float)(q.grid_size - 1); a.cell_span = q.cas_bound - half_grid; a.cell_half = half_grid;
    const uint32_t wgs = sdn_div_up(q.f.M, (uint32_t)kPointsPerWG);
    const int layout = field_table_layout(q.f.offsets_host);
    if (layout == kLayoutQuad) hipLaunchKernelGGL((k_field_hyper_f16<kLayoutQuad, true>), dim3(wgs), dim3(64 * kWaves), 0, st, a, hl);
    else if (layout == kLayoutPad) hipLaunchKernelGGL((k_field_hyper_f16<kLayoutPad, true>), dim3(wgs), dim3(64 * kWaves), 0, st, a, hl);
    else return SDN_E_UNSUPPORTED;   // as the forward
    return sdn_launch_status();
}

}  // namespace sdn_int

extern "C" {

uint32_t sdn_field_hyper_weight_blocks(void) { return (uint32_t)sdn_hyper::kBlkTotal; }

int sdn_field_hyper_forward_f16(const float *xyzs, const float *dirs, const uint32_t *live_idx, const uint32_t *live_count, uint32_t M,
                                const void *weights, const float *ambient_row, const void *table, const int32_t *offsets_host, float S, uint32_t H,
                                float bound, float density_scale, float *sigmas, float *rgbs, void *stream) {
    return sdn_int::field_forward_checked(4, {.xyzs = xyzs, .dirs = dirs, .live_idx = live_idx, .live_count = live_count, .M = M, .weights = weights,
                                              .bias0 = ambient_row, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                              .density_scale = density_scale, .sigmas = sigmas, .rgbs = rgbs},
                                          stream);
}

// The density-grid query of update_extra_state for the ambient-dimension model: sdn_density_query_cells_f16 with this model's packed
// weights and the ambient row of the slice's (perturbed) time where that one takes bias0; nothing deforms, so there is no zero_deform.
int sdn_density_query_cells_hyper_f16(const int32_t *cells, const uint32_t *cell_count, uint32_t n, const float *noise, uint32_t seed,
                                      uint32_t grid_size, float cas_bound, const void *weights, const float *ambient_row, const void *table,
                                      const int32_t *offsets_host, float S, uint32_t H, float bound, float density_scale, float *tmp_slice,
                                      void *stream) {
    return sdn_int::field_cells_checked(4, {.f = {.live_idx = (const uint32_t *)cells, .live_count = cell_count, .M = n, .weights = weights,
                                                  .bias0 = ambient_row, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                                  .density_scale = density_scale, .sigmas = tmp_slice},
                                            .noise = noise, .seed = seed, .grid_size = grid_size, .cas_bound = cas_bound},
                                        stream);
}

}  // extern "C"
