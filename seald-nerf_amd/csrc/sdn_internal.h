// Launch helpers shared between translation units of libsdn_hip (not part of the C ABI).
#pragma once
#include "sdn_common.h"

namespace sdn_int {

// Frame group selection handed (by value) to the loop kernels: with n_frames > 1 ray r belongs to frame r / rays_per_frame,
// marches grid[frame] with the cull grid cull + frame * cull_stride, and every emitted sample's frame goes to slot_frame.
struct FrameSel {
    uint32_t n_frames = 0;        // <= 1: a single frame, the kernels' own grid / cull arguments are used as they are
    uint32_t rays_per_frame = 0;
    uint32_t cull_stride = 0;     // uint32 words between the cull grids of consecutive frames
    uint32_t pad_ = 0;
    const uint8_t *grid[SDN_MAX_GROUP_FRAMES] = {};
    uint8_t *slot_frame = nullptr;
};
FrameSel frame_sel(const SdnRenderCtx &c);

// Pointers the loop derives from the context (one place each):
// the 4-deep ring of {alive rays entering the next iteration, iteration number} snapshots behind the trace
inline int32_t *snap_ring(const SdnRenderCtx &c) { return c.trace + 2 * (size_t)c.n_counters; }
// the survivor-count scratch word behind the ring: n_out of the culled start and of the 1024-ray count / scatter pair
inline int32_t *snap_n_out(const SdnRenderCtx &c) { return snap_ring(c) + 8; }
inline uint32_t *live_counters(const SdnRenderCtx &c) { return (uint32_t *)c.live_counts; }
// per-ray jump targets of the culled start: they live in `sigmas`, which is unused until the first field launch
inline float *jump_buffer(const SdnRenderCtx &c) { return c.rays_tend ? c.sigmas : nullptr; }
// the context's cull grid(s): built, and handed to the marchers, for the 128^3 single-cascade grid only
inline bool has_loop_cull(const SdnRenderCtx &c) { return c.H == 128 && c.C == 1; }
inline const uint32_t *loop_cull(const SdnRenderCtx &c) { return has_loop_cull(c) ? (const uint32_t *)c.cull_bits : nullptr; }

// The steps of the device-driven loop (render_loop.hip) on the buffers of one context; render.hip decides their order.
int loop_begin(const SdnRenderCtx &c, void *mailbox, uint32_t frame_tag, hipStream_t st);
int loop_cull_start(const SdnRenderCtx &c, hipStream_t st);
int loop_march(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st);
int loop_composite_compact(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st, bool freeze = false);
int loop_steady_begin(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st, bool frozen_already = false);
int loop_composite_march(const SdnRenderCtx &c, uint32_t bound_list, hipStream_t st);
int loop_finish(const SdnRenderCtx &c, float bg, float *image_out, float *depth_out, hipStream_t st);
int render_begin(const SdnRenderCtx *c, void *mailbox, uint32_t frame_tag, hipStream_t st);
int build_cull(const uint8_t *bitfield, uint32_t *cull_bits, hipStream_t st, bool with_image = true);
int march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C,
                     uint32_t H, uint32_t M, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                     const float *noises, void *scratch, const void *prebuilt_cull, hipStream_t st);
int build_cull_group(const FrameSel &fs, uint32_t *cull_bits, hipStream_t st);   // one cull grid per frame of the group
int copy_cull(const void *const *prebuilt, uint32_t n_frames, uint32_t *cull_bits, hipStream_t st);   // prebuilt grids -> the context's copy

// One launch of the fused field network (host side; the kernels keep their own argument records).  weights / table: the fp16
// fragments and table of sdn_field_forward_f16, or the packed floats and fp32 table of sdn_field_forward_f32 / _f32x3.
struct FieldCall {
    const float *xyzs = nullptr, *dirs = nullptr;
    const uint32_t *live_idx = nullptr, *live_count = nullptr;   // both or neither
    const int32_t *state = nullptr;      // the loop record (the live count is then live_count[SdnLoopRecord::iteration]), or nullptr
    uint32_t M = 0;
    const void *weights = nullptr;
    const float *bias0 = nullptr;        // n_frames rows
    const void *table = nullptr;
    const int32_t *offsets_host = nullptr;
    float S = 0;
    uint32_t H = 0;
    float bound = 0, density_scale = 0;
    int zero_deform = 0;                 // bit f: frame f is canonical
    float *sigmas = nullptr, *rgbs = nullptr;
    float *deform = nullptr;             // fp32 fields only: optional [M,3] output of the deformation network
    uint32_t expect_points = 0;          // fp16 field only: the caller's estimate of the live points when M is a loose bound (0 = unknown)
    const uint8_t *slot_frame = nullptr; // frame group: frame of every sample slot, or nullptr = one frame
    uint32_t n_frames = 1;
};
// The density-grid query: sigma * density_scale of the jittered centres of cells f.live_idx (nullptr: cells 0 .. f.M - 1) -> f.sigmas[cell]
struct FieldCells {
    FieldCall f;
    const float *noise = nullptr;
    uint32_t seed = 0, grid_size = 0;
    float cas_bound = 0;
};

// rows of bias0 a launch may select
inline uint32_t field_n_frames(const FieldCall &f) {
    if (!f.slot_frame || f.n_frames == 0) return 1u;
    return f.n_frames > (uint32_t)SDN_MAX_GROUP_FRAMES ? (uint32_t)SDN_MAX_GROUP_FRAMES : f.n_frames;
}

// one launcher per kernel; field_forward / field_cells pick by SdnRenderCtx::field_f32 (0: fp16, 1: fp32 MFMAs, 2: split fp16 operands,
// 3: the temporal-basis model's fp16 field, whose bias0 rows are its basis rows -- its density query takes the one row of the slice's
// time --, 4: the ambient-dimension model's fp16 field, whose bias0 rows hold the ambient coordinate in entry 0 -- its density query
// takes the one row of the slice's time too, 5: the temporal-basis model's fp32 field (field_basis_f32.hip): basis rows as kind 3 in
// fp32, the packed floats and the fp32 table in the reference layout as kind 1)
int field_forward_f16(const FieldCall &f, hipStream_t st);
int field_forward_f32(const FieldCall &f, hipStream_t st);
int field_forward_f32x3(const FieldCall &f, hipStream_t st);
int field_forward_basis(const FieldCall &f, hipStream_t st);
int field_forward_hyper(const FieldCall &f, hipStream_t st);
int field_forward_basis_f32(const FieldCall &f, hipStream_t st);
int field_cells_f16(const FieldCells &q, hipStream_t st);
int field_cells_f32(const FieldCells &q, hipStream_t st);
int field_cells_basis(const FieldCells &q, hipStream_t st);
int field_cells_hyper(const FieldCells &q, hipStream_t st);
int field_cells_basis_f32(const FieldCells &q, hipStream_t st);
inline int field_forward(int kind, const FieldCall &f, hipStream_t st) {
    if (kind == 3) return field_forward_basis(f, st);
    if (kind == 4) return field_forward_hyper(f, st);
    if (kind == 5) return field_forward_basis_f32(f, st);
    return kind == 2 ? field_forward_f32x3(f, st) : (kind ? field_forward_f32(f, st) : field_forward_f16(f, st));
}

// What the public entry points check before they launch (every failure is SDN_E_BADARG)
inline bool field_buffers_ok(const FieldCall &f) {
    if (!f.weights || !f.bias0 || !f.table || !f.offsets_host || !f.sigmas) return false;
    if ((f.live_idx == nullptr) != (f.live_count == nullptr)) return false;
    return ((uintptr_t)f.weights & 15u) == 0 && ((uintptr_t)f.table & 3u) == 0;
}
inline int field_forward_checked(int kind, const FieldCall &f, void *stream) {
    if (f.M == 0) return 0;
    if (!f.xyzs || !f.dirs || !f.rgbs || !field_buffers_ok(f)) return SDN_E_BADARG;
    return field_forward(kind, f, (hipStream_t)stream);
}
inline int field_cells_checked(int kind, const FieldCells &q, void *stream) {
    if (q.f.M == 0) return 0;
    if (!field_buffers_ok(q.f)) return SDN_E_BADARG;
    if (q.grid_size < 2 || q.grid_size > 1024 || !(q.cas_bound > 0)) return SDN_E_BADARG;
    // without a list, slot p IS the Morton index: n may not exceed the grid
    if (!q.f.live_idx && (uint64_t)q.f.M > (uint64_t)q.grid_size * q.grid_size * q.grid_size) return SDN_E_BADARG;
    if (kind == 3) return field_cells_basis(q, (hipStream_t)stream);
    if (kind == 4) return field_cells_hyper(q, (hipStream_t)stream);
    if (kind == 5) return field_cells_basis_f32(q, (hipStream_t)stream);
    return kind ? field_cells_f32(q, (hipStream_t)stream) : field_cells_f16(q, (hipStream_t)stream);
}

}  // namespace sdn_int

// Host-side pieces of the fused-MLP operator (ffmlp.hip) that the native training step (train.hip) composes itself: packing of
// several networks in one launch, the fused forward / backward chains on already packed fragments, and any set of weight-gradient
// products  out[M,N] = G[B,ldg]^T X[B,ldx]  (fp16 operands, fp32 split-K partial sums) in one launch + one reduction.
namespace sdn_ffh {
struct PackJob { const void *weights; void *packed; uint32_t in_dim, W, L; int backward, with_last; };
struct DwJob { const void *G; uint32_t ldg, M; const void *X; uint32_t ldx, N; void *out; };
uint32_t total_frags(uint32_t in_dim, uint32_t W, uint32_t L, int backward, int with_last);
int pack_many(const PackJob *jobs, uint32_t n, hipStream_t st);
int forward_packed(const void *inputs, const void *packed, uint32_t B, uint32_t in_dim, uint32_t W, uint32_t L, uint32_t act,
                   void *forward_buffer, void *outputs, hipStream_t st);
int backward_packed(const void *grad, const void *packed, const void *forward_buffer, uint32_t B, uint32_t in_dim, uint32_t W, uint32_t L,
                    uint32_t act, int want_dx, void *backward_buffer, void *grad_inputs, hipStream_t st);
uint64_t dw_jobs_bytes(const DwJob *jobs, uint32_t n, uint32_t B);
int dw_jobs(const DwJob *jobs, uint32_t n, uint32_t B, void *partial, hipStream_t st);
}  // namespace sdn_ffh
