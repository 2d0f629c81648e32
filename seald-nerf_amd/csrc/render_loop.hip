// The inference marcher, its compositor, the alive-list compaction and the device-driven render loop for gfx950 (MI355X).
//
// Holds march_ray and the frame rounds of a marching workgroup, k_march_rays / k_composite_rays / k_compact_* with their public entry
// points (sdn_march_rays, sdn_march_rays_ex, sdn_composite_rays, sdn_compact_alive), and every kernel and host step of the
// device-driven loop (sdn_int::loop_*: init, culled start, compaction + advance, the steady mode's composite+march, finish).
// Behavioural contract: raymarching/src/raymarching.cu:701-905 of the reference (march_rays, composite_rays) and the inference
// loop of dnerf/renderer.py:333-381; line ranges are cited per kernel.  The stepper, the exact cull test, the LDS occupancy caches
// and the lattice closed form come from march_core.h, scans / reductions / the ranked scatter from block_ops.h; the arithmetic
// contract (-ffp-contract=off, bit-exact against oracle/sdn_oracle.c) is described there.
//
// Layout notes (MI355X): one lane per ray, 256-thread workgroups (4 waves, one per SIMD).  The density bitfield of one time slice is
// 256 KiB and lives in the XCD's L2 after first touch; the marcher is bound by dependent L2 byte gathers and by wave divergence, not
// by HBM.  Rays keep image order in rays_alive (stable compaction), so a wave's 64 rays are neighbouring pixels and take similar
// trip counts.
#include "march_core.h"
#include "block_ops.h"

namespace {

// ---------------------------------------------------------------------------
// inference
// ---------------------------------------------------------------------------
// Marches one ray from parameter t for up to n_step samples into its slots (the loop of raymarching.cu:750-804), zero-fills
// the unused slots and returns the number of samples written.
// tend (may be null): this ray's cached cull result.  The bound t_end found by ray_may_hit -- beyond it the ray meets no
// marked cell -- is a property of the ray, not of where the scan started, so the device loop computes it on a ray's first
// march and later iterations only compare (kTendUnset: not computed yet; kTendDead: the ray cannot produce a sample).
// device loop: the cache's base pointer travels in the loop record (sdn_loop_tend; nullptr = no cache)
template <bool FAST>
__device__ __forceinline__ uint32_t march_ray(MarcherT<FAST> &m, const OccCache &oc, float t, float far, uint32_t n_step, float *px, float *pd,
                                              float *pl, float *tend = nullptr, uint8_t *psf = nullptr, uint32_t frame = 0,
                                              const float *t_begin = nullptr) {
    m.fine = oc.fine; m.fx0 = oc.fx0; m.fy0 = oc.fy0; m.fz0 = oc.fz0; m.fnx = oc.fnx; m.fny = oc.fny; m.fnz = oc.fnz;
    uint32_t step = 0;
    // t_begin: the walk resumes at t, a later point of the chain that started at *t_begin (k_cull_start's certified jump): the first
    // sample's second delta is measured from the chain's start, as the walk from there would have measured it
    float last_t = t_begin ? *t_begin : t, x, y, z, dt;
    bool go = t < far;
    float t_end = far;
    if (FAST && oc.s_cull && go) {
        const float cached = tend ? *tend : kTendUnset;
        if (cached != kTendUnset) {
            t_end = cached;                 // kTendDead (< every t) ends the ray here
            go = t < t_end;
        } else {
            go = ray_may_hit(oc.s_cull, m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t, far, t_end, oc.fx0, oc.fy0, oc.fz0, oc.fnx, oc.fny, oc.fnz);
            if (tend) *tend = go ? t_end : kTendDead;
        }
    }
    if (go) {
        while (t < far && t < t_end && step < n_step) {
            if (m.probe(t, x, y, z, dt, oc.s_cull)) {
                px[0] = x; px[1] = y; px[2] = z;
                pd[0] = m.dx; pd[1] = m.dy; pd[2] = m.dz;
                t += dt;
                pl[0] = dt;
                pl[1] = t - last_t;
                last_t = t;
                px += 3; pd += 3; pl += 2;
                if (psf) psf[step] = (uint8_t)frame;   // frame group: which frame's time constants the field network applies
                step++;
            }
        }
    }
    for (uint32_t k = step; k < n_step; k++) {
        px[0] = 0; px[1] = 0; px[2] = 0;
        pd[0] = 0; pd[1] = 0; pd[2] = 0;
        pl[0] = 0; pl[1] = 0;
        px += 3; pd += 3; pl += 2;
    }
    return step;
}

// ---- frame groups (FrameSel::n_frames > 1) -------------------------------------------------------------------------------------
// The alive list is ordered by ray id (stable compaction; the steady mode's frozen list keeps that order) and rays are
// frame-major, so a 256-entry workgroup sees one frame, or two at a frame boundary.  A marching workgroup therefore loops over the
// frames present among its live entries (ascending; one round in all but the <= n_frames - 1 boundary workgroups of a launch):
// per round it loads the LDS occupancy caches of that frame and the lanes of that frame march.  Same code, same LDS address
// space, no per-lane indexing of the kernel-argument record (fs.grid[] is only ever indexed with a workgroup-uniform value).
constexpr uint32_t kNoFrame = 0xFFFFFFFFu;
__device__ __forceinline__ const uint8_t *frame_grid_uniform(const FrameSel &fs, uint32_t frame_uniform) {
    return fs.grid[__builtin_amdgcn_readfirstlane(frame_uniform)];
}

// A marching lane's ray: origin, direction and far bound.  The marching kernels fetch them BEFORE their workgroup's barriers and LDS
// fill, so that the loads land under those instead of behind them.
struct RayIn { float o[3] = {0, 0, 0}, d[3] = {0, 0, 1}, far = 0; };
__device__ __forceinline__ void ray_in_fetch(RayIn &r, int index, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                             const float *__restrict__ fars) {
    r.o[0] = rays_o[(size_t)index * 3]; r.o[1] = rays_o[(size_t)index * 3 + 1]; r.o[2] = rays_o[(size_t)index * 3 + 2];
    r.d[0] = rays_d[(size_t)index * 3]; r.d[1] = rays_d[(size_t)index * 3 + 1]; r.d[2] = rays_d[(size_t)index * 3 + 2];
    r.far = fars[index];
}

// The frame rounds of a marching workgroup (see above): one round per frame present among its marching lanes -- exactly one without a
// frame group -- in which the workgroup loads that frame's LDS occupancy caches and the lanes of that frame call
// march(oc, grid_f, frame, grouped).  Contains barriers: every thread of the workgroup must call it (marches: this lane has a ray to
// march, index: its ray).  s_cull4 / s_fine / s_min4: the kernel's LDS for the caches and the frame minimum.
template <bool FAST, typename March>
__device__ __forceinline__ void frame_rounds(const FrameSel &fs, bool marches, int index, const uint8_t *__restrict__ grid,
                                             const uint32_t *__restrict__ cull, uint4 *s_cull4, unsigned long long *s_fine, uint32_t *s_min4,
                                             March march) {
    const bool grouped = fs.n_frames > 1;  // kernel-uniform
    const uint32_t frame = (grouped && marches) ? (uint32_t)index / fs.rays_per_frame : (grouped ? kNoFrame : 0u);
    uint32_t fcur = grouped ? block_min_256(frame, s_min4) : 0u;
    while (fcur != kNoFrame) {
        const uint8_t *grid_f = grouped ? frame_grid_uniform(fs, fcur) : grid;   // (fcur is workgroup-uniform)
        const uint32_t *cull_f = (grouped && cull) ? cull + (size_t)fcur * fs.cull_stride : cull;
        OccCache oc;
        occ_cache_load<FAST>(cull_f, grid_f, s_cull4, s_fine, oc);
        if (marches && frame == fcur) march(oc, grid_f, frame, grouped);
        if (!grouped) break;
        fcur = block_min_256((frame != kNoFrame && frame > fcur) ? frame : kNoFrame, s_min4);   // (the barriers inside also fence the LDS caches)
    }
}

// Appends the slots n*n_step .. +step of every lane to the live list: one atomicAdd per wave, prefix by wave shuffles.
// Must be called by all 64 lanes of the wave.
__device__ __forceinline__ void live_append(uint32_t step, uint32_t n, uint32_t n_step, uint32_t *__restrict__ live_idx,
                                            uint32_t *__restrict__ live_count) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t incl = step;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += u;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    uint32_t base = 0;
    if (lane == 63 && total) base = atomicAdd(live_count, total);
    base = __shfl(base, 63, 64);
    const uint32_t dst = base + incl - step;
    for (uint32_t k = 0; k < step; k++) live_idx[dst + k] = n * n_step + k;
}

// Resumes the compositing of one ray over its n_step slots (raymarching.cu:845-904).  Returns true if the ray survives.
// The per-ray state and -- in the n_step == 8 case the loop spends most of its iterations in -- all 8 slots of the ray
// (8 sigmas, 24 colours, 16 deltas: twelve 16-byte loads) are fetched before the serial recurrence starts, so the ray pays one
// memory round trip instead of one per sample (a lane is a ray here and there is at most one wave per SIMD to hide latency
// behind); the arithmetic and its order, including the two early exits, are the reference's.
__device__ __forceinline__ bool composite_ray(int index, uint32_t n_step, float T_thresh, const float *s, const float *c, const float *dl,
                                              float *__restrict__ rays_t, float *__restrict__ weights_sum, float *__restrict__ depth,
                                              float *__restrict__ image, float *t_out = nullptr) {
    CompositeAcc a = {rays_t[index], weights_sum[index], depth[index], image[(size_t)index * 3], image[(size_t)index * 3 + 1],
                      image[(size_t)index * 3 + 2]};
    uint32_t step = 0;
    if (n_step == 8) {
        float sv[8], cv[24], dv[16];
        #pragma unroll
        for (int q = 0; q < 2; q++) *reinterpret_cast<float4 *>(sv + 4 * q) = *reinterpret_cast<const float4 *>(s + 4 * q);
        #pragma unroll
        for (int q = 0; q < 6; q++) *reinterpret_cast<float4 *>(cv + 4 * q) = *reinterpret_cast<const float4 *>(c + 4 * q);
        #pragma unroll
        for (int q = 0; q < 4; q++) *reinterpret_cast<float4 *>(dv + 4 * q) = *reinterpret_cast<const float4 *>(dl + 4 * q);
        bool open = true;   // false once the reference's loop would have left through a break
        #pragma unroll
        for (int k = 0; k < 8; k++) {
            if (open && dv[2 * k] == 0) open = false;
            if (open) {
                if (composite_step(a, sv[k], dv[2 * k], dv[2 * k + 1], cv[3 * k], cv[3 * k + 1], cv[3 * k + 2]) < T_thresh) open = false;
                else step++;
            }
        }
    } else {
        while (step < n_step) {
            if (dl[0] == 0) break;
            if (composite_step(a, s[0], dl[0], dl[1], c[0], c[1], c[2]) < T_thresh) break;
            s++; c += 3; dl += 2; step++;
        }
    }
    const bool survives = !(step < n_step);
    if (survives) rays_t[index] = a.t;
    if (t_out) *t_out = a.t;
    weights_sum[index] = a.weight_sum; depth[index] = a.d;
    image[(size_t)index * 3] = a.r; image[(size_t)index * 3 + 1] = a.g; image[(size_t)index * 3 + 2] = a.b;
    return survives;
}

// raymarching.cu:701-805.  Extras over the reference kernel (all optional, none changes a sample):
//   * slots [step, n_step) of each alive ray are written as zeros here and the alignment tail [n_alive*n_step, M_pad)
//     is cleared by the same launch, so the caller never memsets the sample buffers;
//   * cull: exact early-out for rays that cannot produce a sample (see ray_may_hit), LDS occupancy caches;
//   * live_idx / live_count: the slots that received a sample are appended (one atomicAdd per wave, ballot-free prefix
//     via wave shuffles) to a compact list so that the field network is evaluated on samples, not on padded slots.
template <bool FAST>
__global__ void __launch_bounds__(256) k_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive,
                                                    const float *__restrict__ rays_t, const float *__restrict__ rays_o,
                                                    const float *__restrict__ rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                                    uint32_t C, uint32_t H, const uint8_t *__restrict__ grid,
                                                    const float *__restrict__ fars, float *__restrict__ xyzs, float *__restrict__ dirs,
                                                    float *__restrict__ deltas, const float *__restrict__ noises, uint32_t M_pad,
                                                    const uint32_t *__restrict__ cull, uint32_t *__restrict__ live_idx,
                                                    uint32_t *__restrict__ live_count, const int32_t *__restrict__ state,
                                                    const int32_t *__restrict__ rays_alive_b, FrameSel fs, const float *__restrict__ jump) {
    const SdnLoopRecord *rec = sdn_loop(state);
    if (rec) {  // device-driven loop: sizes, ping-pong side and the iteration's live counter come from the loop record
        n_alive = (uint32_t)rec->n_alive;
        n_step = (uint32_t)rec->n_step;
        if (n_alive == 0) return;
        if (rec->side) rays_alive = rays_alive_b;
        live_count += rec->iteration;
        const uint32_t m0 = n_alive * n_step;
        M_pad = m0 + (128u - m0 % 128u);
        if (!(rec->culled_start && rec->iteration == 0)) jump = nullptr;   // the per-ray jump targets of k_cull_start hold for the first march only
        if (rec->iteration != 0) noises = nullptr;   // the loop's noises (SdnRenderCtx::noises) perturb the march of iteration 0 only
        if (blockIdx.x * 256u >= n_alive + 128u) return;   // workgroup-uniform: beyond the list and its alignment tail (the host sizes the grid by a bound)
    }
    __shared__ uint4 s_cull4[FAST ? 256 : 1];  // 32^3 bits = 4 KiB
    __shared__ unsigned long long s_fine[FAST ? kFineCacheCells : 1];  // <= 32 KiB
    __shared__ uint32_t s_min4[4];
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    const int index = n < n_alive ? rays_alive[n] : -1;
    uint32_t step = 0;
    // the ray's inputs are fetched NOW: they land under the workgroup's barriers and its LDS fill instead of behind them
    RayIn ray;
    float t_ray = 0, t_jump = 0, noise = 0;
    if (index >= 0) {
        ray_in_fetch(ray, index, rays_o, rays_d, fars);
        t_ray = rays_t[index];
        if (jump) t_jump = jump[index];
        // drop-in ABI: one offset per list position (the reference's noises[n]); the loop's are per RAY -- iteration 0 of a culled start
        // runs on the compacted list, where position and ray differ (on the reference's arange(N) list they coincide)
        if (noises) noise = noises[rec ? (uint32_t)index : n];
    }
    frame_rounds<FAST>(fs, index >= 0, index, grid, cull, s_cull4, s_fine, s_min4,
                       [&](const OccCache &oc, const uint8_t *grid_f, uint32_t frame, bool grouped) __attribute__((always_inline)) {
        MarcherT<FAST> m;
        m.init(ray.o, ray.d, bound, dt_gamma, max_steps, C, H, grid_f);
        float t = t_ray;
        t += m.step_size(t) * noise;
        float *tend = rec ? sdn_loop_tend(*rec) : nullptr;
        if (tend) tend += index;
        const float t_walk = jump ? t_jump : t;   // (== t where k_cull_start certified no jump)
        step = march_ray<FAST>(m, oc, t_walk, ray.far, n_step, xyzs + (size_t)n * n_step * 3, dirs + (size_t)n * n_step * 3,
                               deltas + (size_t)n * n_step * 2, tend, grouped ? fs.slot_frame + (size_t)n * n_step : nullptr, frame,
                               jump ? &t : nullptr);
    });
    if (n >= n_alive) {
        const uint32_t slot = n_alive * n_step + (n - n_alive);  // spare lanes of the last blocks clear the alignment tail
        if (slot < M_pad) {
            xyzs[(size_t)slot * 3] = 0; xyzs[(size_t)slot * 3 + 1] = 0; xyzs[(size_t)slot * 3 + 2] = 0;
            dirs[(size_t)slot * 3] = 0; dirs[(size_t)slot * 3 + 1] = 0; dirs[(size_t)slot * 3 + 2] = 0;
            deltas[(size_t)slot * 2] = 0; deltas[(size_t)slot * 2 + 1] = 0;
        }
    }
    if (live_idx) live_append(step, n, n_step, live_idx, live_count);  // kernel-uniform condition
}

// raymarching.cu:819-905
__global__ void __launch_bounds__(256) k_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *__restrict__ rays_alive,
                                                        float *__restrict__ rays_t, const float *__restrict__ sigmas,
                                                        const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                                        float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
                                                        const int32_t *__restrict__ state, int32_t *__restrict__ rays_alive_b,
                                                        uint32_t *__restrict__ block_totals) {
    if (state) {
        const SdnLoopRecord &rec = *sdn_loop(state);
        n_alive = sdn_loop_list_len(rec);
        n_step = (uint32_t)rec.n_step;
        if (rec.side) rays_alive = rays_alive_b;
    }
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    bool survives = false;
    if (n < n_alive) {
        const int index = rays_alive[n];
        if (index >= 0) {    // (a frozen list holds dead entries)
            survives = composite_ray(index, n_step, T_thresh, sigmas + (size_t)n * n_step, rgbs + (size_t)n * n_step * 3,
                                     deltas + (size_t)n * n_step * 2, rays_t, weights_sum, depth, image);
            if (!survives) rays_alive[n] = -1;
        }
    }
    if (block_totals) {  // kernel-uniform: survivor count of this 256-ray block, for the fused compaction of the device loop
        __shared__ uint32_t s_cnt[4];
        const uint32_t c = block_count_256(survives, s_cnt);
        if (threadIdx.x == 0) block_totals[blockIdx.x] = c;
    }
}

// ---------------------------------------------------------------------------
// stable compaction of rays_alive >= 0 (replaces the torch mask-select of dnerf/renderer.py:372)
// two launches: per-block survivor counts (wave ballot + popcount), then scatter.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kScanBlock) k_compact_count(const int32_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ block_totals,
                                                              const int32_t *__restrict__ state, const int32_t *__restrict__ in_b) {
    if (state) {
        const SdnLoopRecord &rec = *sdn_loop(state);
        n = sdn_loop_list_len(rec);
        if (rec.side) in = in_b;
        if (blockIdx.x * kScanBlock >= n) return;  // workgroup-uniform
    }
    __shared__ uint32_t lds[16];
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    const bool keep = i < n && in[i] >= 0;
    const unsigned long long mask = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < (kScanBlock >> 6); w++) t += lds[w];
        block_totals[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kScanBlock) k_compact_scatter(const int32_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ block_totals,
                                                                int32_t *__restrict__ out, int32_t *__restrict__ n_out,
                                                                const int32_t *__restrict__ state, const int32_t *__restrict__ in_b,
                                                                int32_t *__restrict__ out_b, uint32_t totals_per_block) {
    // totals_per_block: block_totals holds one count per (kScanBlock / totals_per_block) entries -- 1: k_compact_count's, 4: the
    // per-256-ray survivor counts k_composite_rays wrote (the device loop skips the count launch)
    uint32_t last_block = gridDim.x - 1;
    if (state) {
        const SdnLoopRecord &rec = *sdn_loop(state);
        n = sdn_loop_list_len(rec);
        if (rec.side) { in = in_b; out = out_b; }
        if (n == 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) n_out[0] = 0;
            return;
        }
        last_block = (n - 1) / kScanBlock;
        if (blockIdx.x > last_block) return;  // workgroup-uniform
    }
    __shared__ uint32_t lds[16];
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x * totals_per_block; b += kScanBlock) part += block_totals[b];
    uint32_t prev;   // survivors of the blocks before this one (the scan hands the block's total to every thread)
    block_inclusive_scan(part, lds, prev);
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t total = ranked_scatter<kScanBlock / 64>(i < n ? in[i] : -1, prev, out, lds);
    if (blockIdx.x == last_block && threadIdx.x == 0) n_out[0] = (int32_t)(prev + total);
}


// ---------------------------------------------------------------------------
// device-driven inference loop (dnerf/renderer.py:340-381 without a host round trip per iteration)
// The loop record `state` is an SdnLoopRecord (include/sdn_hip.h documents every word); kernels view it through sdn_loop().
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_loop_init(uint32_t N, uint32_t max_steps, const float *__restrict__ nears, int32_t *__restrict__ alive_a,
                                                   float *__restrict__ rays_t, float *__restrict__ weights_sum, float *__restrict__ depth,
                                                   float *__restrict__ image, int32_t *__restrict__ state, int32_t *__restrict__ live_counts,
                                                   uint32_t n_counters, unsigned long long mailbox, uint32_t frame_tag,
                                                   float *__restrict__ rays_tend) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n < N) {
        if (rays_tend) rays_tend[n] = kTendUnset;
        alive_a[n] = (int32_t)n;
        rays_t[n] = nears[n];
        weights_sum[n] = 0; depth[n] = 0;
        image[(size_t)n * 3] = 0; image[(size_t)n * 3 + 1] = 0; image[(size_t)n * 3 + 2] = 0;
    }
    if (n < n_counters) live_counts[n] = 0;
    if (n == 0) {
        SdnLoopRecord &rec = *sdn_loop(state);
        rec.n_alive = (int32_t)N; rec.n_step = 1; rec.steps_done = 0; rec.iteration = 0; rec.side = 0;
        rec.N = (int32_t)N; rec.max_steps = (int32_t)max_steps; rec.advance_calls = 0;
        rec.frozen_len = 0; rec.survivors = 0;
        rec.mailbox_lo = (int32_t)(uint32_t)mailbox;
        rec.mailbox_hi = (int32_t)(uint32_t)(mailbox >> 32);
        rec.frame_tag = (int32_t)frame_tag;
        const unsigned long long tp = (unsigned long long)(uintptr_t)rays_tend;
        rec.tend_lo = (int32_t)(uint32_t)tp;
        rec.tend_hi = (int32_t)(uint32_t)(tp >> 32);
        rec.culled_start = 0;
    }
}


// Per-iteration snapshot {alive rays entering the next iteration, index of that iteration}: into the device ring `snap`
// (4 deep, immutable once written: the host may copy it out while the next iteration runs) and, when the frame driver
// registered a mailbox in coherent host memory, as ONE 64-bit system-scope store {tag : n_alive} the host polls for --
// no event, no copy, no stream wait on the critical path.  tag = frame_tag << 16 | (call + 1).
__device__ __forceinline__ void publish_snapshot(const SdnLoopRecord &rec, int32_t *__restrict__ snap, int32_t call) {
    snap[(call & 3) * 2] = rec.n_alive;
    snap[(call & 3) * 2 + 1] = call + 1;
    unsigned long long *mb = sdn_loop_mailbox(rec);
    if (mb) {
        const unsigned long long tag = ((uint32_t)rec.frame_tag << 16) | (uint32_t)(call + 1);
        __hip_atomic_store(mb + (call & 3), (tag << 32) | (uint32_t)rec.n_alive, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Advances the loop record past the iteration that just ran; one thread, after every reader of the record in the launch is done.
// Logs the iteration's {n_alive, n_step} in the trace (only iterations that did work), adds its steps, applies `while step < max_steps`
// and sets the survivors n_new as the next iteration's n_alive; freeze: the steady mode starts with the list as it now stands as
// its frozen list; then publishes the snapshot.
// RECOMPACTED: the survivors were compacted to the other side -- the side flips and n_step = max(min(N // n_alive, 8), 1) is set
// (false: the steady mode, whose frozen list stays where it is and whose n_step stays 8: N / n_new >= 8 holds from its start on).
// CULLED_LOGS_N: after a culled start the trace logs N for iteration 0, the reference's N-ray iteration (SdnLoopRecord::culled_start).
template <bool RECOMPACTED, bool CULLED_LOGS_N>
__device__ __forceinline__ void advance_record(SdnLoopRecord &rec, int32_t *__restrict__ trace, int32_t *__restrict__ snap, int32_t n_new,
                                               int freeze) {
    const int32_t it = rec.iteration;
    const int32_t call = rec.advance_calls;   // no-op iterations included
    rec.advance_calls = call + 1;
    if (rec.n_alive > 0) {
        trace[2 * it] = (CULLED_LOGS_N && it == 0 && rec.culled_start) ? rec.N : rec.n_alive;
        trace[2 * it + 1] = rec.n_step;
        rec.steps_done += rec.n_step;
        rec.iteration = it + 1;
        if (RECOMPACTED) rec.side ^= 1;
        if (rec.steps_done >= rec.max_steps) n_new = 0;
        rec.n_alive = n_new;
        if (RECOMPACTED && n_new > 0) {
            const int32_t ns = rec.N / n_new;
            rec.n_step = ns > 8 ? 8 : (ns < 1 ? 1 : ns);
        }
    }
    if (freeze) { rec.frozen_len = rec.n_alive; rec.survivors = 0; }   // (k_steady_begin folded in)
    publish_snapshot(rec, snap, call);
}

// Last-workgroup election of a launch: every workgroup takes a ticket after its last access to what the last one will touch (the
// caller puts a barrier between those accesses and this call); true in every thread of the workgroup that drew the last ticket,
// which then sees the other workgroups' writes.  The ticket is reset for the next launch HERE, before the caller's last-workgroup work
// (every other workgroup of the launch has drawn its ticket by then).  Must be called by the whole workgroup.
__device__ __forceinline__ bool last_workgroup(int32_t *__restrict__ ticket) {
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = (atomicAdd(ticket, 1) == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    if (threadIdx.x == 0) *ticket = 0;
    return true;
}

// The largest lattice point <= target of the lattice t, fl(t + dt), ... (t itself if none): closed form inside a binade, one
// recurrence step across a binade boundary.  Gives up (returns the point reached) where the closed form does not hold.
__device__ __forceinline__ float lattice_floor(float t, float dt, float target) {
    for (int hop = 0; hop < 4; hop++) {
        if (!(t + dt <= target)) break;
        float c;
        uint32_t eb;
        if (!lattice_closed_form(t, dt, 254u, c, eb)) break;
        const float top = __uint_as_float(((eb + 1u) << 23) - 1u);       // the largest float of t's binade
        const float lim = fminf(target, top);
        float k = floorf((lim - t) / c);
        while (t + (k + 1.0f) * c <= lim) k += 1.0f;                       // (products and sums exact: multiples of U below 2^24 U)
        while (k > 0.0f && t + k * c > lim) k -= 1.0f;
        t = t + k * c;
        if (lim == target) break;
        if (!(t + dt <= target)) break;
        t = t + dt;                                                       // the one step that crosses into the next binade
    }
    return t;
}

// Culled start of the device loop (FAST configuration with a cull grid and the per-ray t_end cache).  The reference's iteration 0 marches
// all N rays by one step and the rays without a sample die in its compositing pass; here the exact cull test every ray would run on
// its first march (ray_may_hit: same arguments, same result, the marks read from global memory instead of an LDS copy) runs up front
// for all N rays -- filling the t_end cache -- and iteration 0 then works on the compacted list of the rays that MAY produce a sample:
// dense waves instead of N-ray launches in which most lanes stop at the cull test.  Nothing observable changes: a ray the test rejects
// produces no sample and dies in iteration 0 either way, the survivors of iteration 0 -- and therefore every later iteration, every
// sample and every count -- are the same, and the trace logs N for iteration 0 (SdnLoopRecord::culled_start, advance_record).
// The certified jump.  With a constant step every parameter the marcher visits is a point of the lattice L_0 = t, L_(k+1) = fl(L_k + dt);
// the walk from t visits, of every voxel that holds lattice points, a first one, and leaves it for the first lattice point >= the
// voxel's exit parameter.  Everything before `t_safe` (ray_may_hit) is >= 2 fine voxels away from any occupied voxel, so the walk emits
// nothing there -- it only matters WHERE it stands when it gets there.  lattice_floor gives a lattice point L well before t_safe
// (bit-exact, or it stops early at one); L lies in some run of consecutive lattice points that `locate` puts into the same voxel.
// If every point q of that run has exit_t(q) <= L_a, the first lattice point behind the run, then the walk, wherever in the run it
// lands (it cannot jump the run: the exit parameter of the voxel before it is at most a rounding error beyond the run's first
// point), can never leave it for a point beyond L_a, and every hop advances: L_a is CERTAINLY visited.  The march may start there.
// Returns t when anything is not provable (binade edge, rounding tie, long run).
__device__ __forceinline__ float certified_jump(const MarcherT<true> &m, float t, float t_safe) {
    const float dt = m.dt_const;
    if (!(t_safe > t + 64.0f * dt)) return t;
    const float L = lattice_floor(t, dt, t_safe - 18.0f * dt);
    if (!(L > t)) return t;
    // closed form of the lattice around L (the conditions of lattice_floor, for the 14 steps either side that are looked at)
    float c;
    uint32_t eb;
    if (!(lattice_closed_form(L, dt, 254u, c, eb) && c > 0.0f)) return t;
    if ((__float_as_uint(L - 14.0f * c) >> 23) != eb || (__float_as_uint(L + 14.0f * c) >> 23) != eb) return t;
    float x, y, z;
    int vx, vy, vz, nx, ny, nz;
    m.locate(L, x, y, z, vx, vy, vz);
    // back to the first lattice point of the run
    float q = L;
    int k = 0;
    for (; k < 12; k++) {
        const float qm = q - c;
        if (!(qm > t) || (qm + dt) != q) return t;
        m.locate(qm, x, y, z, nx, ny, nz);
        if (nx != vx || ny != vy || nz != vz) break;
        q = qm;
    }
    if (k == 12) return t;
    // forward over the whole run: the largest exit parameter any of its points computes, and the first point behind it
    float max_tt = -__FLT_MAX__;
    for (k = 0; k < 26; k++) {
        m.locate(q, x, y, z, nx, ny, nz);
        if (nx != vx || ny != vy || nz != vz) break;
        max_tt = fmaxf(max_tt, m.exit_t(q, x, y, z, nx, ny, nz));
        q = q + dt;                                   // the lattice's own recurrence
    }
    if (k == 26 || !(max_tt <= q) || !(q < t_safe - 4.0f * dt)) return t;
    return q;
}

__device__ __forceinline__ bool cull_start_ray(uint32_t n, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                               const float *__restrict__ nears, const float *__restrict__ fars, const uint32_t *__restrict__ cull,
                                               const FrameSel &fs, int32_t *__restrict__ alive_a, float *__restrict__ rays_tend, float bound,
                                               float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H, float *__restrict__ jump,
                                               const float *__restrict__ noises) {
    const uint32_t frame = fs.n_frames > 1 ? n / fs.rays_per_frame : 0u;
    const uint32_t *__restrict__ cull_f = fs.n_frames > 1 ? cull + (size_t)frame * fs.cull_stride : cull;
    const int *meta = reinterpret_cast<const int *>(cull_f + kCullWords);
    const int fx0 = meta[0], fy0 = meta[1], fz0 = meta[2];
    const int fnx = meta[3] - fx0 + 1, fny = meta[4] - fy0 + 1, fnz = meta[5] - fz0 + 1;
    const float t = nears[n], far = fars[n];
    bool go = t < far;
    float t_end = far, start = t;
    if (go) {
        MarcherT<true> m;
        m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, dt_gamma, max_steps, C, H, nullptr);
        // Perturbed first march (SdnRenderCtx::noises): the chain of iteration 0 starts at t0 = near + step_size(near) * noise -- the very
        // expression k_march_rays evaluates -- so t0 is the origin of the step lattice certified_jump walks and the `start` of a ray it
        // certifies nothing for.  The cull scan keeps starting at `near`: it then covers [near, far], a superset of the segment
        // [t0, far] the march can sample, so "no marked cell", t_end and t_safe hold for the march from t0 as they do for the march from
        // near (conservative: a ray whose only marked cells lie in [near, t0) stays on the list, marches, emits nothing and dies in
        // iteration 0 like any other ray without a sample).  No sample changes: both tests only ever REMOVE work that emits nothing.
        const float t0 = noises ? t + m.step_size(t) * noises[n] : t;
        start = t0;
        go = t0 < far;        // a ray perturbed to or past `far` emits nothing (march_ray's own first test)
        float t_safe = -__FLT_MAX__;
        if (go) go = ray_may_hit(cull_f, m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t, far, t_end, fx0, fy0, fz0, fnx, fny, fnz, &t_safe);
        rays_tend[n] = go ? t_end : kTendDead;     // what march_ray would cache on the ray's first march
        if (go && jump && m.dt_is_const) start = certified_jump(m, t0, fminf(t_safe, fminf(far, t_end)));
    }
    alive_a[n] = go ? (int32_t)n : -1;
    if (jump) jump[n] = start;
    return go;
}

__global__ void __launch_bounds__(256) k_cull_start(uint32_t N, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                    const float *__restrict__ nears, const float *__restrict__ fars,
                                                    const uint32_t *__restrict__ cull, FrameSel fs, int32_t *__restrict__ alive_a,
                                                    float *__restrict__ rays_tend, float bound, float dt_gamma, uint32_t max_steps, uint32_t C,
                                                    uint32_t H, float *__restrict__ jump, uint32_t *__restrict__ block_totals,
                                                    const float *__restrict__ noises) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    bool go = false;
    if (n < N) go = cull_start_ray(n, rays_o, rays_d, nears, fars, cull, fs, alive_a, rays_tend, bound, dt_gamma, max_steps, C, H, jump, noises);
    // rays of this 256-ray block that go on: the compaction's scatter sums these (no separate count launch)
    __shared__ uint32_t s_cnt[4];
    const uint32_t c = block_count_256(go, s_cnt);
    if (threadIdx.x == 0) block_totals[blockIdx.x] = c;
}

// after the compaction of the culled start: the list is in alive_b (side 1), n_out[0] rays long
__global__ void k_cull_advance(int32_t *__restrict__ state, const int32_t *__restrict__ n_out, int32_t *__restrict__ trace) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SdnLoopRecord &rec = *sdn_loop(state);
    const int32_t n0 = n_out[0];
    rec.side = 1;
    rec.culled_start = 1;     // iteration 0 runs on the culled list: the trace logs N for it
    if (n0 > 0) {
        rec.n_alive = n0;
    } else {                  // no ray can produce a sample: the reference's iteration 0 (N rays, one step) finds nothing and the loop ends
        trace[0] = rec.N;
        trace[1] = rec.n_step;
        rec.steps_done += rec.n_step;
        rec.iteration = 1;
        rec.n_alive = 0;
    }
}

// snap: 4 x {alive rays entering the next iteration, index of that iteration} -- an immutable per-iteration snapshot the
// host copies out on a side stream while the main stream already runs the next iteration.
__global__ void k_loop_advance(int32_t *__restrict__ state, const int32_t *__restrict__ n_out, int32_t *__restrict__ trace,
                               int32_t *__restrict__ snap, int freeze) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    advance_record<true, true>(*sdn_loop(state), trace, snap, n_out[0], freeze);
}

// Stable compaction of the alive list (256-ray blocks, totals produced by k_composite_rays) fused with the loop advance:
// the workgroup that draws the last ticket -- every workgroup of the launch takes one after its last read of the loop
// record -- sums the totals and advances the record, so no workgroup can see a half-updated record.
__global__ void __launch_bounds__(256) k_scatter_advance(int32_t *__restrict__ alive_a, int32_t *__restrict__ alive_b,
                                                         const uint32_t *__restrict__ block_totals, int32_t *__restrict__ state,
                                                         int32_t *__restrict__ ticket, int32_t *__restrict__ trace, int32_t *__restrict__ snap,
                                                         int freeze) {
    __shared__ uint32_t lds4[4];
    SdnLoopRecord &rec = *sdn_loop(state);
    const uint32_t n = sdn_loop_list_len(rec);
    const int32_t *in = rec.side ? alive_b : alive_a;
    int32_t *out = rec.side ? alive_a : alive_b;
    const uint32_t nb = (n + 255u) / 256u;
    if (blockIdx.x < nb) {
        uint32_t part = 0;
        for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256) part += block_totals[b];
        const uint32_t prev = block_sum_256(part, lds4);
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        ranked_scatter<4>(i < n ? in[i] : -1, prev, out, lds4);
    }
    __syncthreads();
    if (!last_workgroup(ticket)) return;
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) part += block_totals[b];
    const uint32_t total = block_sum_256(part, lds4);
    if (threadIdx.x == 0) advance_record<true, true>(rec, trace, snap, (int32_t)total, freeze);
}

// ---------------------------------------------------------------------------
// steady mode of the device loop: once n_alive <= N / 8 the schedule is n_step = 8 for good (n_alive only shrinks), so
// compositing iteration k and marching iteration k+1 of the same ray can be ONE kernel, and the alive list need not be
// compacted any more (dead entries are skipped; the field network only sees live samples through the live list).
// Two launches per iteration (fused field, composite+march) instead of five.  Samples, schedule and counts are unchanged.
// ---------------------------------------------------------------------------
__global__ void k_steady_begin(int32_t *__restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    SdnLoopRecord &rec = *sdn_loop(state);
    rec.frozen_len = rec.n_alive;
    rec.survivors = 0;
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_composite_march(float T_thresh, int32_t *__restrict__ alive_a, int32_t *__restrict__ alive_b,
                                                         float *__restrict__ rays_t, const float *__restrict__ rays_o,
                                                         const float *__restrict__ rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                                         uint32_t C, uint32_t H, const uint8_t *__restrict__ grid, const float *__restrict__ fars,
                                                         const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                         float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                                                         float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
                                                         const uint32_t *__restrict__ cull, uint32_t *__restrict__ live_idx,
                                                         uint32_t *__restrict__ live_counts, int32_t *__restrict__ state,
                                                         int32_t *__restrict__ ticket, int32_t *__restrict__ trace, int32_t *__restrict__ snap,
                                                         FrameSel fs) {
    __shared__ uint4 s_cull4[FAST ? 256 : 1];
    __shared__ unsigned long long s_fine[FAST ? kFineCacheCells : 1];
    __shared__ uint32_t s_cnt[4], s_min4[4];
    SdnLoopRecord &rec = *sdn_loop(state);
    const uint32_t n_alive = (uint32_t)rec.n_alive, n_step = (uint32_t)rec.n_step, list_len = (uint32_t)rec.frozen_len;
    const int32_t it = rec.iteration;
    int32_t *__restrict__ alive = rec.side ? alive_b : alive_a;
    const bool march_next = (uint32_t)rec.steps_done + n_step < (uint32_t)rec.max_steps;  // `while step < max_steps` admits another iteration
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    bool survives = false;
    uint32_t emitted = 0;
    if (n_alive > 0 && blockIdx.x * 256u < list_len) {  // workgroup-uniform
        const int index = n < list_len ? alive[n] : -1;
        // composite iteration `it` of this ray; survivors march iteration it + 1 below.  The marcher's inputs are fetched together with
        // the compositing's (they land under it, the barriers and the LDS fill), and the ray's new t travels in a register
        RayIn ray;
        float t_new = 0;
        if (index >= 0) {
            if (march_next) ray_in_fetch(ray, index, rays_o, rays_d, fars);
            survives = composite_ray(index, n_step, T_thresh, sigmas + (size_t)n * n_step, rgbs + (size_t)n * n_step * 3,
                                     deltas + (size_t)n * n_step * 2, rays_t, weights_sum, depth, image, &t_new);
            if (!survives) alive[n] = -1;
        }
        frame_rounds<FAST>(fs, survives && march_next, index, grid, cull, s_cull4, s_fine, s_min4,
                           [&](const OccCache &oc, const uint8_t *grid_f, uint32_t frame, bool grouped) __attribute__((always_inline)) {
            float *px = xyzs + (size_t)n * n_step * 3, *pd = dirs + (size_t)n * n_step * 3, *pl = deltas + (size_t)n * n_step * 2;
            MarcherT<FAST> m;
            m.init(ray.o, ray.d, bound, dt_gamma, max_steps, C, H, grid_f);
            float *tend = sdn_loop_tend(rec);
            if (tend) tend += index;
            emitted = march_ray<FAST>(m, oc, t_new, ray.far, n_step, px, pd, pl, tend, grouped ? fs.slot_frame + (size_t)n * n_step : nullptr,
                                      frame);
        });
        live_append(emitted, n, n_step, live_idx, live_counts + it + 1);
    }
    // survivors of this workgroup -> global accumulator; the last workgroup of the launch advances the loop record
    const uint32_t c = block_count_256(survives, s_cnt);
    if (threadIdx.x == 0 && c) atomicAdd(&rec.survivors, (int32_t)c);
    if (!last_workgroup(ticket) || threadIdx.x != 0) return;
    const int32_t n_new = atomicAdd(&rec.survivors, 0);
    rec.survivors = 0;
    advance_record<false, false>(rec, trace, snap, n_new, 0);
}

// image = image + (1 - weights_sum) * bg ; depth = clamp(depth - nears, 0) / (fars - nears)   (dnerf/renderer.py:378-379)
__global__ void __launch_bounds__(256) k_loop_finish(uint32_t N, const float *__restrict__ nears, const float *__restrict__ fars,
                                                     const float *__restrict__ weights_sum, const float *__restrict__ depth,
                                                     const float *__restrict__ image, float bg, float *__restrict__ image_out,
                                                     float *__restrict__ depth_out) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const float w = (1 - weights_sum[n]) * bg;
    image_out[(size_t)n * 3] = image[(size_t)n * 3] + w;
    image_out[(size_t)n * 3 + 1] = image[(size_t)n * 3 + 1] + w;
    image_out[(size_t)n * 3 + 2] = image[(size_t)n * 3 + 2] + w;
    depth_out[n] = fmaxf(depth[n] - nears[n], 0.0f) / (fars[n] - nears[n]);
}

// k_march_rays' arguments by name, for the one function that picks its instantiation (the public marcher and the loop's share it)
struct MarchRays {
    uint32_t threads = 0;                  // lanes to launch
    uint32_t n_alive = 0, n_step = 0;      // 0, 0: the kernel reads them from `state`
    const int32_t *rays_alive = nullptr, *rays_alive_b = nullptr, *state = nullptr;
    const float *rays_t = nullptr, *rays_o = nullptr, *rays_d = nullptr, *fars = nullptr, *noises = nullptr;
    float bound = 0, dt_gamma = 0;
    uint32_t max_steps = 0, C = 0, H = 0, M_pad = 0;
    const uint8_t *grid = nullptr;
    float *xyzs = nullptr, *dirs = nullptr, *deltas = nullptr;
    const uint32_t *cull = nullptr;
    uint32_t *live_idx = nullptr, *live_count = nullptr;
    FrameSel fs;
    const float *jump = nullptr;           // only used with a cull grid
};
int launch_k_march_rays(const MarchRays &m, hipStream_t st) {
    const dim3 g(sdn_div_up(m.threads, 256u)), b(256);
    const uint32_t *cull = cull_grid_applies(m.bound, m.C, m.H) ? m.cull : nullptr;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, g, b, 0, st, m.n_alive, m.n_step, m.rays_alive, m.rays_t, m.rays_o, m.rays_d, m.bound, m.dt_gamma, m.max_steps, m.C,
                           m.H, m.grid, m.fars, m.xyzs, m.dirs, m.deltas, m.noises, m.M_pad, cull, m.live_idx, m.live_count, m.state, m.rays_alive_b,
                           m.fs, cull ? m.jump : (const float *)nullptr);
    };
    if (fast_config(m.bound, m.C, m.H)) launch(k_march_rays<true>); else launch(k_march_rays<false>);
    return sdn_launch_status();
}

}  // namespace

namespace sdn_int {

int loop_begin(const SdnRenderCtx &c, void *mailbox, uint32_t frame_tag, hipStream_t st) {
    const uint32_t threads = c.N > c.n_counters ? c.N : c.n_counters;
    hipLaunchKernelGGL(k_loop_init, dim3(sdn_div_up(threads, 256u)), dim3(256), 0, st, c.N, c.max_steps, c.nears, c.alive_a, c.rays_t, c.weights_sum,
                       c.depth, c.image, c.state, c.live_counts, c.n_counters, (unsigned long long)(uintptr_t)mailbox, frame_tag, c.rays_tend);
    return sdn_launch_status();
}

// Culled start (see k_cull_start): after loop_begin and after the context's cull grid(s) are in place.  Returns 0 without doing
// anything when the configuration has no exact cull test (not the FAST configuration, no cull grid, no t_end cache).
int loop_cull_start(const SdnRenderCtx &c, hipStream_t st) {
    const uint32_t *cull = loop_cull(c);
    if (!cull || !c.rays_tend || !cull_grid_applies(c.bound, c.C, c.H)) return 0;
    uint32_t *block_totals = (uint32_t *)c.block_totals;
    hipLaunchKernelGGL(k_cull_start, dim3(sdn_div_up(c.N, 256u)), dim3(256), 0, st, c.N, c.rays_o, c.rays_d, c.nears, c.fars, cull, frame_sel(c), c.alive_a,
                       c.rays_tend, c.bound, c.dt_gamma, c.max_steps, c.C, c.H, jump_buffer(c), block_totals, c.noises);
    const uint32_t nb = sdn_div_up(c.N, kScanBlock);
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kScanBlock), 0, st, (const int32_t *)c.alive_a, c.N, (const uint32_t *)block_totals, c.alive_b,
                       snap_n_out(c), (const int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, 4u);
    hipLaunchKernelGGL(k_cull_advance, dim3(1), dim3(64), 0, st, c.state, (const int32_t *)snap_n_out(c), c.trace);
    return sdn_launch_status();
}

// the loop's marcher on the alive list (n_alive / n_step from the loop record); jump: the culled start's targets, or nullptr
static int march(const SdnRenderCtx &c, uint32_t bound_alive, const float *jump, hipStream_t st) {
    MarchRays m;
    m.threads = bound_alive + 128u;
    m.rays_alive = c.alive_a; m.rays_alive_b = c.alive_b; m.rays_t = c.rays_t; m.rays_o = c.rays_o; m.rays_d = c.rays_d;
    m.bound = c.bound; m.dt_gamma = c.dt_gamma; m.max_steps = c.max_steps; m.C = c.C; m.H = c.H; m.grid = c.bitfield; m.fars = c.fars;
    m.xyzs = c.xyzs; m.dirs = c.dirs; m.deltas = c.deltas; m.cull = loop_cull(c); m.live_idx = c.live_idx; m.live_count = live_counters(c);
    m.state = c.state; m.fs = frame_sel(c); m.jump = jump;
    m.noises = c.noises;   // per ray, read by the march of iteration 0 only (k_march_rays)
    return launch_k_march_rays(m, st);
}

int loop_march(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st) { return march(c, bound_alive, jump_buffer(c), st); }

int loop_composite_compact(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st, bool freeze) {
    const dim3 g(sdn_div_up(bound_alive, 256u)), b(256);
    uint32_t *block_totals = (uint32_t *)c.block_totals;
    int32_t *snap = snap_ring(c);
    hipLaunchKernelGGL(k_composite_rays, g, b, 0, st, 0u, 0u, c.T_thresh, c.alive_a, c.rays_t, c.sigmas, c.rgbs, c.deltas, c.weights_sum, c.depth, c.image,
                       (const int32_t *)c.state, c.alive_b, block_totals);          // (+ survivors per 256 rays: no separate count launch)
    if (bound_alive > 65536u) {
        // many rays (the first one or two iterations): every scatter workgroup would re-sum thousands of 256-ray totals;
        // use the 1024-ray count / scatter pair and a separate one-thread advance instead.  (Measured again in round 3 with the fused pair up
        // to 131 072 / 262 144 / 524 288 rays: 0.449 / 0.451 / 0.451 ms per frame against 0.441 -- every workgroup of the fused scatter pays a
        // device-scope fence for the last-workgroup election.)
        static_assert(kScanBlock == 1024, "the compositing kernel's 256-ray survivor counts are summed four to a scatter block");
        const uint32_t nb = sdn_div_up(bound_alive, kScanBlock);
        hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kScanBlock), 0, st, (const int32_t *)c.alive_a, 0u, (const uint32_t *)block_totals,
                           c.alive_b, snap_n_out(c), (const int32_t *)c.state, (const int32_t *)c.alive_b, c.alive_a, 4u);
        hipLaunchKernelGGL(k_loop_advance, dim3(1), dim3(64), 0, st, c.state, (const int32_t *)snap_n_out(c), c.trace, snap, freeze ? 1 : 0);
        return sdn_launch_status();
    }
    // n_out doubles as the ticket counter (zero between launches)
    hipLaunchKernelGGL(k_scatter_advance, g, b, 0, st, c.alive_a, c.alive_b, (const uint32_t *)block_totals, c.state, c.n_out, c.trace, snap, freeze ? 1 : 0);
    return sdn_launch_status();
}

int loop_steady_begin(const SdnRenderCtx &c, uint32_t bound_alive, hipStream_t st, bool frozen_already) {
    if (!frozen_already) hipLaunchKernelGGL(k_steady_begin, dim3(1), dim3(64), 0, st, c.state);
    return march(c, bound_alive, nullptr, st);
}

int loop_composite_march(const SdnRenderCtx &c, uint32_t bound_list, hipStream_t st) {
    const dim3 g(sdn_div_up(bound_list, 256u)), b(256);
    const FrameSel fs = frame_sel(c);
    int32_t *snap = snap_ring(c);
    const uint32_t *cull = cull_grid_applies(c.bound, c.C, c.H) ? loop_cull(c) : nullptr;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, g, b, 0, st, c.T_thresh, c.alive_a, c.alive_b, c.rays_t, c.rays_o, c.rays_d, c.bound, c.dt_gamma, c.max_steps, c.C, c.H,
                           c.bitfield, c.fars, c.sigmas, c.rgbs, c.xyzs, c.dirs, c.deltas, c.weights_sum, c.depth, c.image, cull, c.live_idx,
                           live_counters(c), c.state, c.n_out, c.trace, snap, fs);   // (n_out: the ticket counter)
    };
    if (fast_config(c.bound, c.C, c.H)) launch(k_composite_march<true>); else launch(k_composite_march<false>);
    return sdn_launch_status();
}

int loop_finish(const SdnRenderCtx &c, float bg, float *image_out, float *depth_out, hipStream_t st) {
    hipLaunchKernelGGL(k_loop_finish, dim3(sdn_div_up(c.N, 256u)), dim3(256), 0, st, c.N, c.nears, c.fars, c.weights_sum, c.depth, c.image, bg, image_out,
                       depth_out);
    return sdn_launch_status();
}

FrameSel frame_sel(const SdnRenderCtx &c) {
    FrameSel fs;
    if (c.n_group_frames > 1) {
        fs.n_frames = c.n_group_frames;
        fs.rays_per_frame = c.rays_per_frame;
        fs.cull_stride = sdn_cull_grid_bytes() / 4u;
        for (uint32_t f = 0; f < c.n_group_frames && f < SDN_MAX_GROUP_FRAMES; f++) fs.grid[f] = c.frame_bitfield[f];
        fs.slot_frame = c.slot_frame;
    }
    return fs;
}

}  // namespace sdn_int

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

static int launch_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                             const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                             const uint8_t *grid, const float *fars, float *xyzs, float *dirs, float *deltas, const float *noises,
                             uint32_t M_pad, const uint32_t *cull, uint32_t *live_idx, uint32_t *live_count, hipStream_t st) {
    if (n_alive == 0 || n_step == 0) {
        // no sample slots: the M_pad padding slots are still the caller's to read -- the reference hands out zero-filled buffers
        // (raymarching.py:333-335), and no kernel runs here that would clear them
        if (M_pad && xyzs && dirs && deltas) {
            if (hipMemsetAsync(xyzs, 0, (size_t)M_pad * 12, st) != hipSuccess || hipMemsetAsync(dirs, 0, (size_t)M_pad * 12, st) != hipSuccess ||
                hipMemsetAsync(deltas, 0, (size_t)M_pad * 8, st) != hipSuccess)
                return sdn_launch_status();
        }
        return 0;
    }
    if (!rays_alive || !rays_t || !rays_o || !rays_d || !grid || !fars || !xyzs || !dirs || !deltas) return SDN_E_BADARG;
    if (C == 0 || C > 16 || H == 0 || max_steps == 0) return SDN_E_BADARG;
    if ((live_idx == nullptr) != (live_count == nullptr)) return SDN_E_BADARG;
    const uint32_t base = n_alive * n_step;
    if (M_pad < base) M_pad = base;
    MarchRays m;
    m.threads = n_alive + (M_pad - base);  // one lane per alive ray + one per tail slot
    m.n_alive = n_alive; m.n_step = n_step; m.rays_alive = rays_alive; m.rays_t = rays_t; m.rays_o = rays_o; m.rays_d = rays_d;
    m.bound = bound; m.dt_gamma = dt_gamma; m.max_steps = max_steps; m.C = C; m.H = H; m.grid = grid; m.fars = fars;
    m.xyzs = xyzs; m.dirs = dirs; m.deltas = deltas; m.noises = noises; m.M_pad = M_pad; m.cull = cull; m.live_idx = live_idx; m.live_count = live_count;
    return launch_k_march_rays(m, st);
}

int sdn_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                   const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                   const uint8_t *grid, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                   const float *noises, void *stream) {
    (void)nears;  // unused by the reference kernel as well (raymarching.cu:737)
    return launch_march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, fars, xyzs, dirs,
                             deltas, noises, 0, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int sdn_march_rays_ex(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                      const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                      const uint8_t *grid, const float *fars, float *xyzs, float *dirs, float *deltas, const float *noises,
                      uint32_t M_pad, const uint8_t *cull_grid, uint32_t *live_idx, uint32_t *live_count, void *stream) {
    return launch_march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, fars, xyzs, dirs,
                             deltas, noises, M_pad, (const uint32_t *)cull_grid, live_idx, live_count, (hipStream_t)stream);
}

int sdn_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t, const float *sigmas,
                       const float *rgbs, const float *deltas, float *weights_sum, float *depth, float *image, void *stream) {
    if (n_alive == 0 || n_step == 0) return 0;
    if (!rays_alive || !rays_t || !sigmas || !rgbs || !deltas || !weights_sum || !depth || !image) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_rays, dim3(sdn_div_up(n_alive, 256u)), dim3(256), 0, (hipStream_t)stream, n_alive, n_step, T_thresh,
                       rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, (const int32_t *)nullptr, (int32_t *)nullptr,
                       (uint32_t *)nullptr);
    return sdn_launch_status();
}

uint64_t sdn_compact_alive_scratch_bytes(uint32_t n) { return (uint64_t)sdn_div_up(n, kScanBlock) * sizeof(uint32_t); }

int sdn_compact_alive(const int32_t *in, uint32_t n, int32_t *out, int32_t *n_out, void *scratch, void *stream) {
    if (!n_out) return SDN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return (int)hipMemsetAsync(n_out, 0, sizeof(int32_t), st);
    if (!in || !out || !scratch) return SDN_E_BADARG;
    const uint32_t nb = sdn_div_up(n, kScanBlock);
    hipLaunchKernelGGL(k_compact_count, dim3(nb), dim3(kScanBlock), 0, st, in, n, (uint32_t *)scratch, (const int32_t *)nullptr,
                       (const int32_t *)nullptr);
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kScanBlock), 0, st, in, n, (const uint32_t *)scratch, out, n_out,
                       (const int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, 1u);
    return sdn_launch_status();
}

}  // extern "C"
