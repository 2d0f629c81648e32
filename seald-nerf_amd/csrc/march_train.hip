// The training marcher and the training compositors for gfx950 (MI355X).
//
// Holds the counting pass of a training march (lane per ray, and wave per ray for the constant step), the offsets / finish / emit
// kernels behind it, sdn_int::march_rays_train, and the compositing kernels of a training step (forward, backward, whole rays).
// Behavioural contract: raymarching/src/raymarching.cu:312-682 of the reference (march_rays_train and composite_rays_train; line
// ranges cited per kernel).  The stepper, the exact cull test and the lattice closed form come from march_core.h, the block scan from
// block_ops.h; the arithmetic contract (-ffp-contract=off, bit-exact against oracle/sdn_oracle.c) is described there.
#include "march_core.h"
#include "block_ops.h"

namespace {

// ---------------------------------------------------------------------------
// training march: count pass -> deterministic exclusive scan -> write pass
// (raymarching.cu:312-480; the reference allocates slots with two racing atomicAdds)
// ---------------------------------------------------------------------------
template <bool FAST>
__global__ void __launch_bounds__(256) k_march_train_count(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                           const uint8_t *__restrict__ grid, float bound, float dt_gamma,
                                                           uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                                                           const float *__restrict__ nears, const float *__restrict__ fars,
                                                           const float *__restrict__ noises, uint32_t *__restrict__ num_steps_out,
                                                           const uint32_t *__restrict__ cull, float *__restrict__ sample_t) {
    // The one marching pass of a training step: counts every ray's samples AND records their parameters t (sample_t
    // [N, max_steps]), from which the emit pass rebuilds positions and deltas with the marcher's own expressions -- the reference
    // (and the first version of this file) marches every ray a second time to write them.  Same LDS occupancy caches and exact
    // cull-grid early-out as the inference marcher: most rays of a training batch miss the object and stop here at once.
    __shared__ uint4 s_cull4[FAST ? 256 : 1];
    __shared__ unsigned long long s_fine[FAST ? kFineCacheCells : 1];
    OccCache oc;
    occ_cache_load<FAST>(cull, grid, s_cull4, s_fine, oc);
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    MarcherT<FAST> m;
    m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, dt_gamma, max_steps, C, H, grid);
    m.fine = oc.fine; m.fx0 = oc.fx0; m.fy0 = oc.fy0; m.fz0 = oc.fz0; m.fnx = oc.fnx; m.fny = oc.fny; m.fnz = oc.fnz;
    const float far = fars[n];
    float t = nears[n];
    t += m.step_size(t) * noises[n];
    uint32_t num_steps = 0;
    float x, y, z, dt;
    bool go = t < far;
    float t_end = far;
    if (FAST && oc.s_cull && go)
        go = ray_may_hit(oc.s_cull, m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t, far, t_end, oc.fx0, oc.fy0, oc.fz0, oc.fnx, oc.fny, oc.fnz);
    float *ts = sample_t + (size_t)n * max_steps;
    while (go && t < far && t < t_end && num_steps < max_steps) {
        if (m.probe(t, x, y, z, dt, oc.s_cull)) {
            ts[num_steps] = t;
            num_steps++;
            t += dt;
        }
    }
    num_steps_out[n] = num_steps;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Wave-per-ray form of the counting pass (FAST configuration with a constant step, i.e. dt_gamma == 0: what dnerf runs).
//
// With a constant step every parameter the marcher ever visits is a point of ONE lattice  L_0 = t_start, L_{k+1} = fl(L_k + dt):
// a sample advances by dt, and an empty voxel is left by `do t += dt while (t < tt)` -- the same additions.  Which lattice points
// are VISITED is a chain: next(k) = k + 1 if L_k lies in an occupied voxel, else the first m > k with L_m >= tt_k (tt_k: the voxel's
// exit parameter, from L_k alone).  So 64 lanes take 64 consecutive lattice points, evaluate occupancy / exit parameter in
// parallel with the sequential marcher's own expressions, and the wave walks the chain over ballots (scalar work, one readlane
// per empty voxel).  Visited set, samples, counts and the recorded parameters are the sequential kernel's bit for bit: nothing
// is approximated, the dependent chain of ~1000 cycles per voxel probe just becomes one probe round per 64 lattice points.
// One ray per wave instead of one per lane: 4096 rays fill the chip (4 waves per SIMD) where the lane-per-ray kernel kept 64
// waves busy for as long as its longest ray.  Occupancy bits and cull marks are read from global memory (L2-resident, 256 KiB +
// 4 KiB): a probe round is one parallel load, an LDS image per 4-ray workgroup would cost more than it saves.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lane_lattice(float base, float dt, uint32_t lane, float &next_base, float &closed_step) {
    // L_{lane} of the lattice starting at base, by `lane` successive additions (float addition is not associative: the values
    // must come from the recurrence); also returns L_64.
    // Closed form for the common case (lattice_closed_form, and no binade crossing inside the window).  All conditions are
    // wave-uniform; anything else (binade crossing inside the window, a tie, a tiny base) takes the recurrence.
    {
        float c;
        uint32_t eb;
        const bool closed = lattice_closed_form(base, dt, 255u, c, eb);
        const float last = base + 64.0f * c;
        if (closed && eb == (__float_as_uint(last) >> 23)) {
            next_base = last;
            closed_step = c;                                        // L_k = base + k c holds for k = 0 .. 64
            return base + (float)lane * c;
        }
    }
    closed_step = 0.0f;
    float v = base, mine = base;
    #pragma unroll 8
    for (uint32_t i = 0; i < 64; i++) {
        if (i == lane) mine = v;
        v += dt;
    }
    next_base = v;
    return mine;
}

__global__ void __launch_bounds__(256) k_march_train_count_wave(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                                const uint8_t *__restrict__ grid, float bound, uint32_t max_steps, uint32_t N,
                                                                uint32_t H, const float *__restrict__ nears, const float *__restrict__ fars,
                                                                const float *__restrict__ noises, uint32_t *__restrict__ num_steps_out,
                                                                const uint32_t *__restrict__ cull, float *__restrict__ sample_t) {
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (n >= N) return;   // wave-uniform
    MarcherT<true> m;
    m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, 0.0f, max_steps, 1u, H, grid);
    const float far = fars[n], dt = m.dt_const;
    float t0 = nears[n];
    t0 += m.step_size(t0) * noises[n];
    bool go = t0 < far;
    float t_end = far;
    if (cull && go) {
        // ray_may_hit with the scan positions spread over the lanes (same positions: s_i by i successive additions of ds)
        const int *meta = reinterpret_cast<const int *>(cull + kCullWords);
        const int bx0 = meta[0], by0 = meta[1], bz0 = meta[2];
        const int bnx = meta[3] - bx0 + 1, bny = meta[4] - by0 + 1, bnz = meta[5] - bz0 + 1;
        const CullRange r = cull_scan_range(m.ox, m.oy, m.oz, m.dx, m.dy, m.dz, t0, far, bx0, by0, bz0, bnx, bny, bnz);
        const float ds = r.ds, s1 = r.s1;
        if (!r.may) {
            go = false;
        } else {
            bool hit = false, ended = false;
            float base = r.s0;
            for (int round = 0; round < 2 && !ended; round++) {   // 96 scan positions: lanes 0..63, then 0..31
                float nb, unused_step;
                const float s = lane_lattice(base, ds, lane, nb, unused_step);
                base = nb;
                const bool in_range = round == 0 || lane < 32u;
                const float ss = fminf(s, s1);
                const float x = clampf_(m.ox + ss * m.dx, -1.0f, 1.0f), y = clampf_(m.oy + ss * m.dy, -1.0f, 1.0f), z = clampf_(m.oz + ss * m.dz, -1.0f, 1.0f);
                const int cx = (int)fminf((x + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
                const int cy = (int)fminf((y + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
                const int cz = (int)fminf((z + 1) * (0.5f * kCullRes), (float)(kCullRes - 1));
                const bool marked = in_range && cull_marked(cull, cx, cy, cz);
                // the sequential scan stops after the first position with s >= s1 (that position is still tested)
                const unsigned long long stop = __ballot(in_range && s >= s1);
                const uint32_t last = stop ? (uint32_t)__builtin_ctzll(stop) : (round == 0 ? 63u : 31u);
                const unsigned long long mk = __ballot(marked && lane <= last);
                if (mk) {
                    hit = true;
                    const uint32_t top = 63u - (uint32_t)__builtin_clzll(mk);
                    t_end = __shfl(ss + ds, (int)top, 64);
                }
                if (stop) ended = true;
            }
            if (!ended) { t_end = far; hit = true; }   // longer than 96 cells: "may hit, no early end"
            go = hit;
        }
    }
    uint32_t num_steps = 0;
    float *ts = sample_t + (size_t)n * max_steps;
    float base = t0;
    float carry_tt = -__FLT_MAX__;      // exit parameter of an empty voxel whose successor lies beyond the previous window
    // One window = 64 consecutive lattice points, one per lane.  A window's occupancy bytes are loaded while the window BEFORE it is
    // walked (the lattice does not depend on the walk), and for every lattice point, marked by the cull grid or not: the two
    // dependent loads per window of the first version (cull word, then occupancy byte: two L2 round trips with nothing to hide them
    // but three sibling waves doing the same) were the kernel's time.  An unmarked cull cell has no occupied voxel, so reading the
    // voxel's own bit gives the same answer.
    struct Window { float t, nb, cstep, x, y, z; int nx, ny, nz; uint32_t byte, bit; bool act; };
    auto fetch = [&](float from) __attribute__((always_inline)) {
        Window w;
        w.t = lane_lattice(from, dt, lane, w.nb, w.cstep);
        w.act = w.t < far && w.t < t_end;           // the loop condition of the sequential marcher at this lattice point
        // occupancy and (for an empty voxel) the exit parameter, with MarcherT<true>::probe's expressions
        w.x = clampf_(m.ox + w.t * m.dx, -bound, bound); w.y = clampf_(m.oy + w.t * m.dy, -bound, bound); w.z = clampf_(m.oz + w.t * m.dz, -bound, bound);
        w.nx = (int)clampf_((w.x + 1) * m.halfH, 0.0f, m.Hm1); w.ny = (int)clampf_((w.y + 1) * m.halfH, 0.0f, m.Hm1);
        w.nz = (int)clampf_((w.z + 1) * m.halfH, 0.0f, m.Hm1);
        const uint32_t index = morton3D_8bit((uint32_t)w.nx, (uint32_t)w.ny, (uint32_t)w.nz);
        w.byte = grid[index >> 3];                  // positions are clamped: a valid address for every lattice point
        w.bit = index & 7u;
        return w;
    };
    Window cur_w{};
    if (go) cur_w = fetch(base);
    while (go && num_steps < max_steps) {
        const Window nxt_w = fetch(cur_w.nb);
        const float t = cur_w.t, nb = cur_w.nb, cstep = cur_w.cstep, x = cur_w.x, y = cur_w.y, z = cur_w.z;
        const int nx = cur_w.nx, ny = cur_w.ny, nz = cur_w.nz;
        const bool act = cur_w.act;
        const bool occ = act && ((cur_w.byte >> cur_w.bit) & 1u);
        const float tx = ((((float)nx + m.ex) * m.twoRH - 1) - x) * m.rdx;
        const float ty = ((((float)ny + m.ey) * m.twoRH - 1) - y) * m.rdy;
        const float tz = ((((float)nz + m.ez) * m.twoRH - 1) - z) * m.rdz;
        const float tt = t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
        const unsigned long long occ_m = __ballot(act && occ), act_m = __ballot(act);
        // successor of an empty lane inside this window: the first later lattice point >= tt (at least one step), else 64
        // (a 128^3 voxel is crossed in at most 8 steps of dt_min; longer crossings walk on)
        uint32_t nxt = lane + 1u;
        const bool empty = act && !occ;
        if (cstep > 0.0f) {
            // closed-form window (wave-uniform): the lattice values are base + j cstep exactly, so the successor is an index
            // computation per lane -- an estimate by division, then exact comparisons against the lattice values themselves
            if (empty) {
                const float q = (tt - base) / cstep;
                int j = q < 64.0f ? (int)ceilf(q) : 64;
                if (j < (int)lane + 1) j = (int)lane + 1;
                while (j > (int)lane + 1 && base + (float)(j - 1) * cstep >= tt) j--;
                while (j < 64 && base + (float)j * cstep < tt) j++;
                nxt = (uint32_t)j;
            }
        } else {
            for (int k = 0; k < 64; k++) {
                const float lv = __shfl(t, (int)(nxt & 63u), 64);
                const bool more = empty && nxt < 64u && lv < tt;
                if (!__any(more)) break;
                if (more) nxt++;
            }
        }
        // entry point of the chain into this window
        uint32_t cur0 = 0;
        float new_carry = -__FLT_MAX__;
        if (carry_tt != -__FLT_MAX__) {
            const unsigned long long ge = __ballot(t >= carry_tt);
            cur0 = ge ? (uint32_t)__builtin_ctzll(ge) : 64u;
            if (!ge) new_carry = carry_tt;      // the voxel's exit lies beyond this window too: keep walking
        }
        // The walk itself is a SCALAR loop: position, masks, budget and the emitted set live in SGPRs (pinned with readfirstlane --
        // the compiler's uniformity analysis does not see through the loop-carried values and otherwise runs the loop as divergent
        // vector code under exec masks: measured 440 cycles per hop, 55 000 of a long ray's 81 000 cycles).
        uint32_t cur = __builtin_amdgcn_readfirstlane(cur0);
        uint32_t budget = __builtin_amdgcn_readfirstlane(max_steps - num_steps);
        uint32_t emit_lo = 0, emit_hi = 0;
        bool done = false;
        while (cur < 64u) {
            const unsigned long long am = act_m >> cur, om = occ_m >> cur;
            if (!(am & 1ull)) { done = true; break; }                      // t >= far or t >= t_end: the ray is finished
            if (om & 1ull) {
                // a run of occupied lattice points: every one is visited and sampled
                const unsigned long long rest = ~om;
                uint32_t run = rest ? (uint32_t)__builtin_ctzll(rest) : 64u - cur;
                if (run > 64u - cur) run = 64u - cur;
                if (run >= budget) { run = budget; done = true; }
                const unsigned long long bits = ((run >= 64u) ? ~0ull : ((1ull << run) - 1ull)) << cur;
                emit_lo = __builtin_amdgcn_readfirstlane(emit_lo | (uint32_t)bits);
                emit_hi = __builtin_amdgcn_readfirstlane(emit_hi | (uint32_t)(bits >> 32));
                budget = __builtin_amdgcn_readfirstlane(budget - run);
                cur = __builtin_amdgcn_readfirstlane(cur + run);
                if (done) break;
            } else {
                // (v_readlane with a scalar lane index, not an LDS-latency ds_bpermute)
                const uint32_t to = (uint32_t)__builtin_amdgcn_readlane((int)nxt, (int)cur);
                if (to >= 64u) new_carry = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tt), (int)cur));
                cur = to;
            }
        }
        const unsigned long long emit = ((unsigned long long)emit_hi << 32) | emit_lo;
        if ((emit >> lane) & 1ull) ts[num_steps + (uint32_t)__popcll(emit & ((1ull << lane) - 1ull))] = t;
        num_steps = __builtin_amdgcn_readfirstlane(num_steps + (uint32_t)__popcll(emit));
        if (done) break;
        carry_tt = new_carry;
        base = nb;
        cur_w = nxt_w;
    }
    if (lane == 0) num_steps_out[n] = num_steps;
}

// pass A: per-block totals
__global__ void __launch_bounds__(kScanBlock) k_scan_block_totals(const uint32_t *__restrict__ vals, uint32_t N, uint32_t *__restrict__ block_totals) {
    __shared__ uint32_t lds[16];
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t total;
    block_inclusive_scan(i < N ? vals[i] : 0u, lds, total);
    if (threadIdx.x == 0) block_totals[blockIdx.x] = total;
}

// pass B: offsets[i] = exclusive scan (every block re-sums the totals of the blocks before it:
// <= 625 L2-resident words for a full 800x800 frame); writes rays[] and bumps counter[] like
// the reference's atomics would, but in ray order.
__global__ void __launch_bounds__(kScanBlock) k_march_train_offsets(const uint32_t *__restrict__ num_steps, uint32_t N,
                                                                    const uint32_t *__restrict__ block_totals,
                                                                    int32_t *__restrict__ rays, int32_t *__restrict__ counter,
                                                                    uint32_t *__restrict__ base_out) {
    __shared__ uint32_t lds[16];
    __shared__ uint32_t s_prev;
    // sum of previous blocks' totals, cooperatively
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kScanBlock) part += block_totals[b];
    uint32_t prev_total;
    block_inclusive_scan(part, lds, prev_total);
    if (threadIdx.x == 0) s_prev = prev_total;
    __syncthreads();
    const uint32_t base = (uint32_t)counter[0];  // reference semantics: slots start at the counter's current value
    const uint32_t ray_base = (uint32_t)counter[1];
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    const uint32_t v = i < N ? num_steps[i] : 0u;
    uint32_t total;
    const uint32_t incl = block_inclusive_scan(v, lds, total);
    if (i < N) {
        const uint32_t ri = ray_base + i;
        rays[ri * 3] = (int32_t)i;
        rays[ri * 3 + 1] = (int32_t)(base + s_prev + incl - v);
        rays[ri * 3 + 2] = (int32_t)v;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        base_out[0] = base;  // consumed by the write pass; counter itself is bumped by k_march_train_finish
        base_out[1] = s_prev + total;
        base_out[2] = ray_base;
    }
}

// A training batch (N of a few thousand rays) does not need the two-pass scan: ONE workgroup walks the rays in chunks of its size with
// a running carry, writes the ray records and bumps the counters itself (the emit pass takes its bases from base_out) -- three
// launches (block totals, offsets, finish) become one.
__global__ void __launch_bounds__(kScanBlock) k_march_train_offsets_small(const uint32_t *__restrict__ num_steps, uint32_t N, int32_t *__restrict__ rays,
                                                                          int32_t *__restrict__ counter, uint32_t *__restrict__ base_out) {
    __shared__ uint32_t lds[16];
    const uint32_t base = (uint32_t)counter[0], ray_base = (uint32_t)counter[1];
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < N; c0 += kScanBlock) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t v = i < N ? num_steps[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_inclusive_scan(v, lds, total);
        if (i < N) {
            const uint32_t ri = ray_base + i;
            rays[ri * 3] = (int32_t)i;
            rays[ri * 3 + 1] = (int32_t)(base + carry + incl - v);
            rays[ri * 3 + 2] = (int32_t)v;
        }
        carry += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        base_out[0] = base; base_out[1] = carry; base_out[2] = ray_base;
        counter[0] = (int32_t)(base + carry);
        counter[1] = (int32_t)(ray_base + N);
    }
}

__global__ void k_march_train_finish(int32_t *__restrict__ counter, const uint32_t *__restrict__ base_out, uint32_t N) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counter[0] += (int32_t)base_out[1];
        counter[1] += (int32_t)N;
    }
}

// Emit pass: one wave per ray, one lane per sample.  From the recorded t of a sample the marcher's own expressions give its
// position (clamp(o + t d)), its step dt = step_size(t) and the parameter after it, t + dt; delta[1] is the difference of two
// consecutive "after" parameters (the first one against the perturbed start) -- bit for bit what the sequential loop wrote
// (raymarching.cu:427-479), but coalesced and without marching again.
template <bool FAST>
__global__ void __launch_bounds__(256) k_march_train_emit(const float *__restrict__ rays_o, const float *__restrict__ rays_d, float bound,
                                                          float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                                                          const float *__restrict__ nears, const float *__restrict__ noises,
                                                          const int32_t *__restrict__ rays, const uint32_t *__restrict__ bases,
                                                          const float *__restrict__ sample_t, float *__restrict__ xyzs,
                                                          float *__restrict__ dirs, float *__restrict__ deltas) {
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (n >= N) return;
    const uint32_t ray_base = bases[2];              // the ray counter's value before this call (the offsets pass recorded it)
    const uint32_t point_index = (uint32_t)rays[(size_t)(ray_base + n) * 3 + 1];
    const uint32_t num_steps = (uint32_t)rays[(size_t)(ray_base + n) * 3 + 2];
    if (num_steps == 0 || point_index + num_steps > M) return;
    MarcherT<FAST> m;
    m.init(rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, bound, dt_gamma, max_steps, C, H, nullptr);
    float t0 = nears[n];
    t0 += m.step_size(t0) * noises[n];
    const float *ts = sample_t + (size_t)n * max_steps;
    for (uint32_t k = lane; k < num_steps; k += 64u) {
        const float t = ts[k];
        const float dt = m.step_size(t);
        const float after = t + dt;
        float last = t0;
        if (k > 0) { const float tp = ts[k - 1]; last = tp + m.step_size(tp); }
        const size_t p = (size_t)point_index + k;
        xyzs[p * 3] = clampf_(m.ox + t * m.dx, -bound, bound);
        xyzs[p * 3 + 1] = clampf_(m.oy + t * m.dy, -bound, bound);
        xyzs[p * 3 + 2] = clampf_(m.oz + t * m.dz, -bound, bound);
        dirs[p * 3] = m.dx; dirs[p * 3 + 1] = m.dy; dirs[p * 3 + 2] = m.dz;
        deltas[p * 2] = dt;
        deltas[p * 2 + 1] = after - last;
    }
}

// raymarching.cu:501-577
__global__ void __launch_bounds__(256) k_composite_train_fwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                             const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                             uint32_t M, uint32_t N, float T_thresh, float *__restrict__ weights_sum,
                                                             float *__restrict__ depth, float *__restrict__ image) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    if (num_steps == 0 || offset + num_steps > M) {
        weights_sum[index] = 0; depth[index] = 0;
        image[(size_t)index * 3] = 0; image[(size_t)index * 3 + 1] = 0; image[(size_t)index * 3 + 2] = 0;
        return;
    }
    const float *s = sigmas + offset, *c = rgbs + (size_t)offset * 3, *dl = deltas + (size_t)offset * 2;
    uint32_t step = 0;
    float T = 1.0f, r = 0, g = 0, b = 0, ws = 0, t = 0, d = 0;
    while (step < num_steps) {
        const float alpha = 1.0f - sdn_exp_cr(-s[0] * dl[0]);
        const float weight = alpha * T;
        r += weight * c[0]; g += weight * c[1]; b += weight * c[2];
        t += dl[1];
        d += weight * t;
        ws += weight;
        T *= 1.0f - alpha;
        if (T < T_thresh) break;
        s++; c += 3; dl += 2; step++;
    }
    weights_sum[index] = ws; depth[index] = d;
    image[(size_t)index * 3] = r; image[(size_t)index * 3 + 1] = g; image[(size_t)index * 3 + 2] = b;
}

// (CompositeAcc / composite_step, one step of the inference compositing recurrence: sdn_common.h -- the one-pass tint's schedule replay
// in seal.hip finds a ray's termination sample with the same code)

// The INFERENCE compositing arithmetic (kernel_composite_rays, raymarching.cu:819-905: transmittance as 1 - weights_sum, the stop
// test on the transmittance IN FRONT of a sample, t running from the ray's near bound) over ALL samples of a ray at once, in the
// (offset, count) layout of march_rays_train.  With a ray's samples listed up front the iteration loop of the inference branch
// (dnerf/renderer.py:333-381) collapses into march -> field -> this kernel: per ray the same additions in the same order, so image and
// weights_sum are those of the loop bit for bit; the loop only exists to stop marching terminated rays early, which pays for a
// frame of 640 000 rays and costs a chain of ~30 dependent launches for a batch of 4 096.
__global__ void __launch_bounds__(256) k_composite_whole_rays(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                              const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                              const float *__restrict__ nears, uint32_t M, uint32_t N, float T_thresh,
                                                              float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    CompositeAcc a = {0, 0, 0, 0, 0, 0};
    if (num_steps != 0 && offset + num_steps <= M) {
        const float *s = sigmas + offset, *c = rgbs + (size_t)offset * 3, *dl = deltas + (size_t)offset * 2;
        a.t = nears[index];
        for (uint32_t step = 0; step < num_steps; step++) {
            if (dl[0] == 0) break;
            if (composite_step(a, s[0], dl[0], dl[1], c[0], c[1], c[2]) < T_thresh) break;
            s++; c += 3; dl += 2;
        }
    }
    weights_sum[index] = a.weight_sum; depth[index] = a.d;
    image[(size_t)index * 3] = a.r; image[(size_t)index * 3 + 1] = a.g; image[(size_t)index * 3 + 2] = a.b;
}

// raymarching.cu:602-682
__global__ void __launch_bounds__(256) k_composite_train_bwd(const float *__restrict__ grad_weights_sum, const float *__restrict__ grad_image,
                                                             const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                             const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                             const float *__restrict__ weights_sum, const float *__restrict__ image,
                                                             uint32_t M, uint32_t N, float T_thresh, float *__restrict__ grad_sigmas,
                                                             float *__restrict__ grad_rgbs) {
    const uint32_t n = threadIdx.x + blockIdx.x * blockDim.x;
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[n * 3], offset = (uint32_t)rays[n * 3 + 1], num_steps = (uint32_t)rays[n * 3 + 2];
    if (num_steps == 0 || offset + num_steps > M) return;
    const float gws = grad_weights_sum[index];
    const float gi0 = grad_image[(size_t)index * 3], gi1 = grad_image[(size_t)index * 3 + 1], gi2 = grad_image[(size_t)index * 3 + 2];
    const float r_final = image[(size_t)index * 3], g_final = image[(size_t)index * 3 + 1], b_final = image[(size_t)index * 3 + 2];
    const float ws_final = weights_sum[index];
    const float *s = sigmas + offset, *c = rgbs + (size_t)offset * 3, *dl = deltas + (size_t)offset * 2;
    float *gs = grad_sigmas + offset, *gc = grad_rgbs + (size_t)offset * 3;
    uint32_t step = 0;
    float T = 1.0f, r = 0, g = 0, b = 0;
    while (step < num_steps) {
        const float alpha = 1.0f - sdn_exp_cr(-s[0] * dl[0]);
        const float weight = alpha * T;
        r += weight * c[0]; g += weight * c[1]; b += weight * c[2];
        T *= 1.0f - alpha;
        gc[0] = gi0 * weight; gc[1] = gi1 * weight; gc[2] = gi2 * weight;
        gs[0] = dl[0] * (gi0 * (T * c[0] - (r_final - r)) + gi1 * (T * c[1] - (g_final - g)) +
                         gi2 * (T * c[2] - (b_final - b)) + gws * (1 - ws_final));
        if (T < T_thresh) break;
        s++; c += 3; dl += 2; gs++; gc += 3; step++;
    }
}

// byte offsets into the training marcher's scratch: scan workspace | cull grid of the time slice | t of every sample [N, max_steps]
struct TrainScratch { uint64_t cull, sample_t; };
TrainScratch train_scratch(uint32_t N) {
    const uint64_t words = (uint64_t)N + sdn_div_up(N, kScanBlock) + 4u;   // num_steps, block totals, bases
    const uint64_t head = (words * sizeof(uint32_t) + 15u) & ~(uint64_t)15u;
    const uint64_t cull_bytes = ((uint64_t)(kCullWords + 8u) * sizeof(uint32_t) + 15u) & ~(uint64_t)15u;
    return {head, head + cull_bytes};
}

}  // namespace

// prebuilt_cull: the cull grid of `grid` from sdn_build_cull_grid (a caller that marches the same occupancy slice step after step
// keeps it), or nullptr: built here into the scratch
int sdn_int::march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma, uint32_t max_steps, uint32_t N,
                              uint32_t C, uint32_t H, uint32_t M, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                              int32_t *rays, int32_t *counter, const float *noises, void *scratch, const void *prebuilt_cull, hipStream_t st) {
    if (N == 0) return 0;
    if (!rays_o || !rays_d || !grid || !nears || !fars || !xyzs || !dirs || !deltas || !rays || !counter || !noises || !scratch)
        return SDN_E_BADARG;
    if (C == 0 || C > 16 || H == 0 || max_steps == 0 || ((uintptr_t)scratch & 15u) || ((uintptr_t)prebuilt_cull & 15u)) return SDN_E_BADARG;
    uint32_t *num_steps = (uint32_t *)scratch;
    const uint32_t nb = sdn_div_up(N, kScanBlock);
    uint32_t *block_totals = num_steps + N;
    uint32_t *base_out = block_totals + nb;
    const TrainScratch off = train_scratch(N);
    uint32_t *own_cull = (uint32_t *)((unsigned char *)scratch + off.cull);
    const uint32_t *cull = own_cull;
    float *sample_t = (float *)((unsigned char *)scratch + off.sample_t);
    const bool fast = fast_config(bound, C, H);
    const bool use_cull = cull_grid_applies(bound, C, H);
    if (use_cull && prebuilt_cull) {
        cull = (const uint32_t *)prebuilt_cull;
    } else if (use_cull) {
        int rc = sdn_int::build_cull(grid, own_cull, st, false);   // (the scratch has no room for the image)
        if (rc) return rc;
    }
    if (fast && dt_gamma == 0.0f && H <= 256u)   // constant step: one WAVE per ray (k_march_train_count_wave), same samples bit for bit
        hipLaunchKernelGGL(k_march_train_count_wave, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, rays_o, rays_d, grid, bound, max_steps, N, H, nears,
                           fars, noises, num_steps, use_cull ? cull : nullptr, sample_t);
    else if (fast) hipLaunchKernelGGL(k_march_train_count<true>, dim3(sdn_div_up(N, 256u)), dim3(256), 0, st, rays_o, rays_d, grid, bound, dt_gamma,
                                 max_steps, N, C, H, nears, fars, noises, num_steps, use_cull ? cull : nullptr, sample_t);
    else hipLaunchKernelGGL(k_march_train_count<false>, dim3(sdn_div_up(N, 256u)), dim3(256), 0, st, rays_o, rays_d, grid, bound, dt_gamma,
                            max_steps, N, C, H, nears, fars, noises, num_steps, (const uint32_t *)nullptr, sample_t);
    // The reference writes ray records at rays[atomicAdd(counter+1, 1)] and points at atomicAdd(counter, n):
    // both bases are read on the device from the counter the caller hands in (zeroed by dnerf/renderer.py:291-292).
    const bool small = N <= 16u * kScanBlock;
    if (small) {
        hipLaunchKernelGGL(k_march_train_offsets_small, dim3(1), dim3(kScanBlock), 0, st, num_steps, N, rays, counter, base_out);
    } else {
        hipLaunchKernelGGL(k_scan_block_totals, dim3(nb), dim3(kScanBlock), 0, st, num_steps, N, block_totals);
        hipLaunchKernelGGL(k_march_train_offsets, dim3(nb), dim3(kScanBlock), 0, st, num_steps, N, block_totals, rays, counter, base_out);
    }
    if (fast) hipLaunchKernelGGL(k_march_train_emit<true>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, rays_o, rays_d, bound, dt_gamma, max_steps, N, C, H, M,
                                 nears, noises, rays, base_out, sample_t, xyzs, dirs, deltas);
    else hipLaunchKernelGGL(k_march_train_emit<false>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, rays_o, rays_d, bound, dt_gamma, max_steps, N, C, H, M,
                            nears, noises, rays, base_out, sample_t, xyzs, dirs, deltas);
    if (!small) hipLaunchKernelGGL(k_march_train_finish, dim3(1), dim3(64), 0, st, counter, base_out, N);
    return sdn_launch_status();
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

uint64_t sdn_march_rays_train_scratch_bytes(uint32_t N, uint32_t max_steps) {
    return train_scratch(N).sample_t + (uint64_t)N * max_steps * sizeof(float);
}

int sdn_march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                         uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *nears,
                         const float *fars, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                         const float *noises, void *scratch, void *stream) {
    return sdn_int::march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, nears, fars, xyzs, dirs, deltas, rays, counter, noises,
                                     scratch, nullptr, (hipStream_t)stream);
}

int sdn_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, uint32_t M,
                                     uint32_t N, float T_thresh, float *weights_sum, float *depth, float *image, void *stream) {
    if (N == 0) return 0;
    // (M == 0: empty sample tensors have no address; every ray then takes the kernel's `offset + num_steps > M` exit and reads none)
    if ((M != 0 && (!sigmas || !rgbs || !deltas)) || !rays || !weights_sum || !depth || !image) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_train_fwd, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, sigmas, rgbs, deltas, rays, M, N,
                       T_thresh, weights_sum, depth, image);
    return sdn_launch_status();
}

int sdn_composite_whole_rays(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, const float *nears, uint32_t M,
                             uint32_t N, float T_thresh, float *weights_sum, float *depth, float *image, void *stream) {
    if (N == 0) return 0;
    if (!sigmas || !rgbs || !deltas || !rays || !nears || !weights_sum || !depth || !image) return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_whole_rays, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, sigmas, rgbs, deltas, rays, nears, M, N,
                       T_thresh, weights_sum, depth, image);
    return sdn_launch_status();
}

int sdn_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image, const float *sigmas, const float *rgbs,
                                      const float *deltas, const int32_t *rays, const float *weights_sum, const float *image,
                                      uint32_t M, uint32_t N, float T_thresh, float *grad_sigmas, float *grad_rgbs, void *stream) {
    if (N == 0) return 0;
    if (M == 0) return 0;       // no sample, no gradient entry to write
    if (!grad_weights_sum || !grad_image || !sigmas || !rgbs || !deltas || !rays || !weights_sum || !image || !grad_sigmas || !grad_rgbs)
        return SDN_E_BADARG;
    hipLaunchKernelGGL(k_composite_train_bwd, dim3(sdn_div_up(N, 256u)), dim3(256), 0, (hipStream_t)stream, grad_weights_sum, grad_image,
                       sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh, grad_sigmas, grad_rgbs);
    return sdn_launch_status();
}

}  // extern "C"
