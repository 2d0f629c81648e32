// Shared device/host helpers for libsdn_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sdn_hip.h"

#define SDN_WAVE 64

static inline int sdn_launch_status() {
    hipError_t e = hipGetLastError();
    return (int)e;
}

// The loop record (SdnLoopRecord, include/sdn_hip.h) behind the `int32_t *state` every loop kernel and field kernel is handed
static_assert(sizeof(SdnLoopRecord) == 16 * sizeof(int32_t), "SdnRenderCtx::state is 16 ints");
static_assert(offsetof(SdnLoopRecord, n_alive) == 0 && offsetof(SdnLoopRecord, iteration) == 12 && offsetof(SdnLoopRecord, N) == 20 &&
              offsetof(SdnLoopRecord, max_steps) == 24 && offsetof(SdnLoopRecord, culled_start) == 60, "words the host and other files read");
__host__ __device__ __forceinline__ SdnLoopRecord *sdn_loop(int32_t *state) { return reinterpret_cast<SdnLoopRecord *>(state); }
__host__ __device__ __forceinline__ const SdnLoopRecord *sdn_loop(const int32_t *state) { return reinterpret_cast<const SdnLoopRecord *>(state); }
// Length of the alive list the loop kernels walk: the frozen list of the steady mode (dead entries = -1 included) when one exists -- the
// compositing + compaction pass then RE-compacts it (render.hip, FrameRun::enqueue) -- else the compacted list.
__device__ __forceinline__ uint32_t sdn_loop_list_len(const SdnLoopRecord &rec) {
    const int32_t frozen = rec.frozen_len;
    return frozen ? (uint32_t)frozen : (uint32_t)rec.n_alive;
}
__device__ __forceinline__ float *sdn_loop_tend(const SdnLoopRecord &rec) {
    return reinterpret_cast<float *>(((unsigned long long)(uint32_t)rec.tend_hi << 32) | (uint32_t)rec.tend_lo);
}
__device__ __forceinline__ unsigned long long *sdn_loop_mailbox(const SdnLoopRecord &rec) {
    return reinterpret_cast<unsigned long long *>(((unsigned long long)(uint32_t)rec.mailbox_hi << 32) | (uint32_t)rec.mailbox_lo);
}

template <typename T>
static inline T sdn_div_up(T a, T b) { return (a + b - 1) / b; }

// The counter-based generator of the training kernels: splitmix64 of (seed, counter), 64 random bits
__device__ __forceinline__ uint64_t sdn_splitmix64(uint64_t seed, uint32_t i) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1u);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// float(exp(double(x))): agrees with the oracle's correctly rounded exp except for
// double-rounding ties (~1e-9 of inputs); the compositing kernels are HBM/latency
// bound, the fp64 polynomial is free next to their loads.
__device__ __forceinline__ float sdn_exp_cr(float x) { return (float)exp((double)x); }

// One step of the inference compositing recurrence (raymarching.cu:862-887) on a ray's accumulators: the sample of density sigma, step
// dt and colour c, whose parameter lies dt_after behind the previous one.  Returns T, the transmittance IN FRONT of the sample, for the
// caller's stop test; the two early exits (dt == 0 before the step, T < T_thresh after it) stay with the callers.
struct CompositeAcc { float t, weight_sum, d, r, g, b; };
__device__ __forceinline__ float composite_step(CompositeAcc &a, float sigma, float dt, float dt_after, float cr, float cg, float cb) {
    const float alpha = 1.0f - sdn_exp_cr(-sigma * dt);
    const float T = 1 - a.weight_sum;
    const float weight = alpha * T;
    a.weight_sum += weight;
    a.t += dt_after;
    a.d += weight * a.t;
    a.r += weight * cr; a.g += weight * cg; a.b += weight * cb;
    return T;
}
