// Fused dynamic-NeRF field evaluation on MFMA for gfx950 (MI355X), inference.
//
//   (xyz, dir) --freq--> deform MLP (8 x 128) --> xyz' --tiled grid (16 lv x 2)--> sigma MLP (64, 16)
//                                                    dir --SH(4)--^ ++ geo_feat --> color MLP (64, 64, 3)
//
// Behavioural contract: NeRFNetwork.forward of the reference under `-O` (dnerf/network.py:123-169 with torch
// autocast): every Linear takes fp16 inputs / weights, accumulates in fp32 and rounds its output to fp16; the
// encoders run in fp32 (their custom_fwd casts); the grid table and its output are fp16 with the per-corner
// half rounding of kernel_grid (gridencoder.cu:164-191); sigma = exp(fp32(h0)); rgb = fp16(sigmoid(.)).
// In the reference this is 13 cuBLAS GEMMs + ~25 elementwise / encoder kernels per loop iteration, each
// round-tripping [M,128] activations through HBM.  Here it is ONE launch and activations never leave registers.
//
// Mapping (see DESIGN.md "fused field kernel"):
//   * workgroup = 8 waves = 256 sample points (two workgroups per CU: 4 waves per SIMD, <= 128 VGPRs -- measured faster
//     than 6-wave workgroups at 3 waves per SIMD with deeper LDS prefetch: occupancy wins); one wave = 32 points = the N dimension of
//     v_mfma_f32_32x32x16_f16.  Weights are the A operand (M = output features), activations the B operand
//     (K = input features).  The accumulator of layer i (feature rows in registers, point on the lane) converts
//     in place (ReLU, cvt_pk_f16) into the B operand of layer i+1 -- no cross-lane traffic between layers.  The
//     k-order this implies (element j of lane-half h <-> feature 16s + 8(j>>2) + 4h + (j&3)) is baked into the
//     host-side weight packing (dnerf_amd/fused.py), as are the first layer's freq-feature order, the
//     grid-feature order and the SH / geo_feat order of the colour net.
//   * weights (240 fragments of 1 KiB, fragment order) are streamed through LDS in 8 stages
//     (D0 16 KiB | D1..D6 32 KiB each | D7+S0+S1+C0+C1+C2 32 KiB) with direct-to-LDS loads
//     (global_load_lds_dwordx4), double-buffered, one barrier per stage: stage s+1 lands while stage s feeds
//     the MFMAs through conflict-free ds_read_b128 (lane-linear fragments).  HBM/L2 sees each weight byte once
//     per 256 points instead of once per 32.
//   * the time encoding is the same for every point: its contribution W0[:,63:76] . enc(t) is a per-frame
//     bias vector (computed on the host) loaded as the initial accumulator of the first layer.
//   * the 128 table gathers per point are split over the two lane-halves (levels 0-7 / 8-15); row strides,
//     wrap masks and scales of the tiled levels are host-precomputed (no integer division on the device).
//   * optional live-sample index list: only slots that hold a sample are evaluated (the reference evaluates
//     the network on every padded slot).
#include <math.h>
#include <type_traits>
#include <stdlib.h>

#include "sdn_common.h"
#include "sdn_internal.h"
#include "cell_points.h"
#include "grid_common.h"
#include "field_f16_net.h"

namespace {

using namespace sdn_f16;

#ifdef SDN_STAMPS
// Diagnostic build only (make diag; the product library has no stamp): raw shader-clock stamps of k_field_f16, stored as they are taken
// (nothing is kept in registers: the throughput variant has none to spare) by lane 0 of waves 0 and 7 of the first 2048 workgroups.
// g_field_stamps[(2 wg + w) * 32 + k] (w = 0: wave 0, 1: wave 7):
//   k = 0 entry  1 point loaded + freq features  2 first stage barrier passed  3 D0 issued  4..9 hidden layers D1..D6 issued
//   10 last conversion + tail-stage barrier  11 D7 + deformation  12 grid encode  13 sigma net  14 SH + colour net  15 sigmoid + stores
//   16 HW_ID register (CU / SE / SIMD of the wave)  17 XCC_ID register
constexpr uint32_t kStampWGs = 2048;
__device__ unsigned long long g_field_stamps[kStampWGs * 2 * 32];
#define FSTAMP(k) do { __builtin_amdgcn_sched_barrier(0); if (stamp_on) { stamp_slot[k] = __builtin_amdgcn_s_memtime(); } __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define FSTAMP(k) ((void)0)
#endif

constexpr int kStageBytes = 32768;
constexpr int kWaves = 8;                 // waves per workgroup, 32 points each; two workgroups per CU = 4 waves per SIMD
constexpr int kPointsPerWG = 32 * kWaves;

using sdn_cells::cell_uniform;
using sdn_cells::compact_bits3;

// Stage `nbytes` (multiple of 4 KiB) of packed weights global -> LDS, all 256 threads, 16 B per lane per instruction.
// One wave-instruction moves 1 KiB to a wave-uniform LDS base + lane * 16 (global_load_lds_dwordx4).
__device__ __forceinline__ void stage_load(const unsigned char *__restrict__ g, unsigned char *lds, int nbytes, uint32_t wave, uint32_t lane) {
    for (int c = (int)wave; c < nbytes / 1024; c += kWaves) {
        const uint32_t off = __builtin_amdgcn_readfirstlane((uint32_t)c * 1024u);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + off + lane * 16),
                                         (__attribute__((address_space(3))) void *)(lds + off), 16, 0, 0);
    }
}

// One 1-KiB piece of a stage: piece k of this wave (pieces are dealt to the waves round-robin, as stage_load does).
__device__ __forceinline__ void stage_piece(const unsigned char *__restrict__ g, unsigned char *lds, int k, uint32_t wave, uint32_t lane) {
    const uint32_t off = __builtin_amdgcn_readfirstlane((wave + (uint32_t)k * kWaves) * 1024u);
    // (uniform 64-bit base in SGPRs + one 32-bit lane offset: the saddr form of the load, no 64-bit VGPR address per piece)
    const __attribute__((address_space(1))) unsigned char *base = (const __attribute__((address_space(1))) unsigned char *)(g + off);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(base + (lane << 4)),
                                     (__attribute__((address_space(3))) void *)(lds + off), 16, 0, 0);
}

// A staged buffer may be read once (a) every wave's own direct-to-LDS loads have landed -- they are pending LDS writes on the
// VM counter, and hipcc does NOT reliably emit the vmcnt wait in front of __syncthreads() for them (checked in the ISA:
// only lgkmcnt was waited) -- and (b) the workgroup has met at the barrier.
__device__ __forceinline__ void stage_wait_and_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// OCC = waves per SIMD the kernel is compiled for, LA = LDS fragment reads kept in flight ahead of the MFMAs of a hidden layer.
//   <4, 2>: the throughput variant (128 VGPRs, two workgroups per CU) for launches that fill the chip;
//   <2, 8>: the latency variant for launches of at most one workgroup per CU (the tail iterations of a frame, every iteration
//           of a ray-sharded frame): with two waves per SIMD nothing hides an LDS round trip per MFMA, so a whole k-step of
//           fragments is read ahead (256-VGPR budget).
// CELLS: the density-grid query of update_extra_state (dnerf/renderer.py:453-555): slot p is a Morton cell index, the point is
//   that cell's jittered centre, only sigma is evaluated and it is stored at sigmas[p] (a slice of tmp_grid).
// LAYOUT of the fp16 table:
//   kLayoutRef   the reference's (grid.py:118-127): the (x, x+1) pair of a gather is clamped into the level, a wrap is patched;
//   kLayoutPad   every level followed by one extra row that repeats the level's row 0: the (x, x+1) row pair of a gather is always two
//                consecutive rows -- no clamp, no wrap bookkeeping, no patch path; 4 gathers of 8 B per level;
//   kLayoutQuad  one 16-byte BLOCK per row r of a level: rows {r, r+1, r+s1, r+s1+1} (each mod the level's row count) -- the four
//                (x, y) corners of the cell whose low corner is row r (sdn_field_build_quad_table): 2 gathers of 16 B per level.  The
//                phase is bound by the rate at which the texture-address unit takes divergent lane addresses (~1 per cycle and CU:
//                64 gathers per point are as many cycles of that unit as the point's 240 MFMAs are of a matrix pipe), not by bytes:
//                half the gathers, the same values into the same arithmetic.
// The network's stages are field_f16_net.h's; what is written here is this kernel's schedule.
template <int OCC, int LA, bool CELLS, int LAYOUT>
__global__ void __launch_bounds__(64 * kWaves, OCC) k_field_f16(FieldArgs P, TiledLevels lv) {
    constexpr bool PAD = LAYOUT != kLayoutRef;   // (no clamp / wrap bookkeeping in either derived layout)
    constexpr int kGridBatch = OCC >= 4 ? 4 : 8;   // grid levels (per lane-half) whose gathers are in flight together (register budget)
    // Two SEPARATE LDS arrays, and a hidden-layer loop unrolled so that every access names its array at compile time: the compiler
    // treats a direct-to-LDS load as a store to LDS and puts `s_waitcnt vmcnt(0)` in front of every later LDS read it cannot prove
    // disjoint -- with one array indexed by `l & 1` that was every layer's first fragment read, i.e. each layer waited for the
    // NEXT layer's 32 KiB to land before it issued its first MFMA (found in the ISA; ~600 cycles per layer).
    __shared__ __attribute__((aligned(16))) unsigned char s_w0[kStageBytes];
    __shared__ __attribute__((aligned(16))) unsigned char s_w1[kStageBytes];
    // (the largest alignment of the three: the LDS layout pass then places it at offset 0, where its 32 per-level reads address it with
    //  the instructions' 16-bit immediate offsets instead of one v_or_b32 each -- behind the two 32 KiB arrays it sat at 0x10000)
    __shared__ __attribute__((aligned(4096))) uint4 s_lv[16][2];   // per grid level: {offset, s1, s2, hsize}, {mask, scale, -, -}
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#ifdef SDN_STAMPS
    const uint32_t wave_u = __builtin_amdgcn_readfirstlane(wave);
    const bool stamp_on = ((wave_u == 0u) | (wave_u == 7u)) && lane == 0 && blockIdx.x < kStampWGs;
    unsigned long long *stamp_slot = g_field_stamps + ((size_t)blockIdx.x * 2 + (wave_u ? 1 : 0)) * 32;
    FSTAMP(0);
    if (stamp_on) {
        stamp_slot[16] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
        stamp_slot[17] = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // HW_REG_XCC_ID
    }
#endif
    levels_to_lds(s_lv, lv);        // visible to everyone after the first stage barrier below
    const uint32_t count = live_points(P);
    if (blockIdx.x * (uint32_t)kPointsPerWG >= count) return;  // workgroup-uniform: nothing to do, no barrier touched
    const uint32_t n = lane & 31u, h = lane >> 5;
    const uint32_t i = blockIdx.x * (uint32_t)kPointsPerWG + wave * 32u + n;
    const bool valid = i < count;
    const uint32_t ii = valid ? i : (count - 1);  // idle lanes recompute the last point and store nothing
    const uint32_t p = P.live_idx ? P.live_idx[ii] : ii;

    // stage 0 (D0, 16 KiB) -> buf 0 and stage 1 (D1) -> buf 1 start now and land under the feature computation
    stage_load(P.weights + (size_t)kBlkD0 * 1024, s_w0, 16 * 1024, wave, lane);
    stage_load(P.weights + (size_t)kBlkD1 * 1024, s_w1, kStageBytes, wave, lane);

    float x0, x1, x2, d0 = 0, d1 = 0, d2 = 0;
    if constexpr (CELLS) {
        // dnerf/renderer.py:480-490 (== :517-524), the same fp32 operations in the same order:
        //   xyzs = 2 * coords / (grid_size - 1) - 1;  cas_xyzs = xyzs * (bound - half_grid);  cas_xyzs += (rand * 2 - 1) * half_grid
        float xs[3];
        #pragma unroll
        for (int d = 0; d < 3; d++) {
            const float c = (float)compact_bits3(p >> d);
            const float r = P.cell_noise ? P.cell_noise[(size_t)ii * 3 + d] : cell_uniform(P.cell_seed, ii * 3u + (uint32_t)d);
            xs[d] = ((2.0f * c) * P.cell_inv - 1.0f) * P.cell_span + (r * 2.0f - 1.0f) * P.cell_half;
        }
        x0 = xs[0]; x1 = xs[1]; x2 = xs[2];
    } else {
        x0 = P.xyzs[(size_t)p * 3]; x1 = P.xyzs[(size_t)p * 3 + 1]; x2 = P.xyzs[(size_t)p * 3 + 2];
        d0 = P.dirs[(size_t)p * 3]; d1 = P.dirs[(size_t)p * 3 + 1]; d2 = P.dirs[(size_t)p * 3 + 2];
    }

    // ---------------- deform layer 0: freq features, the frame's bias row as the initial accumulator ----------------
    half8 bf[8];
    {
        float sv0[3], cv0[3];
        freq_base(x0, x1, x2, h, sv0, cv0);
        freq_operand(x0, x1, x2, h, sv0, cv0, bf);
    }
    f32x16 acc[4];
    const uint32_t frame = P.slot_frame ? P.slot_frame[p] : 0u;   // kernel-uniform condition
    bias_rows(P.bias0 + 128u * frame, h, acc);
    // Wave priority follows the phase.  All vector instructions of a SIMD share one issue port and the arbiter prefers the oldest
    // wave, so a co-resident workgroup that is in its VALU-only grid phase starves a younger one's MFMAs completely (measured:
    // the second workgroup of a CU made no progress until the first had retired -- two tiles took 28 + 23 us, not ~35).  An MFMA
    // needs the port for 8 of its 32 cycles: with the matrix phases at higher priority the other workgroup's VALU work
    // fills the remaining 24 and the two phases overlap.
    FSTAMP(1);
    __builtin_amdgcn_s_setprio(2);
    stage_wait_and_sync();  // D0 and D1 are resident
    FSTAMP(2);
    #pragma unroll
    for (int ks = 0; ks < 4; ks++) {
        #pragma unroll
        for (int mt = 0; mt < 4; mt++) acc[mt] = mfma(lds_frag(s_w0, mt * 4 + ks, lane), bf[ks], acc[mt]);
    }
    FSTAMP(3);
    // ---------------- deform layers 1..6 (128 -> 128, ReLU): stage l+1 uses buffer (l+1)&1 ----------------
    // One hidden layer: fragments from `cur`, refill of `other` (static arrays: see the comment at their declaration).
    auto hidden_layer = [&](int l, const unsigned char *cur, unsigned char *other) __attribute__((always_inline)) {
        #pragma unroll
        for (int t = 0; t < 4; t++) acc_to_frags<true>(acc[t], bf[2 * t], bf[2 * t + 1]);
        stage_wait_and_sync();  // stage l+1 landed for everyone; everyone is done reading the other buffer (layer l)
        // refill the other buffer with stage l+2 (D(l+2) for l < 5, the tail stage for l == 5); it lands under this layer's MFMAs
        // (its four 1-KiB pieces per wave are issued between this layer's MFMAs, not in front of them: a direct-to-LDS load costs
        // 60-180 cycles of issue)
        const unsigned char *__restrict__ refill_src = P.weights + (size_t)(l < 5 ? kBlkD1 + (l + 1) * 32 : kBlkD7) * 1024;
        // (a software-pipelined variant -- fragments of k-step ks+1 read while the MFMAs of ks run -- needs 32 more VGPRs,
        // i.e. 3 waves per SIMD instead of 4, and measured 20 % slower: latency is hidden by occupancy here)
        // look-ahead: the LDS reads of fragments i+1 .. i+LA are in flight while MFMA i issues
        half8 ring[LA];
        #pragma unroll
        for (int j = 0; j < LA; j++) ring[j] = lds_frag(cur, (j & 3) * 8 + (j >> 2), lane);
        #pragma unroll
        for (int i = 0; i < 32; i++) {
            const int ks = i >> 2, mt = i & 3;
            const half8 a = ring[i % LA];
            if (i + LA < 32) ring[i % LA] = lds_frag(cur, ((i + LA) & 3) * 8 + ((i + LA) >> 2), lane);
            if ((i & 7) == 1 && (i >> 3) < kStageBytes / 1024 / kWaves) stage_piece(refill_src, other, i >> 3, wave, lane);
            acc[mt] = mfma(a, bf[ks], ks == 0 ? zero_tile() : acc[mt]);
        }
        // pin the interleaving the look-ahead needs (left alone, the scheduler sinks every read to just before its MFMA to save
        // registers, and each MFMA then waits out a full LDS round trip): LA reads, then MFMA / read alternating
        __builtin_amdgcn_sched_group_barrier(0x100, LA, 0);
        #pragma unroll
        for (int i = 0; i < 32 - LA; i++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, LA, 0);
    };
    #pragma unroll 1
    for (int lp = 0; lp < 3; lp++) {      // layers 2 lp (reads s_w1, refills s_w0) and 2 lp + 1 (the other way round)
        hidden_layer(2 * lp, s_w1, s_w0);
        FSTAMP(4 + 2 * lp);
        hidden_layer(2 * lp + 1, s_w0, s_w1);
        FSTAMP(5 + 2 * lp);
    }
    #pragma unroll
    for (int t = 0; t < 4; t++) acc_to_frags<true>(acc[t], bf[2 * t], bf[2 * t + 1]);
    stage_wait_and_sync();  // tail stage (D7 | S0 | S1 | C0 | C1 | C2) resident in buffer 1
    FSTAMP(10);
    const unsigned char *tail = s_w1;

    float u[3];
    grid_coords(deform_d7(tail, bf, lane), lane, x0, x1, x2, (P.zero_deform >> frame) & 1, P, u);
    __builtin_amdgcn_s_setprio(0);
    FSTAMP(11);
    // ---------------- grid encode: lane-half h evaluates levels 8h .. 8h+7 ----------------
    uint32_t gfw[2][4];   // 8 levels x 2 features as packed pairs
    {
        const bool oob = out_of_grid(u);
        const unsigned char *__restrict__ table_bytes = reinterpret_cast<const unsigned char *>(P.table);
        // per level: the constants from their LDS copy, the cell (field_f16_net.h) and the row of its low corner -- row 0 for a point outside
        struct LevelCell { uint32_t offset, s1, s2, hsize, mask, base; };
        auto cell_of = [&](int li, float (&fr)[3]) {
            const uint4 k0 = s_lv[8 * h + li][0], k1 = s_lv[8 * h + li][1];
            return LevelCell{k0.x, k0.y, k0.z, k0.w, k1.x, level_cell(k0, k1, u, fr, oob)};
        };
        #pragma unroll
        for (int lb = 0; lb < 8 / kGridBatch; lb++) {
            float pos[kGridBatch][3];
            if constexpr (LAYOUT == kLayoutQuad) {
                // one 16-byte block = the four (x, y) corners of a cell: 2 gathers per level (z and z + 1).  All gathers of the batch are
                // issued back to back (independent, L2 / Infinity Cache latency overlapped) before any is consumed.
                uint4 quads[kGridBatch][2];
                #pragma unroll
                for (int lq = 0; lq < kGridBatch; lq++) {
                    const LevelCell c = cell_of(lb * kGridBatch + lq, pos[lq]);
                    const uint32_t r0 = c.base & c.mask, r1 = (c.base + c.s2) & c.mask;
                    // (uniform 64-bit base + 32-bit byte offset: the host refuses tables of 2^28 blocks or more)
                    __builtin_memcpy(&quads[lq][0], table_bytes + ((c.offset + r0) << 4), 16);
                    __builtin_memcpy(&quads[lq][1], table_bytes + ((c.offset + r1) << 4), 16);
                }
                #pragma unroll
                for (int lq = 0; lq < kGridBatch; lq++) {
                    const int li = lb * kGridBatch + lq;
                    const uint32_t feat = interp_corners(pos[lq], [&](uint32_t idx) { return quad_corner(quads[lq], idx); });
                    gfw[li >> 2][li & 3] = oob ? 0u : feat;
                }
            } else {
                // The x and x+1 corners of a (y, z) corner pair are neighbouring table rows, so one 8-byte gather fetches both:
                // 4 gathers per level instead of 8.
                uint2 pairs[kGridBatch][4];
                uint32_t wrapbits = 0;   // bit 4 lq + c: that gather's x corner is the last row of a capped level (x+1 wraps to row 0)
                #pragma unroll
                for (int lq = 0; lq < kGridBatch; lq++) {
                    const LevelCell lc = cell_of(lb * kGridBatch + lq, pos[lq]);
                    #pragma unroll
                    for (uint32_t c = 0; c < 4; c++) {
                        const uint32_t row0 = (lc.base + ((c & 1u) ? lc.s1 : 0u) + ((c & 2u) ? lc.s2 : 0u)) & lc.mask;
                        // the pair (rl, rl + 1) is always inside the level (PAD: row hsize exists and repeats row 0)
                        const uint32_t rl = PAD ? row0 : min(row0, lc.hsize - 2u);
                        __builtin_memcpy(&pairs[lq][c], table_bytes + ((lc.offset + rl) << 2), 8);   // 4-byte aligned 8-byte gather
                        if (!PAD && row0 > rl) wrapbits |= 1u << (4 * lq + (int)c);
                    }
                }
                // On a capped level the x corner may be the LAST row: it is then the second row of the pair that was fetched and the
                // x+1 corner is row 0.  Patched after every gather of the batch has been issued (a branch per gather would make each
                // wait for its own data); practically never taken (1 row in 2^19).
                if (!PAD && __builtin_expect(wrapbits != 0u, 0)) {
                    #pragma unroll
                    for (int lq = 0; lq < kGridBatch; lq++) {
                        #pragma unroll
                        for (uint32_t c = 0; c < 4; c++) {
                            if ((wrapbits >> (4 * lq + (int)c)) & 1u) {
                                const int li = lb * kGridBatch + lq;   // wrapped: row0 == mask, so the x+1 corner is row 0 of the level
                                const uint32_t offset = s_lv[8 * h + li][0].x;
                                pairs[lq][c].x = pairs[lq][c].y;
                                pairs[lq][c].y = *reinterpret_cast<const uint32_t *>(table_bytes + (offset << 2));
                            }
                        }
                    }
                }
                #pragma unroll
                for (int lq = 0; lq < kGridBatch; lq++) {
                    const int li = lb * kGridBatch + lq;
                    const uint32_t feat = interp_corners(pos[lq], [&](uint32_t idx) { return (idx & 1u) ? pairs[lq][idx >> 1].y : pairs[lq][idx >> 1].x; });
                    gfw[li >> 2][li & 3] = oob ? 0u : feat;
                }
            }
            // keep the batches apart: hoisting the next batch's index math and gathers above this batch's interpolation doubles the
            // live registers (spills under the 128-VGPR cap of the throughput variant)
            if (lb + 1 < 8 / kGridBatch) __builtin_amdgcn_sched_barrier(0);
        }
    }
    FSTAMP(12);
    half8 gf[2];
    grid_operand(gfw, gf);
    const f32x16 hv = sigma_net(tail, gf, lane);
    const float sigma = density(hv, P.density_scale);
    if constexpr (CELLS) {
        if (h == 0 && valid) P.sigmas[p] = sigma;   // duplicates in the list: any one of them wins, as with tmp_grid[indices] = sigmas
        return;
    }
    FSTAMP(13);
    half8 cf[2] = {geo_operand(hv), sh_operand(d0, d1, d2, h)}, c2f[4];
    f32x16 c1[2];
    colour_hidden(tail, cf, lane, c1);
    relu_frags(c1, c2f);
    const f32x16 co = colour_out(tail, c2f, lane);
    FSTAMP(14);
    if (h == 0 && valid) store_sigma_rgb(P, p, sigma, co);
    FSTAMP(15);
}

// The reference sizes every level to a multiple of 8 rows (grid.py:124).  The two derived layouts are self-describing through the
// offsets they come with: a PADDED table (one extra row per level repeating the level's row 0) has level sizes == 1 mod 8, a QUAD table
// (one 16-byte block per row, two unused blocks behind every level) == 2 mod 8 (dnerf_amd/fused.py builds both).
int table_layout(const int32_t *offsets_host) {
    uint32_t seen = 0;
    for (uint32_t l = 0; l < 16; l++) {
        const uint32_t r = (uint32_t)(offsets_host[l + 1] - offsets_host[l]) & 7u;
        seen |= 1u << r;
    }
    return seen == 2u ? kLayoutPad : (seen == 4u ? kLayoutQuad : kLayoutRef);
}
bool table_is_padded(const int32_t *offsets_host) { return table_layout(offsets_host) == kLayoutPad; }

// 1 / v when v is a (normal) power of two -- x / v == x * (1 / v) exactly for every x -- else 0
float exact_reciprocal(float v) {
    int e = 0;
    if (!(v > 0.0f) || !isfinite(v) || frexpf(v, &e) != 0.5f || e < -100 || e > 100) return 0.0f;
    return 1.0f / v;
}

// D = 3 (the deformation and temporal-basis models' grid) or 4 (the ambient-dimension model's: s3 [16] receives the fourth stride)
int fill_tiled_levels(TiledLevels &lv, const int32_t *offsets_host, float S, uint32_t H, uint32_t D = 3, uint32_t *s3 = nullptr) {
    if (D != 3 && !(D == 4 && s3)) return SDN_E_BADARG;
    const int layout = table_layout(offsets_host);
    for (uint32_t l = 0; l < 16; l++) {
        const uint32_t hsize = (uint32_t)(offsets_host[l + 1] - offsets_host[l]) - (layout == kLayoutPad ? 1u : (layout == kLayoutQuad ? 2u : 0u));
        if (hsize == 0 || (uint32_t)offsets_host[16] >= (1u << 28)) return SDN_E_BADARG;   // (32-bit byte offsets into the table)
        const float scale = exp2f((float)l * S) * (float)H - 1.0f;  // gridencoder.cu:138
        const uint32_t res = (uint32_t)ceil((double)scale) + 1;      // gridencoder.cu:139
        // get_grid_index (gridencoder.cu:66-84) for align_corners = false, gridtype = tiled:
        //   stride = 1; for d: if (stride <= hsize) { index += pos[d] * stride; stride *= res + 1; }
        // (64-bit here: a stride that no longer fits is never used -- the loop has stopped by then)
        uint64_t stride = 1;
        uint32_t s[4] = {0, 0, 0, 0};
        for (uint32_t d = 0; d < D && stride <= hsize; d++) {
            s[d] = (uint32_t)stride;
            stride *= (res + 1);
        }
        if (s[0] != 1) return SDN_E_BADARG;
        // (the 4-D kernel forms cell x stride with 24-bit multiplies, as level_cell does: strides never exceed the level's size)
        if (D == 4 && hsize > (1u << 24)) return SDN_E_UNSUPPORTED;
        if (s3) s3[l] = s[3];
        lv.offset[l] = (uint32_t)offsets_host[l];
        lv.s1[l] = s[1];
        lv.s2[l] = s[2];
        lv.hsize[l] = hsize;
        const bool pow2 = (hsize & (hsize - 1)) == 0;
        // a non-power-of-two level must be dense (every corner has its own row), otherwise the AND/min form would be wrong
        if (!pow2 && (s[D - 1] == 0 || stride > hsize)) return SDN_E_UNSUPPORTED;
        lv.mask[l] = pow2 ? hsize - 1 : 0xFFFFFFFFu;
        lv.scale[l] = scale;
    }
    return 0;
}

#include "field_pp.inc"

// Quad table: block (offset_q[l] + r) of level l = rows {r, r + 1, r + s1, r + s1 + 1} of the level, each mod its row count, as fp16 pairs
// (the corners (x, y), (x+1, y), (x, y+1), (x+1, y+1) of the cell whose low corner is row r: get_grid_index adds 1 / s1 per step and
// takes the sum mod the row count, gridencoder.cu:66-84).  T = float or __half (rounded to fp16 as grid.py:43-44's `.half()` does).
struct QuadLevels { uint32_t src[17]; uint32_t s1[16]; };
template <typename T>
__global__ void k_build_quad_table(const T *__restrict__ emb, QuadLevels q, uint4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // source row
    if (i >= q.src[16]) return;
    uint32_t l = 0;
    #pragma unroll
    for (uint32_t k = 1; k < 16; k++) l += (i >= q.src[k]) ? 1u : 0u;
    const uint32_t a = q.src[l], hs = q.src[l + 1] - a, r = i - a, s1 = q.s1[l];
    auto row = [&](uint32_t rr) {
        const T *p = emb + (size_t)(a + rr % hs) * 2;
        const __half2 v = __halves2half2(__float2half_rn((float)p[0]), __float2half_rn((float)p[1]));
        return __builtin_bit_cast(uint32_t, v);
    };
    out[i + 2u * l] = make_uint4(row(r), row(r + 1u), row(r + s1), row(r + s1 + 1u));
}

}  // namespace

namespace sdn_int {

static int g_field_pp = -1;   // 1: large launches take the persistent ping-pong kernel (default), 0: never; -1: read SDN_FIELD_PP
static int g_field_pp_wgs = 0;   // workgroups of a persistent launch; 0 = one per CU
constexpr uint32_t kPPMinTilesPerCU = 4;   // launches of at least this many 256-point tiles per CU take the persistent kernel

// the kernels' argument records of one call (cell fields zero: field_cells_f16 sets its own)
int field_table_layout(const int32_t *offsets_host) { return table_layout(offsets_host); }
int fill_tiled_levels_nd(TiledLevels &lv, uint32_t (*s3)[16], uint32_t D, const int32_t *offsets_host, float S, uint32_t H) {
    return fill_tiled_levels(lv, offsets_host, S, H, D, s3 ? *s3 : nullptr);
}
int fill_field_args(FieldArgs &a, TiledLevels &lv, const FieldCall &f) {
    int rc = fill_tiled_levels(lv, f.offsets_host, f.S, f.H);
    if (rc) return rc;
    fill_field_record(a, f);
    return 0;
}
void fill_field_record(FieldArgs &a, const FieldCall &f) {
    a.xyzs = f.xyzs; a.dirs = f.dirs; a.live_idx = f.live_idx; a.live_count = f.live_count; a.state = f.state; a.M = f.M;
    a.weights = (const unsigned char *)f.weights; a.bias0 = f.bias0; a.table = (const __half *)f.table;
    a.sigmas = f.sigmas; a.rgbs = f.rgbs; a.bound = f.bound; a.density_scale = f.density_scale; a.zero_deform = f.zero_deform;
    a.inv_2bound = exact_reciprocal(2 * f.bound);
    a.slot_frame = f.slot_frame; a.n_frames = field_n_frames(f);
    a.cell_noise = nullptr; a.cell_seed = 0; a.cell_inv = a.cell_span = a.cell_half = 0;
    a.pp_soft = 0;
}

// One-tile-per-workgroup launch: the table layout x the variant (small: the latency variant, at most one workgroup per CU).  A
// reference-layout table (the public entry point with a caller's own table) has one variant only -- with the wrap bookkeeping the
// throughput variant does not fit 128 VGPRs without spilling; the derived layouts are the product path -- and no density query.
template <bool CELLS>
static void launch_tile(int layout, bool small, uint32_t wgs, const FieldArgs &a, const TiledLevels &lv, hipStream_t st) {
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(wgs), dim3(64 * kWaves), 0, st, a, lv); };
    if (layout == kLayoutQuad) small ? go(k_field_f16<2, 8, CELLS, kLayoutQuad>) : go(k_field_f16<4, 2, CELLS, kLayoutQuad>);
    else if (layout == kLayoutPad) small ? go(k_field_f16<2, 8, CELLS, kLayoutPad>) : go(k_field_f16<4, 2, CELLS, kLayoutPad>);
    else if constexpr (!CELLS) go(k_field_f16<2, 8, false, kLayoutRef>);
}

// launch used by both the C entry point and the device-driven render loop (render.hip)
int field_forward_f16(const FieldCall &f, hipStream_t st) {
    TiledLevels lv;
    FieldArgs a;
    int rc = fill_field_args(a, lv, f);
    if (rc) return rc;
    const uint32_t M = f.M, expect_points = f.expect_points;
    const uint32_t wgs = sdn_div_up(M, (uint32_t)kPointsPerWG);
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
    }
    // expect_points (0 = unknown): the caller's estimate of the live points when M is only a loose bound of them
    const uint32_t busy = expect_points ? sdn_div_up(expect_points < M ? expect_points : M, (uint32_t)kPointsPerWG) : wgs;
    // latency variant (one workgroup per CU, deep LDS read-ahead) while the launch is at most one workgroup per CU.  (Measured,
    // profiles/r02_field_latency_rounds.txt: running 2+ ROUNDS of lone workgroups instead of one round of co-resident pairs is
    // slower -- 57.6 vs 51.9 us at 126 976 points.)
    bool small = busy <= (uint32_t)cus;
    {   // SDN_FIELD_VARIANT=throughput / latency pins the variant (measurements only)
        static int pin = -1;
        if (pin < 0) {
            const char *e = getenv("SDN_FIELD_VARIANT");
            pin = !e ? 0 : (e[0] == 't' ? 1 : (e[0] == 'l' ? 2 : 0));
        }
        if (pin == 1) small = false;
        if (pin == 2) small = true;
    }
    const int layout = table_layout(f.offsets_host);
    // persistent ping-pong form (field_pp.inc): one 16-wave workgroup per CU walking tile pairs, for launches of at least two rounds of
    // the CUs (SDN_FIELD_PP=0 keeps every launch on the one-tile-per-workgroup kernels: measurements only)
    if (g_field_pp < 0) {
        const char *e = getenv("SDN_FIELD_PP");
        g_field_pp = e ? atoi(e) : 1;
    }
    if (g_field_pp && layout == kLayoutQuad && busy >= kPPMinTilesPerCU * (uint32_t)cus && a.n_frames <= kPPMaxFrames && M < (1u << 28)) {
        const uint32_t pairs = sdn_div_up(M, kPPTile);     // (tiles: the unit the kernel deals out)
        int pp_cus = g_field_pp_wgs > 0 ? g_field_pp_wgs : cus;
        if (pp_cus > cus) pp_cus = cus;
        // The launch covers every CU; the kernel, which knows the live count, keeps G of the workgroups (the others leave at once):
        // the fewest that finish in as many rounds as `pp_cus` would need -- or, when one workgroup per CU saves a whole round over
        // `pp_cus`, the fewest that finish in that many (SDN_FIELD_PP_BALANCE=0: exactly pp_cus, as before; 2: never more than pp_cus)
        static int balance = -1;
        if (balance < 0) {
            const char *e = getenv("SDN_FIELD_PP_BALANCE");
            balance = e ? atoi(e) : 0;
        }
        const uint32_t grid = balance == 1 ? (uint32_t)cus : (uint32_t)pp_cus;
        a.pp_soft = (uint32_t)pp_cus | (balance == 0 ? 0x80000000u : (balance == 2 ? 0x40000000u : 0u));
        hipLaunchKernelGGL(k_field_pp_f16, dim3(pairs < grid ? pairs : grid), dim3(64 * kPPWaves), 0, st, a, lv);
        return sdn_launch_status();
    }
    launch_tile<false>(layout, small, wgs, a, lv, st);
    return sdn_launch_status();
}

// sigma * density_scale of jittered occupancy-grid cell centres -> tmp_grid slice (density.hip drives the whole update)
int field_cells_f16(const FieldCells &q, hipStream_t st) {
    TiledLevels lv;
    FieldArgs a;
    int rc = fill_field_args(a, lv, q.f);
    if (rc) return rc;
    a.cell_noise = q.noise; a.cell_seed = q.seed;
    const float half_grid = q.cas_bound / (float)q.grid_size;
    a.cell_inv = 1.0f / (float)(q.grid_size - 1); a.cell_span = q.cas_bound - half_grid; a.cell_half = half_grid;
    const uint32_t wgs = sdn_div_up(q.f.M, (uint32_t)kPointsPerWG);
    const int layout = table_layout(q.f.offsets_host);
    if (layout == kLayoutRef) return SDN_E_UNSUPPORTED;   // the density query is only built for the derived layouts
    launch_tile<true>(layout, wgs <= 256u, wgs, a, lv, st);
    return sdn_launch_status();
}

}  // namespace sdn_int

extern "C" {

uint32_t sdn_field_weight_blocks(void) { return (uint32_t)kBlkTotal; }

// Kernel selection for large launches of the fused field network: 1 = persistent ping-pong kernel (the default), 0 = one tile per
// workgroup for every launch (the two produce identical bits; tests and A/B measurements switch here), -1 = back to SDN_FIELD_PP / default.
void sdn_field_select_kernel(int persistent) { sdn_int::g_field_pp = persistent; }
// Workgroups of a persistent launch (0 = one per CU, the default).  A stream of frames in several loop contexts leaves an eighth of the
// CUs to the other frames' marchers and compositors -- which cannot share a CU with a 16-wave, 156-KiB workgroup and otherwise wait
// for a whole persistent launch to end: 0.410 -> 0.398 ms per frame with 224 of 256 (profiles/r04_field_pp_kernel.txt).
void sdn_field_persistent_workgroups(int n) { sdn_int::g_field_pp_wgs = n > 0 ? n : 0; }

// Builds the fused kernel's QUAD table (16 bytes per row, see kLayoutQuad) from embeddings in the reference layout.
//   embeddings [ref_offsets_host[16], 2] of dtype (SDN_F32 / SDN_F16), ref_offsets_host [17] the reference's level offsets (grid.py:118-127);
//   out: (ref_offsets_host[16] + 32) blocks of 16 bytes -- level l starts at block ref_offsets_host[l] + 2 l (pass those 17 values as
//   `offsets_host` to the field entry points: level sizes == 2 mod 8 announce the layout).
int sdn_field_build_quad_table(const void *embeddings, int dtype, const int32_t *ref_offsets_host, float S, uint32_t H, void *out, void *stream) {
    return sdn_field_build_quad_table_nd(embeddings, dtype, 3, ref_offsets_host, S, H, out, stream);
}
// The same for a grid of input_dim 3 or 4: a QUAD block is the four (x, y) corners whatever lies above them, so only the levels'
// validation depends on the dimension; the blocks of a 3-D table are what sdn_field_build_quad_table writes.
int sdn_field_build_quad_table_nd(const void *embeddings, int dtype, uint32_t input_dim, const int32_t *ref_offsets_host, float S, uint32_t H, void *out,
                                  void *stream) {
    if (!embeddings || !ref_offsets_host || !out || ((uintptr_t)out & 15u) != 0) return SDN_E_BADARG;
    TiledLevels lv;
    uint32_t s3[16];
    int rc = fill_tiled_levels(lv, ref_offsets_host, S, H, input_dim, s3);   // (reference offsets: level sizes are multiples of 8)
    if (rc) return rc;
    QuadLevels q;
    for (int l = 0; l < 17; l++) q.src[l] = (uint32_t)ref_offsets_host[l];
    for (int l = 0; l < 16; l++) q.s1[l] = lv.s1[l];
    const uint32_t rows = q.src[16];
    if (rows == 0) return SDN_E_BADARG;
    if (hipMemsetAsync(out, 0, ((size_t)rows + 32) * 16, (hipStream_t)stream) != hipSuccess) return sdn_launch_status();
    if (dtype == SDN_F32)
        hipLaunchKernelGGL(k_build_quad_table<float>, dim3(sdn_div_up(rows, 256u)), dim3(256), 0, (hipStream_t)stream, (const float *)embeddings, q, (uint4 *)out);
    else if (dtype == SDN_F16)
        hipLaunchKernelGGL(k_build_quad_table<__half>, dim3(sdn_div_up(rows, 256u)), dim3(256), 0, (hipStream_t)stream, (const __half *)embeddings, q, (uint4 *)out);
    else
        return SDN_E_BADARG;
    return sdn_launch_status();
}

#ifdef SDN_STAMPS
// diagnostic build only: the persistent kernel's slot stamps (g_pp_stamps: 256 workgroups x 2 sets x 128 words), cleared behind the copy
int sdn_debug_pp_stamps(unsigned long long *out) {
    if (!out) return SDN_E_BADARG;
    if (hipDeviceSynchronize() != hipSuccess) return sdn_launch_status();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pp_stamps), sizeof(unsigned long long) * 256 * 2 * 128) != hipSuccess) return sdn_launch_status();
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_pp_stamps)) != hipSuccess) return sdn_launch_status();
    return (int)hipMemset(p, 0, sizeof(unsigned long long) * 256 * 2 * 128);
}
// diagnostic build only: copies out and clears the field kernel's stamp sums (see g_field_stamps)
// (out: sdn_debug_field_stamp_words() 64-bit words; the buffer is cleared behind the copy)
uint32_t sdn_debug_field_stamp_words(void) { return kStampWGs * 2 * 32; }
int sdn_debug_field_stamps(unsigned long long *out) {
    if (!out) return SDN_E_BADARG;
    if (hipDeviceSynchronize() != hipSuccess) return sdn_launch_status();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_field_stamps), sizeof(unsigned long long) * kStampWGs * 2 * 32) != hipSuccess) return sdn_launch_status();
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_field_stamps)) != hipSuccess) return sdn_launch_status();
    return (int)hipMemset(p, 0, sizeof(unsigned long long) * kStampWGs * 2 * 32);
}
#endif

// Fused field forward, `-O` numerics (fp16 MLPs / table, fp32 encoders).  weights: packed by dnerf_amd/fused.py
// (sdn_field_weight_blocks() KiB); bias0 [128] f32; table fp16 [rows,2]; offsets_host [17] (16 levels).
int sdn_field_forward_f16(const float *xyzs, const float *dirs, const uint32_t *live_idx, const uint32_t *live_count, uint32_t M,
                          const void *weights, const float *bias0, const void *table, const int32_t *offsets_host, float S, uint32_t H,
                          float bound, float density_scale, int zero_deform, float *sigmas, float *rgbs, void *stream) {
    return sdn_int::field_forward_checked(0, {.xyzs = xyzs, .dirs = dirs, .live_idx = live_idx, .live_count = live_count, .M = M, .weights = weights,
                                              .bias0 = bias0, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                              .density_scale = density_scale, .zero_deform = zero_deform ? 1 : 0, .sigmas = sigmas, .rgbs = rgbs},
                                          stream);
}

}  // extern "C"
