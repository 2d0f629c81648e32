// Native training step of the dynamic field for gfx950 (MI355X): one C call = one optimizer step.
//
// Behavioural contract (what the step computes, in the reference's own order and dtypes):
//   dnerf/utils.py:38-125       train_step: render the ray batch, MSE against the ground truth (main_dnerf.py:103), mean
//   dnerf/renderer.py:260-331   run_cuda, training branch: near_far_from_aabb -> march_rays_train(perturb, mean_count budget) ->
//                               network -> density_scale -> composite_rays_train -> image + (1 - weights_sum) * bg
//   dnerf/network.py:123-169    freq(x,10) ++ freq(t,6) -> deformation MLP (8 x 128) -> x + deform (0 at t == 0) -> tiled grid ->
//                               sigma MLP (64) -> trunc_exp | SH(d,4) ++ geo -> colour MLP (64,64) -> sigmoid, all bias-free
//                               Linear layers under fp16 autocast (fp16 operands, fp32 accumulation, fp16 result per layer)
//   nerf/utils.py:880-906       GradScaler.scale(loss).backward(); scaler.step(optimizer); scaler.update(); ema.update()
//   main_dnerf.py:118           Adam(betas (0.9, 0.99), eps 1e-15) over network.py:260-275's groups (tables at lr, MLPs at lr_net)
//
// Why a native step: at 4096 rays / ~9000 samples the op-by-op step is ~160 launches of a few microseconds each (autograd glue:
// casts, fills, cats, the per-call weight packing, a 48 -> 24 MB table cast per step, three optimizer passes) -- launch-bound even
// when replayed as one HIP graph.  Here the step is ~35 launches: the existing operators' kernels (marching, fused MLP chains,
// grid encoder, compositing) composed directly, the glue between them fused into a handful of small kernels, every layer's
// weight gradient in one split-K launch, and ONE optimizer pass that also rewrites the fp16 copies the next step reads and clears
// the table's gradient accumulator.  Nothing is read back to the host.
//
// Everything below the MLP chains is per-sample streaming work (a few hundred bytes per sample): those kernels are launch- and
// latency-bound at this batch size, not bandwidth-bound; the optimizer pass over the 12 M-entry table is the one HBM-bound piece
// (30 B per entry: p, m, v read + written fp32, fp16 gradient read + cleared, fp16 copy written).
#include <math.h>
#include <stddef.h>

#include <type_traits>

#include "sdn_common.h"
#include "sdn_internal.h"
#include "sh_eval.h"

namespace {

using namespace sdn_sh;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// ---- the network's fixed geometry (dnerf/network.py:10-96 defaults; the mirror is dnerf_amd/network.py) ------------------------------
constexpr uint32_t kDefIn = 80, kDefCols = 76, kDefW = 128, kDefL = 7;   // 63 + 13 frequency features (padded to 80) -> 7 hidden layers -> 3
constexpr uint32_t kSigIn = 32, kSigW = 64, kSigOut = 16;               // 16 levels x 2 -> 64 -> 1 + 15
constexpr uint32_t kColIn = 32, kColCols = 31, kColW = 64, kColL = 2;    // SH 16 ++ geo 15 (padded to 32) -> 64 -> 64 -> 3
constexpr uint32_t kDefFlat = kDefW * kDefIn + (kDefL - 1) * kDefW * kDefW + 16 * kDefW;
constexpr uint32_t kColFlat = kColW * kColIn + (kColL - 1) * kColW * kColW + 16 * kColW;
constexpr uint32_t kLevels = 16;
constexpr uint32_t ACT_RELU = 0;
static_assert(kDefIn % 8 == 0, "kDefIn: whole 16-byte fp16 row pieces, whole 4-k-pair steps of the fp32 chains");
template <typename T> constexpr bool kHalf = std::is_same<T, _Float16>::value;   // the fp16 (-O) step's instance of a shared kernel

struct Hyper {          // written by the optimizer prologue, read by the update kernel
    float inv_scale;
    float step_size[2][2];   // [table | net][everything else | deformation MLP]
    float bc2_sqrt[2];
    float found_inf;
    int32_t skip;
    int32_t pad_[7];
};

// the fp32 step's packed weights (k_f32_pack): packed floats of one product: tiles x steps x 64.  Forward chain: first layer (in / 2
// steps), L - 1 hidden, last (1 tile); backward chain: last^T (8 steps), L - 1 hidden^T, first^T if dX
constexpr uint64_t pk_floats(uint32_t rows, uint32_t steps) { return (uint64_t)((rows + 31u) / 32u) * steps * 64u; }
constexpr uint64_t chain_fwd_floats(uint32_t in, uint32_t W, uint32_t L) { return pk_floats(W, in / 2) + (L - 1) * pk_floats(W, W / 2) + pk_floats(16, W / 2); }
constexpr uint64_t chain_bwd_floats(uint32_t in, uint32_t W, uint32_t L, bool dx) { return pk_floats(W, 8) + (L - 1) * pk_floats(W, W / 2) + (dx ? pk_floats(in, W / 2) : 0); }
constexpr uint64_t kPkDefF = 0, kPkDefB = kPkDefF + chain_fwd_floats(kDefIn, kDefW, kDefL);
constexpr uint64_t kPkSigF = kPkDefB + chain_bwd_floats(kDefIn, kDefW, kDefL, false);
constexpr uint64_t kPkSigB = kPkSigF + chain_fwd_floats(kSigIn, kSigW, 1);
constexpr uint64_t kPkColF = kPkSigB + chain_bwd_floats(kSigIn, kSigW, 1, true);
constexpr uint64_t kPkColB = kPkColF + chain_fwd_floats(kColIn, kColW, kColL);
constexpr uint64_t kPkTotal = kPkColB + chain_bwd_floats(kColIn, kColW, kColL, true);
// the fp32 step's split-K weight gradients: samples per chunk, floats per chunk's partial sums
constexpr uint32_t kDwChunk = 512;
constexpr uint32_t kDwTotal = kDefFlat + kSigW * kSigIn + kSigOut * kSigW + kColFlat;

// The workspace of either step (sdn_train_layout / _f32).  The fp32 step's rows and gradients have the fp16 step's shapes at 4-byte
// elements; only the fp16 step has parameter copies (w_*), ffmlp packings (pk_*_*) and enc_rm, only the fp32 step has `pk`.
struct Layout {
    uint64_t total;
    uint64_t w_table, w_deform, w_sigma0, w_sigma1, w_color, g_table, hyper;                 // persistent
    uint64_t pk_def_f, pk_def_b, pk_col_f, pk_col_b, pk;
    uint64_t nears, fars, noises, rays, pts, march;     // sample set 0 ...
    uint64_t set_stride;                                //  ... set 1 = + set_stride
    uint64_t dcol_out, dh0;
    uint64_t enc_in, def_hidden, def_out, xdef, grid_out, dy_dx, enc_rm, h1, hout, sigmas, col_in, col_hidden, col_out;
    uint64_t weights_sum, depth, image, sq_err;
    uint64_t col_bwd, dcol_in, dh, dh1, denc, dx, ddef, def_bwd;
    uint64_t g_deform, g_sigma0, g_sigma1, g_color, dw_partial;
};

void dw_job_list(const Layout &L, unsigned char *ws, uint32_t M, sdn_ffh::DwJob *jobs, uint32_t &n);

Layout make_layout(uint32_t N, uint32_t M, uint32_t max_steps, uint64_t table_entries, bool fp32) {
    Layout L{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) { const uint64_t o = at; at = (at + bytes + 255u) & ~(uint64_t)255u; return o; };
    const uint64_t m = M, n = N, e = fp32 ? 4 : 2;    // bytes per element of the network's rows and gradients
    if (!fp32) {
        L.w_table = take(table_entries * 2);  L.w_deform = take(kDefFlat * 2);  L.w_sigma0 = take(kSigW * kSigIn * 2);
        L.w_sigma1 = take(kSigOut * kSigW * 2);  L.w_color = take(kColFlat * 2);
    }
    L.g_table = take(table_entries * e);
    L.hyper = take(sizeof(Hyper));
    if (fp32) {
        L.pk = take(kPkTotal * 4);
    } else {
        L.pk_def_f = take((uint64_t)sdn_ffh::total_frags(kDefIn, kDefW, kDefL, 0, 1) * 1024);
        L.pk_def_b = take((uint64_t)sdn_ffh::total_frags(kDefIn, kDefW, kDefL, 1, 0) * 1024);
        L.pk_col_f = take((uint64_t)sdn_ffh::total_frags(kColIn, kColW, kColL, 0, 1) * 1024);
        L.pk_col_b = take((uint64_t)sdn_ffh::total_frags(kColIn, kColW, kColL, 1, 1) * 1024);
    }
    // two sets of sample buffers (phase 1 of the next batch runs beside phase 2 of this one)
    L.nears = take(n * 4);  L.fars = take(n * 4);  L.noises = take(n * 4);  L.rays = take(n * 12);
    L.pts = take(m * 32);                       // xyzs [M,3] | dirs [M,3] | deltas [M,2], zero-filled by every march
    L.march = take(sdn_march_rays_train_scratch_bytes(N, max_steps));
    L.set_stride = at - L.nears;
    at += L.set_stride;
    L.dcol_out = take(m * 16 * e);              // the gradient rows the compositing backward fills for the samples rays own:
    L.dh0 = take(m * e);                        // zero-filled by every step (dh0 must follow dcol_out: one fill)
    L.enc_in = take(m * kDefIn * e);  L.def_hidden = take(m * kDefL * kDefW * e);  L.def_out = take(m * 16 * e);
    L.xdef = take(m * 12);  L.grid_out = take(m * kLevels * 2 * e);  L.dy_dx = take(m * kLevels * 6 * e);
    if (!fp32) L.enc_rm = take(m * kSigIn * 2);
    L.h1 = take(m * kSigW * e);  L.hout = take(m * kSigOut * e);  L.sigmas = take(m * 4);
    L.col_in = take(m * kColIn * e);  L.col_hidden = take(m * kColL * kColW * e);  L.col_out = take(m * 16 * e);
    L.weights_sum = take(n * 4);  L.depth = take(n * 4);  L.image = take(n * 12);  L.sq_err = take(n * 4);
    L.col_bwd = take(m * kColL * kColW * e);  L.dcol_in = take(m * kColIn * e);
    L.dh = take(m * kSigOut * e);  L.dh1 = take(m * kSigW * e);  L.denc = take(m * kLevels * 2 * e);  L.dx = take(m * 3 * e);
    L.ddef = take(m * 16 * e);  L.def_bwd = take(m * kDefL * kDefW * e);
    L.g_deform = take(kDefFlat * e);  L.g_sigma0 = take(kSigW * kSigIn * e);  L.g_sigma1 = take(kSigOut * kSigW * e);  L.g_color = take(kColFlat * e);
    if (fp32) {
        L.dw_partial = take((uint64_t)sdn_div_up(M, kDwChunk) * kDwTotal * 4);
    } else {
        sdn_ffh::DwJob jobs[16];
        uint32_t nj = 0;
        dw_job_list(L, nullptr, M, jobs, nj);
        L.dw_partial = take(sdn_ffh::dw_jobs_bytes(jobs, nj, M));
    }
    L.total = at;
    return L;
}

// all 13 weight-gradient products of the step: deformation MLP (8), colour MLP (3), sigma MLP (2)
void dw_job_list(const Layout &L, unsigned char *ws, uint32_t M, sdn_ffh::DwJob *jobs, uint32_t &n) {
    auto H = [&](uint64_t off) { return (const _Float16 *)(ws + off); };
    auto G = [&](uint64_t off) { return (_Float16 *)(ws + off); };
    n = 0;
    const size_t mw = (size_t)M * kDefW, mc = (size_t)M * kColW;
    // deformation MLP (layout of the flat gradient: [128, 80] ++ 6 x [128, 128] ++ [16, 128]; ffmlp.cu:800-876 for the pairing)
    jobs[n++] = {H(L.ddef), 16, 16, H(L.def_hidden) + (kDefL - 1) * mw, kDefW, kDefW, G(L.g_deform) + kDefW * kDefIn + (kDefL - 1) * kDefW * kDefW};
    for (uint32_t j = kDefL - 1; j >= 1; j--)
        jobs[n++] = {H(L.def_bwd) + (kDefL - 1 - j) * mw, kDefW, kDefW, H(L.def_hidden) + (j - 1) * mw, kDefW, kDefW,
                     G(L.g_deform) + kDefW * kDefIn + (j - 1) * kDefW * kDefW};
    jobs[n++] = {H(L.def_bwd) + (kDefL - 1) * mw, kDefW, kDefW, H(L.enc_in), kDefIn, kDefIn, G(L.g_deform)};
    // colour MLP ([64, 32] ++ [64, 64] ++ [16, 64])
    jobs[n++] = {H(L.dcol_out), 16, 16, H(L.col_hidden) + (kColL - 1) * mc, kColW, kColW, G(L.g_color) + kColW * kColIn + (kColL - 1) * kColW * kColW};
    for (uint32_t j = kColL - 1; j >= 1; j--)
        jobs[n++] = {H(L.col_bwd) + (kColL - 1 - j) * mc, kColW, kColW, H(L.col_hidden) + (j - 1) * mc, kColW, kColW,
                     G(L.g_color) + kColW * kColIn + (j - 1) * kColW * kColW};
    jobs[n++] = {H(L.col_bwd) + (kColL - 1) * mc, kColW, kColW, H(L.col_in), kColIn, kColIn, G(L.g_color)};
    // sigma MLP: dW2 [16, 64] = dh^T h1, dW1 [64, 32] = dh1^T enc
    jobs[n++] = {H(L.dh), kSigOut, kSigOut, H(L.h1), kSigW, kSigW, G(L.g_sigma1)};
    jobs[n++] = {H(L.dh1), kSigW, kSigW, H(L.enc_rm), kSigIn, kSigIn, G(L.g_sigma0)};
}

// ---- small kernels --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float u01(uint64_t seed, uint32_t i) {   // splitmix64 -> 24 random bits -> [0, 1), like torch.rand's float grid
    return (float)(uint32_t)(sdn_splitmix64(seed, i) >> 40) * (1.0f / 16777216.0f);
}

__global__ void __launch_bounds__(256) k_train_rays(float *__restrict__ noises, const float *__restrict__ given, uint32_t N, uint64_t seed, int perturb,
                                                    int32_t *counter) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { counter[0] = 0; counter[1] = 0; }                              // renderer.py:296-298 counter.zero_()
    if (i < N) noises[i] = perturb ? (given ? given[i] : u01(seed, i)) : 0.0f;
}

// freq(x, 10) ++ freq(t, 6) as the input rows of the deformation MLP (freqencoder.cu:30-58's formula; in fp16 the autocast cast of
// F.linear's input).  One thread per (sample, 16th of a row).
template <typename T>
__global__ void __launch_bounds__(256) k_train_encode(const float *__restrict__ xyzs, uint32_t M, float time, T *__restrict__ enc, Hyper *hyper,
                                                      uint4 *__restrict__ zero_fill, uint32_t zero_n16) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (kHalf<T>) {   // the fp16 step only (the fp32 step has no found_inf and clears these rows with a fill)
        if (t == 0) hyper->found_inf = 0.0f;       // first kernel of a step's own phase: the non-finite flag of this step's gradients
        // the gradient rows the compositing backward fills only for the samples rays own (dcol_out .. dh0: 34 B per sample, i.e. at
        // most three 16-byte words per 16 threads of a sample) are cleared here instead of by a fill of their own
        if (t < zero_n16) zero_fill[t] = make_uint4(0u, 0u, 0u, 0u);
    }
    const uint32_t b = t >> 4, j = t & 15u;
    if (b >= M) return;
    T *row = enc + (size_t)b * kDefIn;
    const float half_pi = 3.141592653589793f / 2;
    if (j < 10) {
        #pragma unroll
        for (int d = 0; d < 3; d++) {
            const float a = scalbnf(xyzs[(size_t)b * 3 + d], (int)j);
            row[3 + 6 * j + d] = (T)sinf(a + 0.0f);
            row[6 + 6 * j + d] = (T)sinf(a + half_pi);
        }
    } else if (j == 10) {
        #pragma unroll
        for (int d = 0; d < 3; d++) row[d] = (T)xyzs[(size_t)b * 3 + d];
    } else if (j == 11) {
        row[63] = (T)time;
        #pragma unroll
        for (int f = 0; f < 6; f++) {
            const float a = scalbnf(time, f);
            row[64 + 2 * f] = (T)sinf(a + 0.0f);
            row[65 + 2 * f] = (T)sinf(a + half_pi);
        }
    } else if (j == 12) {
        row[76] = 0; row[77] = 0; row[78] = 0; row[79] = 0;
    }
}

// x + deform (network.py:140-145, deform = 0 on the canonical frame), normalised as GridEncoder.forward does (grid.py:146)
template <typename T>
__global__ void __launch_bounds__(256) k_train_xdef(const float *__restrict__ xyzs, const T *__restrict__ def_out, uint32_t M, int zero_deform,
                                                    float bound, float *__restrict__ xdef) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * 3) return;
    const uint32_t b = t / 3, d = t - b * 3;
    const float v = xyzs[t] + (zero_deform ? 0.0f : (float)def_out[(size_t)b * 16 + d]);
    xdef[t] = (v + bound) / (2 * bound);
}

// ---- the sigma MLP on the matrix cores ------------------------------------------------------------------------------------------------
// 32 -> 64 -> 16, 3 072 MACs per sample: one wave = 32 samples = N of v_mfma_f32_32x32x16_f16, weights are the A operand (M = output
// features), 4 + 4 MFMAs forward, 2 + 4 backward.  As in the fused MLP kernels (ffmlp_kernels.h) a layer's accumulator (feature
// rows 8(i>>2) + 4h + (i&3) of tile Mt in registers, the sample on the lane) converts in place into the next layer's B fragments,
// and rows leave / enter as 16-byte pieces through the half-wave exchange.  (A first version ran one LANE per sample on v_dot2 with
// the weights broadcast from LDS: 22 us forward / 13 us backward at 9 000 samples -- a chain of 1 536 dependent dot products per
// lane at one wave per CU.)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x16 mfma16(h8 a, h8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void half_wave_exchange(uint32_t &a, uint32_t &b) {      // lanes 32-63 of a <-> lanes 0-31 of b (whole wave active)
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}
// this lane's 4-feature runs of two neighbouring 8-feature groups <-> the 16 contiguous bytes of the row it stores / loaded
__device__ __forceinline__ uint4 runs_to_row16(h4 g0, h4 g1) {
    uint2 a = __builtin_bit_cast(uint2, g0), b = __builtin_bit_cast(uint2, g1);
    half_wave_exchange(a.x, b.x);
    half_wave_exchange(a.y, b.y);
    return uint4{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void row16_to_runs(uint4 v, h4 &g0, h4 &g1) {
    uint2 a{v.x, v.y}, b{v.z, v.w};
    half_wave_exchange(a.x, b.x);
    half_wave_exchange(a.y, b.y);
    g0 = __builtin_bit_cast(h4, a);
    g1 = __builtin_bit_cast(h4, b);
}
__device__ __forceinline__ h8 join(h4 a, h4 b) { return h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }
// A fragment of a row-major weight matrix W[rows, ld]: lane (m, h) holds W[m][16 s + 8 (j >> 2) + 4 h + (j & 3)], rows >= n_rows are zero
__device__ __forceinline__ h8 a_frag(const _Float16 *w, uint32_t ld, uint32_t n_rows, uint32_t m, uint32_t s, uint32_t h) {
    if (m >= n_rows) return h8{0, 0, 0, 0, 0, 0, 0, 0};
    const _Float16 *p = w + (size_t)m * ld + 16 * s + 4 * h;
    return join(*reinterpret_cast<const h4 *>(p), *reinterpret_cast<const h4 *>(p + 8));
}
// A fragment of the TRANSPOSE: lane (m, h) holds W[16 s + 8 (j >> 2) + 4 h + (j & 3)][m]
__device__ __forceinline__ h8 a_frag_t(const _Float16 *w, uint32_t ld, uint32_t m, uint32_t s, uint32_t h) {
    h8 v;
    #pragma unroll
    for (int j = 0; j < 8; j++) v[j] = w[(size_t)(16 * s + 8 * (j >> 2) + 4 * h + (j & 3)) * ld + m];
    return v;
}

// forward: grid features -> sigma MLP -> trunc_exp (activation.py:5-17) x density_scale; SH(d, 4); the colour MLP's input row
// [SH 16 | sigma-MLP output 16] (the log-density column meets a zero weight column: `w_color` is kept in that order)
struct SigmaFwd {
    const _Float16 *grid_out;   // [16][M][2]
    const _Float16 *w1, *w2;    // [64,32], [16,64]
    const float *dirs;          // [M,3]
    _Float16 *enc_rm, *h1, *hout, *col_in;
    float *sigmas;
    uint32_t M;
    float density_scale;
};

__global__ void __launch_bounds__(64) k_train_sigma_fwd(SigmaFwd P) {
    const uint32_t lane = threadIdx.x, n = lane & 31u, h = lane >> 5;
    const uint32_t b_raw = blockIdx.x * 32 + n;
    const bool live = b_raw < P.M;
    const uint32_t b = live ? b_raw : P.M - 1;
    h8 B1[2];
    #pragma unroll
    for (uint32_t s = 0; s < 2; s++) {
        h2 e[4];
        #pragma unroll
        for (uint32_t u = 0; u < 2; u++)
            #pragma unroll
            for (uint32_t v = 0; v < 2; v++) e[2 * u + v] = reinterpret_cast<const h2 *>(P.grid_out)[(size_t)(8 * s + 4 * u + 2 * h + v) * P.M + b];
        B1[s] = h8{e[0][0], e[0][1], e[1][0], e[1][1], e[2][0], e[2][1], e[3][0], e[3][1]};
        const uint4 row16 = runs_to_row16(h4{e[0][0], e[0][1], e[1][0], e[1][1]}, h4{e[2][0], e[2][1], e[3][0], e[3][1]});
        if (live) *reinterpret_cast<uint4 *>(P.enc_rm + (size_t)b * kSigIn + 16 * s + 8 * h) = row16;
    }
    h8 B2[4];
    #pragma unroll
    for (uint32_t Mt = 0; Mt < 2; Mt++) {
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        #pragma unroll
        for (uint32_t s = 0; s < 2; s++) acc = mfma16(a_frag(P.w1, kSigIn, kSigW, 32 * Mt + n, s, h), B1[s], acc);
        _Float16 v[16];
        #pragma unroll
        for (int i = 0; i < 16; i++) { const _Float16 x = (_Float16)acc[i]; v[i] = x > (_Float16)0 ? x : x * (_Float16)0; }   // x * (x > 0): keeps NaN (ffmlp_kernels.h relu16)
        #pragma unroll
        for (uint32_t p = 0; p < 2; p++) {
            const h4 g0{v[8 * p], v[8 * p + 1], v[8 * p + 2], v[8 * p + 3]}, g1{v[8 * p + 4], v[8 * p + 5], v[8 * p + 6], v[8 * p + 7]};
            B2[2 * Mt + p] = join(g0, g1);
            const uint4 row16 = runs_to_row16(g0, g1);
            if (live) *reinterpret_cast<uint4 *>(P.h1 + (size_t)b * kSigW + 32 * Mt + 16 * p + 8 * h) = row16;
        }
    }
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) acc = mfma16(a_frag(P.w2, kSigW, kSigOut, n, s, h), B2[s], acc);
    // rows 0..15 of the output tile: this lane holds o[4h .. 4h+3] (i = 0..3) and o[8+4h .. 8+4h+3] (i = 4..7)
    const h4 o0{(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]}, o1{(_Float16)acc[4], (_Float16)acc[5], (_Float16)acc[6], (_Float16)acc[7]};
    const uint4 orow = runs_to_row16(o0, o1);
    float sh[16], u0[1], u1[1], u2[1];
    sh_eval<4, false>(P.dirs[(size_t)b * 3], P.dirs[(size_t)b * 3 + 1], P.dirs[(size_t)b * 3 + 2], sh, u0, u1, u2);
    if (live) {
        *reinterpret_cast<uint4 *>(P.hout + (size_t)b * kSigOut + 8 * h) = orow;
        *reinterpret_cast<uint4 *>(P.col_in + (size_t)b * kColIn + 16 + 8 * h) = orow;
        h8 shh;
        #pragma unroll
        for (int j = 0; j < 8; j++) shh[j] = (_Float16)(h ? sh[8 + j] : sh[j]);
        *reinterpret_cast<h8 *>(P.col_in + (size_t)b * kColIn + 8 * h) = shh;
        if (h == 0) P.sigmas[b] = P.density_scale * expf((float)o0[0]);
    }
}

__device__ __forceinline__ _Float16 sigmoid16(_Float16 c) { return (_Float16)(1.0f / (1.0f + expf(-(float)c))); }

// ---- compositing, one WAVE per ray ------------------------------------------------------------------------------------------------
// composite_rays_train (raymarching.cu:501-577 forward, :602-682 backward) walks a ray's samples one after the other; with one lane per
// ray a batch of 4096 rays is 64 waves whose time is the longest ray's chain of dependent loads and double-precision exps (24 + 30 us
// for ~9000 samples).  Here lane i of a wave takes sample i of the ray: alpha in parallel, transmittance as a prefix PRODUCT across
// the lanes, the ray's sums as wave reductions.  The early stop `T < T_thresh` of the sequential loop becomes a per-sample predicate
// (sample i is composited iff the transmittance in front of it is >= T_thresh: T never grows).  The sums are tree sums, so results
// differ from the sequential operator's in the last bits (the public composite_rays_train op keeps the sequential order and the
// bit-exact contract).  Folded in: the fp16 sigmoid of the colour MLP's output (network.py:166) in front, the background mix and
// the MSE gradient per ray behind (renderer.py:318, utils.py:85), and in the backward kernel the gradients through sigmoid,
// density_scale and trunc_exp (activation.py:12-17) down to the fp16 rows the MLP backward chains start from.
__device__ __forceinline__ float wave_excl_product(float v, uint32_t lane) {   // exclusive prefix product over the 64 lanes
    float inc = v;
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float u = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc *= u; }
    const float up = __shfl_up(inc, 1);
    return lane == 0 ? 1.0f : up;
}
__device__ __forceinline__ float wave_incl_sum(float v, uint32_t lane) {
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float u = __shfl_up(v, o); if (lane >= (uint32_t)o) v += u; }
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one chunk of <= 64 samples of a ray: everything the forward AND the backward need about sample `i`
struct SampleTerms { bool on; float alpha, T, weight, delta0, t, c[3]; };

// The precision the compositing kernels run in.  Fp16Net: the -O step -- fp16 colour MLP output (the fp16 sigmoid), fp16 gradient
// rows, the loss scaled by the GradScaler's factor.  Fp32Net: everything fp32, the loss unscaled (the disabled scaler).
struct Fp16Net {
    typedef _Float16 T;
    static __device__ __forceinline__ float colour(_Float16 c) { return (float)sigmoid16(c); }
    static __device__ __forceinline__ float loss_scale(const float *s) { return *s; }
    // the first 16 bytes of sample s's colour-gradient row, from the gradient gi of its ray's image
    static __device__ __forceinline__ void store_dcol(_Float16 *row, const float (&gi)[3], const SampleTerms &s) {
        _Float16 dc[3];
        #pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const _Float16 g16 = (_Float16)(gi[ch] * s.weight);                          // composite's float32 cast, backwards
            dc[ch] = (_Float16)(((float)g16 * (1.0f - s.c[ch])) * s.c[ch]);              // sigmoid backward on fp16 (a * (1 - y) * y in float)
        }
        *reinterpret_cast<h8 *>(row) = h8{dc[0], dc[1], dc[2], 0, 0, 0, 0, 0};
    }
};
struct Fp32Net {
    typedef float T;
    static __device__ __forceinline__ float colour(float c) { return 1.0f / (1.0f + expf(-c)); }
    static __device__ __forceinline__ float loss_scale(const float *) { return 1.0f; }
    static __device__ __forceinline__ void store_dcol(float *row, const float (&gi)[3], const SampleTerms &s) {
        float dc[3];
        #pragma unroll
        for (int ch = 0; ch < 3; ch++) dc[ch] = ((gi[ch] * s.weight) * (1.0f - s.c[ch])) * s.c[ch];
        *reinterpret_cast<float4 *>(row) = float4{dc[0], dc[1], dc[2], 0.0f};
    }
};

template <class Net> struct CompositeArgs {
    typedef typename Net::T T;
    const float *sigmas, *deltas;        // [M] (density_scale applied), [M,2]
    const T *col_out, *hout;             // [M,16] colour MLP output (pre-sigmoid), [M,16] sigma MLP output (column 0: log density)
    const int32_t *rays;                 // [N,3]
    const float *bg, *gt, *loss_scale;   // (loss_scale: the fp16 step's only)
    float *weights_sum, *depth, *image, *image_out, *sq_err;   // per ray; sq_err [N]: sum over channels of (pred - gt)^2
    T *dcol_out, *dh0;                   // backward: [M,16], [M]
    uint32_t M, N;
    float T_thresh, bg_value, density_scale;
    // optional error-map update (utils.py:91-113): the map row of this step's frame, every ray's cell in it, every ray's loss
    float *error_row;
    const int32_t *inds_coarse;
    float *ray_loss_out;
};

template <class Net>
__device__ __forceinline__ SampleTerms sample_terms(const CompositeArgs<Net> &P, uint32_t idx, bool in_ray, float T_carry, float t_carry, uint32_t lane,
                                                    float &T_next, float &t_next) {
    SampleTerms s{};
    float one_minus = 1.0f, d1 = 0.0f;
    if (in_ray) {
        s.delta0 = P.deltas[(size_t)idx * 2];
        d1 = P.deltas[(size_t)idx * 2 + 1];
        s.alpha = 1.0f - sdn_exp_cr(-P.sigmas[idx] * s.delta0);
        one_minus = 1.0f - s.alpha;
        #pragma unroll
        for (int ch = 0; ch < 3; ch++) s.c[ch] = Net::colour(P.col_out[(size_t)idx * 16 + ch]);
    }
    s.T = T_carry * wave_excl_product(one_minus, lane);
    s.t = t_carry + wave_incl_sum(d1, lane);
    s.on = in_ray && s.T >= P.T_thresh;
    s.weight = s.on ? s.alpha * s.T : 0.0f;
    T_next = __shfl(s.T * one_minus, 63);
    t_next = __shfl(s.t, 63);
    return s;
}

template <class Net>
__global__ void __launch_bounds__(256) k_train_composite_fwd(CompositeArgs<Net> P) {
    const uint32_t lane = threadIdx.x & 63u, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= P.N) return;
    const uint32_t index = (uint32_t)P.rays[n * 3], offset = (uint32_t)P.rays[n * 3 + 1], count = (uint32_t)P.rays[n * 3 + 2];
    float ws = 0, d = 0, r = 0, g = 0, b = 0;
    if (count != 0 && offset + count <= P.M) {
        float T_carry = 1.0f, t_carry = 0.0f;
        for (uint32_t c0 = 0; c0 < count && T_carry >= P.T_thresh; c0 += 64) {
            float T_next, t_next;
            const SampleTerms s = sample_terms(P, offset + c0 + lane, c0 + lane < count, T_carry, t_carry, lane, T_next, t_next);
            ws += s.weight; d += s.weight * s.t;
            r += s.weight * s.c[0]; g += s.weight * s.c[1]; b += s.weight * s.c[2];
            T_carry = T_next; t_carry = t_next;
        }
        ws = wave_sum(ws); d = wave_sum(d); r = wave_sum(r); g = wave_sum(g); b = wave_sum(b);
    }
    if (lane == 0) {
        P.weights_sum[index] = ws; P.depth[index] = d;
        const float img[3] = {r, g, b};
        float sq = 0.0f;
        #pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            P.image[(size_t)index * 3 + ch] = img[ch];
            const float bgc = P.bg ? P.bg[(size_t)index * 3 + ch] : P.bg_value;
            const float pred = img[ch] + (1.0f - ws) * bgc;          // renderer.py:318
            const float e = pred - P.gt[(size_t)index * 3 + ch];
            sq += e * e;
            if (P.image_out) P.image_out[(size_t)index * 3 + ch] = pred;
        }
        P.sq_err[index] = sq;
        if (P.error_row) {
            // utils.py:85, :109-110, for every ray of the batch (one without samples predicts the background).  No two rays share a
            // cell (the draw is without replacement), so the read-modify-write needs no atomic.
            const float l = sq / 3.0f;
            const int32_t c = P.inds_coarse[index];
            P.error_row[c] = 0.1f * P.error_row[c] + 0.9f * l;
            if (P.ray_loss_out) P.ray_loss_out[index] = l;
        }
    }
}

// loss = mean over rays of the mean over channels of (pred - gt)^2 (utils.py:85, :125): a deterministic tree sum in ONE workgroup
// (folding it into the last block of the compositing launch, or the optimizer prologue into the last block of the non-finite check,
// was measured and reverted: the agent-scope release every block then needs before its ticket costs ~1.7 us per block, 5 -> 26 us
// and 12 -> 19 us for the two launches)
__global__ void __launch_bounds__(1024) k_train_loss(const float *__restrict__ sq_err, uint32_t N, float *__restrict__ loss_out) {
    __shared__ float s_part[16];
    float acc = 0.0f;
    for (uint32_t r = threadIdx.x; r < N; r += 1024) acc += sq_err[r] / 3.0f;
    acc = wave_sum(acc);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < 16; w++) t += s_part[w];
        *loss_out = t / (float)N;
    }
}

template <class Net>
__global__ void __launch_bounds__(256) k_train_composite_bwd(CompositeArgs<Net> P) {
    const uint32_t lane = threadIdx.x & 63u, n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= P.N) return;
    const uint32_t index = (uint32_t)P.rays[n * 3], offset = (uint32_t)P.rays[n * 3 + 1], count = (uint32_t)P.rays[n * 3 + 2];
    if (count == 0 || offset + count > P.M) return;
    // gradient of scale * loss with respect to this ray's image and weights_sum (MSE mean over 3 N values; the background mix)
    const float ws_final = P.weights_sum[index];
    const float cg = (Net::loss_scale(P.loss_scale) / (float)P.N) / 3.0f;
    float gi[3], fin[3], gws = 0.0f;
    #pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        fin[ch] = P.image[(size_t)index * 3 + ch];
        const float bgc = P.bg ? P.bg[(size_t)index * 3 + ch] : P.bg_value;
        const float pred = fin[ch] + (1.0f - ws_final) * bgc;
        gi[ch] = ((pred - P.gt[(size_t)index * 3 + ch]) * 2.0f) * cg;
        gws -= gi[ch] * bgc;
    }
    float T_carry = 1.0f, t_carry = 0.0f, acc_c[3] = {0, 0, 0};
    for (uint32_t c0 = 0; c0 < count && T_carry >= P.T_thresh; c0 += 64) {
        float T_next, t_next;
        const uint32_t idx = offset + c0 + lane;
        const SampleTerms s = sample_terms(P, idx, c0 + lane < count, T_carry, t_carry, lane, T_next, t_next);
        // raymarching.cu:655-675: r, g, b are the running sums INCLUDING this sample, T the transmittance BEHIND it
        float run[3];
        #pragma unroll
        for (int ch = 0; ch < 3; ch++) run[ch] = acc_c[ch] + wave_incl_sum(s.weight * s.c[ch], lane);
        if (s.on) {
            const float T_after = s.T * (1.0f - s.alpha);
            const float g_sigma = s.delta0 * (gi[0] * (T_after * s.c[0] - (fin[0] - run[0])) + gi[1] * (T_after * s.c[1] - (fin[1] - run[1])) +
                                              gi[2] * (T_after * s.c[2] - (fin[2] - run[2])) + gws * (1.0f - ws_final));
            Net::store_dcol(P.dcol_out + (size_t)idx * 16, gi, s);
            const float x = fminf(fmaxf((float)P.hout[(size_t)idx * kSigOut], -15.0f), 15.0f);
            P.dh0[idx] = (typename Net::T)((g_sigma * P.density_scale) * expf(x));      // density_scale, trunc_exp backward (fp16: the cast)
        }
        #pragma unroll
        for (int ch = 0; ch < 3; ch++) acc_c[ch] = __shfl(run[ch], 63);
        T_carry = T_next; t_carry = t_next;
    }
}

// sigma MLP backward: dh = [trunc_exp gradient | colour MLP's gradient of columns 17..31 of its input], dh1 = (W2^T dh) * relu',
// denc = W1^T dh1 in the grid encoder's [level][sample][2] layout; dh and dh1 also row-major for the weight-gradient products.
struct SigmaBwd {
    const _Float16 *dh0, *dcol_in, *h1, *w1, *w2;
    _Float16 *dh, *dh1, *denc;
    uint32_t M;
};

__global__ void __launch_bounds__(64) k_train_sigma_bwd(SigmaBwd P) {
    const uint32_t lane = threadIdx.x, n = lane & 31u, h = lane >> 5;
    const uint32_t b_raw = blockIdx.x * 32 + n;
    const bool live = b_raw < P.M;
    const uint32_t b = live ? b_raw : P.M - 1;
    // columns 16..31 of the colour MLP's input gradient are d(sigma-MLP output); column 16 (log density: zero weights there) is
    // replaced by the compositing's gradient through trunc_exp
    uint4 raw = *reinterpret_cast<const uint4 *>(P.dcol_in + (size_t)b * kColIn + 16 + 8 * h);
    if (h == 0) raw.x = (raw.x & 0xFFFF0000u) | (uint32_t)__builtin_bit_cast(unsigned short, P.dh0[b]);
    if (live) *reinterpret_cast<uint4 *>(P.dh + (size_t)b * kSigOut + 8 * h) = raw;
    h4 d0, d1;
    row16_to_runs(raw, d0, d1);
    const h8 Bd = join(d0, d1);
    h8 B2[4];
    #pragma unroll
    for (uint32_t Mt = 0; Mt < 2; Mt++) {
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        acc = mfma16(a_frag_t(P.w2, kSigW, 32 * Mt + n, 0, h), Bd, acc);
        #pragma unroll
        for (uint32_t p = 0; p < 2; p++) {
            h4 f0, f1;
            row16_to_runs(*reinterpret_cast<const uint4 *>(P.h1 + (size_t)b * kSigW + 32 * Mt + 16 * p + 8 * h), f0, f1);
            h4 g0, g1;
            #pragma unroll
            for (int e = 0; e < 4; e++) {
                const _Float16 a0 = (_Float16)acc[8 * p + e], a1 = (_Float16)acc[8 * p + 4 + e];      // g * (f > 0): a non-finite g stays visible
                g0[e] = f0[e] > (_Float16)0 ? a0 : a0 * (_Float16)0;
                g1[e] = f1[e] > (_Float16)0 ? a1 : a1 * (_Float16)0;
            }
            B2[2 * Mt + p] = join(g0, g1);
            const uint4 row16 = runs_to_row16(g0, g1);
            if (live) *reinterpret_cast<uint4 *>(P.dh1 + (size_t)b * kSigW + 32 * Mt + 16 * p + 8 * h) = row16;
        }
    }
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) acc = mfma16(a_frag_t(P.w1, kSigIn, n, s, h), B2[s], acc);
    // row m = 8 q + 4 h + (i & 3) of the tile is grid feature m = 2 level + channel
    if (live) {
        #pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            reinterpret_cast<h2 *>(P.denc)[(size_t)(4 * q + 2 * h) * P.M + b] = h2{(_Float16)acc[4 * q], (_Float16)acc[4 * q + 1]};
            reinterpret_cast<h2 *>(P.denc)[(size_t)(4 * q + 2 * h + 1) * P.M + b] = h2{(_Float16)acc[4 * q + 2], (_Float16)acc[4 * q + 3]};
        }
    }
}

// gradient of the deformation MLP's output: grid input gradient, / (2 bound) of the normalisation (in fp16 the cast of
// `deform.to(x.dtype)`); zero columns 3..15 of the operator's 16-wide output
template <typename T>
__global__ void __launch_bounds__(256) k_train_deform_grad(const T *__restrict__ dx, uint32_t M, float bound, T *__restrict__ ddef) {
    typedef T piece __attribute__((ext_vector_type(16 / sizeof(T))));   // 16 bytes of a row: a row of 16 is sizeof(T) pieces
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= M) return;
    T d[3];
    #pragma unroll
    for (int c = 0; c < 3; c++) d[c] = (T)((float)dx[(size_t)b * 3 + c] / (2 * bound));
    piece *row = reinterpret_cast<piece *>(ddef + (size_t)b * 16);
    row[0] = piece{d[0], d[1], d[2]};
    #pragma unroll
    for (uint32_t k = 1; k < sizeof(T); k++) row[k] = piece{};
}

// ---- optimizer ------------------------------------------------------------------------------------------------------------------
struct CheckArgs { const _Float16 *g[5]; uint32_t n8[5]; uint32_t count; Hyper *hyper; uint32_t col_seg; };

struct Prologue {
    Hyper *hyper;
    float *steps, *scale;
    int32_t *tracker;
    double beta1, beta2, lr_table, lr_net;
    float growth, backoff;
    uint32_t interval;
    int deform_active;
    float divisor;
};

// GradScaler's non-finite check over every gradient of the step (amp's _amp_foreach_non_finite_check_and_unscale_)
__global__ void __launch_bounds__(256) k_train_check(CheckArgs A) {
    bool bad = false;
    for (uint32_t s = 0; s < A.count; s++) {
        const uint4 *p = reinterpret_cast<const uint4 *>(A.g[s]);
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n8[s]; i += gridDim.x * blockDim.x) {
            const uint4 v = p[i];
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
            // input column 16 of the colour MLP's first layer is the log-density column: its weight is structurally zero and its
            // "gradient" (dcol_hidden^T . log-density) has no counterpart in the reference and never reaches Adam (the `split` of
            // build_segments skips it) -- an fp16 overflow there must not skip the step.  Row r, column 16 = half 0 of uint4 4 r + 2.
            if (s == A.col_seg && i < kColW * kColIn / 8 && (i & 3u) == 2u) w[0] &= 0xFFFF0000u;
            #pragma unroll
            for (int k = 0; k < 4; k++) bad |= ((w[k] & 0x7C00u) == 0x7C00u) | ((w[k] & 0x7C000000u) == 0x7C000000u);
        }
    }
    if (bad) A.hyper->found_inf = 1.0f;
}

// One thread: the skip decision, bias corrections in double as torch's Adam computes them on the host (adam.py _single_tensor_adam:
// 1 - beta ** step, lr / bias_correction1, bias_correction2 ** 0.5), and amp_update_scale (AmpKernels.cu) for the NEXT step.
// Without a scaler (the fp32 step: the disabled GradScaler) every step counts; found_inf, scale and tracker are not read.
template <bool SCALER>
__global__ void k_train_prologue(Prologue P) {
    Hyper *h = P.hyper;
    bool found = false;
    float scale = 1.0f;
    if constexpr (SCALER) {
        found = h->found_inf != 0.0f;
        scale = *P.scale;
        h->skip = found ? 1 : 0;
        h->inv_scale = (float)(1.0 / ((double)scale * (double)P.divisor));
    }
    if (!found) {
        P.steps[0] += 1.0f;
        if (P.deform_active) P.steps[1] += 1.0f;
    }
    for (int g = 0; g < 2; g++) {
        const double st = (double)P.steps[g] > 0 ? (double)P.steps[g] : 1.0;
        const double bc1 = 1.0 - pow(P.beta1, st), bc2 = 1.0 - pow(P.beta2, st);
        h->step_size[0][g] = (float)(P.lr_table / bc1);
        h->step_size[1][g] = (float)(P.lr_net / bc1);
        h->bc2_sqrt[g] = (float)sqrt(bc2);
    }
    if constexpr (!SCALER) return;
    if (found) {
        *P.scale = scale * P.backoff;
        *P.tracker = 0;
    } else {
        const int32_t ok = *P.tracker + 1;
        if (ok == (int32_t)P.interval) {
            const float grown = scale * P.growth;
            if (isfinite(grown)) *P.scale = grown;
            *P.tracker = 0;
        } else {
            *P.tracker = ok;
        }
    }
}

template <typename G> struct AdamSeg {
    float *p, *m, *v, *ema;
    G *g;               // gradient (fp16: scaled by the loss scale), element (r, c) at r * ld + c
    _Float16 *w16;      // fp16 copy, same layout (the fp16 step's only)
    uint32_t n, cols, ld, split;      // columns >= split sit one column further right (the colour MLP's input layer: [SH 16 | 0 | geo 15])
    uint32_t lr_idx, group, zero_grad, frozen, blk_begin;
};
template <typename G> struct AdamArgs {
    AdamSeg<G> seg[SDN_TRAIN_N_PARAMS];
    uint32_t nseg;
    const Hyper *hyper;
    float one_minus_b1, b2, one_minus_b2, eps, ema_keep;   // ema_keep = 1 - decay
};

// the gradient Adam sees: the fp16 step's unscaled the way GradScaler.unscale_ does (float(grad) * inv_scale), the fp32 step's as is
__device__ __forceinline__ float adam_grad(_Float16 g, float inv_scale) { return (float)g * inv_scale; }
__device__ __forceinline__ float adam_grad(float g, float) { return g; }

// torch.optim.Adam, single-tensor form (adam.py:_single_tensor_adam; amsgrad / weight_decay / maximize off):   m.lerp_(g, 1 - b1);
// v.mul_(b2).addcmul_(g, g, 1 - b2);  denom = sqrt(v) / bias_correction2_sqrt + eps;  p.addcdiv_(m, denom, -step_size).   The same
// pass clears the table's gradient accumulator and applies torch_ema's shadow -= (1 - decay) * (shadow - p).  In the fp16 step
// (G = _Float16) it also writes the fp16 copy the next step's kernels read (the autocast casts of the reference), and a step with a
// non-finite gradient changes nothing but the accumulator and the shadows; the fp32 step has no copies and no skip.
template <typename G>
__global__ void __launch_bounds__(256) k_train_adam(AdamArgs<G> A) {
    typedef G g4 __attribute__((ext_vector_type(4)));
    uint32_t s = 0;
    for (uint32_t k = 1; k < A.nseg; k++) s = blockIdx.x >= A.seg[k].blk_begin ? k : s;
    const AdamSeg<G> &S = A.seg[s];
    const Hyper &H = *A.hyper;
    const bool update = !(kHalf<G> && H.skip) && !S.frozen;
    const float inv_scale = H.inv_scale, step_size = H.step_size[S.lr_idx][S.group], bc2s = H.bc2_sqrt[S.group];
    // the table (12.2 M contiguous entries: the pass's HBM traffic) four entries per lane: 16-byte loads and stores
    const uint32_t first = (blockIdx.x - S.blk_begin) * 1024u;
    if (S.cols == S.ld && first + 1024u <= S.n && !S.ema && update) {
        const uint32_t i = first + 4u * threadIdx.x;
        float4 p = *reinterpret_cast<const float4 *>(S.p + i), m = *reinterpret_cast<const float4 *>(S.m + i), v = *reinterpret_cast<const float4 *>(S.v + i);
        const g4 gv = *reinterpret_cast<const g4 *>(S.g + i);
        float *pp = &p.x, *mm = &m.x, *vv = &v.x;
        h4 w;
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            const float g = adam_grad(gv[e], inv_scale);
            mm[e] = mm[e] + A.one_minus_b1 * (g - mm[e]);
            vv[e] = vv[e] * A.b2 + (A.one_minus_b2 * g) * g;
            const float denom = sqrtf(vv[e]) / bc2s + A.eps;
            pp[e] = pp[e] - step_size * (mm[e] / denom);
            w[e] = (_Float16)pp[e];
        }
        *reinterpret_cast<float4 *>(S.m + i) = m; *reinterpret_cast<float4 *>(S.v + i) = v; *reinterpret_cast<float4 *>(S.p + i) = p;
        if constexpr (kHalf<G>) *reinterpret_cast<h4 *>(S.w16 + i) = w;
        if (S.zero_grad) *reinterpret_cast<g4 *>(S.g + i) = g4{0, 0, 0, 0};
        return;
    }
    const uint32_t base = first + threadIdx.x;
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = base + 256u * k;
        if (i >= S.n) break;
        uint32_t j = i;
        if (S.cols != S.ld) { const uint32_t r = i / S.cols, c = i - r * S.cols; j = r * S.ld + c + (c >= S.split ? 1u : 0u); }
        float p = S.p[i];
        if (update) {
            const float g = adam_grad(S.g[j], inv_scale);
            float m = S.m[i], v = S.v[i];
            m = m + A.one_minus_b1 * (g - m);
            v = v * A.b2 + (A.one_minus_b2 * g) * g;
            const float denom = sqrtf(v) / bc2s + A.eps;
            p = p - step_size * (m / denom);
            S.m[i] = m; S.v[i] = v; S.p[i] = p;
            if constexpr (kHalf<G>) S.w16[j] = (_Float16)p;
        }
        if (S.zero_grad) S.g[j] = (G)0;
        if (S.ema) { const float e = S.ema[i]; S.ema[i] = e - (e - p) * A.ema_keep; }
    }
}

// fp16 copies from the fp32 masters (sdn_train_refresh)
__global__ void __launch_bounds__(256) k_train_copy16(AdamArgs<_Float16> A) {
    uint32_t s = 0;
    for (uint32_t k = 1; k < A.nseg; k++) s = blockIdx.x >= A.seg[k].blk_begin ? k : s;
    const AdamSeg<_Float16> &S = A.seg[s];
    const uint32_t base = (blockIdx.x - S.blk_begin) * 1024u + threadIdx.x;
    #pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = base + 256u * k;
        if (i >= S.n) break;
        uint32_t j = i;
        if (S.cols != S.ld) { const uint32_t r = i / S.cols, c = i - r * S.cols; j = r * S.ld + c + (c >= S.split ? 1u : 0u); }
        S.w16[j] = (_Float16)S.p[i];
    }
}

// parameter i of SDN_TRAIN_N_PARAMS -> its place in the gradients (and the fp16 step's copies)
template <typename G>
uint32_t build_segments(const SdnTrainStep *s, const Layout &L, AdamArgs<G> &A) {
    unsigned char *ws = (unsigned char *)s->workspace;
    struct Place { uint64_t w, g; uint32_t off, rows, cols, ld, lr, group; };
    Place pl[SDN_TRAIN_N_PARAMS];
    const uint32_t table_n = (uint32_t)s->grid_offsets[kLevels] * 2u;
    pl[0] = {L.w_table, L.g_table, 0, table_n / 2, 2, 2, 0, 0};
    pl[1] = {L.w_deform, L.g_deform, 0, kDefW, kDefCols, kDefIn, 1, 1};
    for (uint32_t i = 1; i < kDefL; i++) pl[1 + i] = {L.w_deform, L.g_deform, kDefW * kDefIn + (i - 1) * kDefW * kDefW, kDefW, kDefW, kDefW, 1, 1};
    pl[8] = {L.w_deform, L.g_deform, kDefW * kDefIn + (kDefL - 1) * kDefW * kDefW, 3, kDefW, kDefW, 1, 1};
    pl[9] = {L.w_sigma0, L.g_sigma0, 0, kSigW, kSigIn, kSigIn, 1, 0};
    pl[10] = {L.w_sigma1, L.g_sigma1, 0, kSigOut, kSigW, kSigW, 1, 0};
    pl[11] = {L.w_color, L.g_color, 0, kColW, kColCols, kColIn, 1, 0};
    pl[12] = {L.w_color, L.g_color, kColW * kColIn, kColW, kColW, kColW, 1, 0};
    pl[13] = {L.w_color, L.g_color, kColW * kColIn + kColW * kColW, 3, kColW, kColW, 1, 0};
    uint32_t blk = 0;
    for (int i = 0; i < SDN_TRAIN_N_PARAMS; i++) {
        const SdnTrainParam &q = s->params[i];
        AdamSeg<G> &S = A.seg[i];
        S.p = q.param; S.m = q.exp_avg; S.v = q.exp_avg_sq; S.ema = q.ema;
        S.g = (G *)(ws + pl[i].g) + pl[i].off; S.w16 = kHalf<G> ? (_Float16 *)(ws + pl[i].w) + pl[i].off : nullptr;
        S.n = pl[i].rows * pl[i].cols; S.cols = pl[i].cols; S.ld = pl[i].ld; S.split = i == 11 ? 16u : 0xFFFFFFFFu;
        S.lr_idx = pl[i].lr; S.group = pl[i].group; S.zero_grad = i == 0; S.frozen = 0; S.blk_begin = blk;
        blk += sdn_div_up(S.n, 1024u);
    }
    A.nseg = SDN_TRAIN_N_PARAMS;
    return blk;
}

// Adam over the segments [i0, i1) of a full segment list (workgroup ranges re-based)
void launch_adam(const AdamArgs<_Float16> &all, uint32_t i0, uint32_t i1, hipStream_t st) {
    AdamArgs<_Float16> A = all;
    uint32_t blk = 0;
    for (uint32_t i = i0; i < i1; i++) {
        A.seg[i - i0] = all.seg[i];
        A.seg[i - i0].blk_begin = blk;
        blk += sdn_div_up(all.seg[i].n, 1024u);
    }
    A.nseg = i1 - i0;
    hipLaunchKernelGGL(k_train_adam<_Float16>, dim3(blk), dim3(256), 0, st, A);
}

// the optimizer pass of a step: its segments, the frozen deformation MLP, Adam's and the EMA's constants
template <typename G>
uint32_t adam_args(const SdnTrainStep *s, const Layout &L, Hyper *hyper, bool freeze_deform, AdamArgs<G> &A) {
    const uint32_t blocks = build_segments(s, L, A);
    if (freeze_deform) for (uint32_t i = 1; i <= kDefL + 1; i++) A.seg[i].frozen = 1;
    A.hyper = hyper;
    A.one_minus_b1 = (float)(1.0 - s->beta1); A.b2 = (float)s->beta2; A.one_minus_b2 = (float)(1.0 - s->beta2); A.eps = (float)s->eps;
    A.ema_keep = 1.0f - s->ema_decay;
    return blocks;
}

int table_wait(const SdnTrainStep *s, hipStream_t st) {
    if (s->table_stream && s->table_done && hipStreamWaitEvent(st, (hipEvent_t)s->table_done, 0) != hipSuccess) return sdn_launch_status();
    return 0;
}

bool workspace_ok(const SdnTrainStep *s) { return s && s->workspace && !((uintptr_t)s->workspace & 255u); }

// the record checks of sdn_train_step_f16 / _f32.  The fp32 step has no optimizer-only mode and no overlapped table pass (data
// parallelism), and no scaler: loss_scale and growth_tracker are not read.
bool step_ok(const SdnTrainStep *s, bool fp32) {
    if (!workspace_ok(s)) return false;
    if (s->mode < 0 || s->mode > (fp32 ? 1 : 2)) return false;
    if (fp32 ? (s->table_stream || s->table_ready || s->table_done)
             : (s->table_stream != nullptr) != (s->table_ready != nullptr) || (s->table_stream != nullptr) != (s->table_done != nullptr)) return false;
    if (s->phase < 0 || s->phase > 2 || (s->mode == 2 && s->phase != 0)) return false;
    if (s->mode != 2 && s->phase != 2 && (!s->rays_o || !s->rays_d || !s->bitfield || !s->aabb || !s->counter)) return false;
    if (s->mode != 2 && s->phase != 1 && (!s->target || !s->loss_out)) return false;
    if (s->mode != 2 && s->phase != 1 && s->error_row && !s->inds_coarse) return false;
    if (s->N == 0 || s->M == 0 || s->max_steps == 0 || s->bound <= 0 || (fp32 && s->grid_offsets[kLevels] <= 0)) return false;
    for (int i = 0; i < SDN_TRAIN_N_PARAMS; i++) if (!s->params[i].param) return false;
    if (s->mode != 1) {
        if (!s->adam_steps || (!fp32 && (!s->loss_scale || !s->growth_tracker))) return false;
        // (a frozen deformation MLP -- SealD-NeRF's edit training -- has no optimizer state: its Adam segments are never touched)
        for (int i = 0; i < SDN_TRAIN_N_PARAMS; i++) {
            const bool frozen = s->deform_frozen && i >= 1 && i <= (int)kDefL + 1;
            if (!frozen && (!s->params[i].exp_avg || !s->params[i].exp_avg_sq)) return false;
        }
    } else if (!fp32 && !s->loss_scale) {
        return false;
    }
    const uint64_t expect[SDN_TRAIN_N_PARAMS] = {(uint64_t)s->grid_offsets[kLevels] * 2, kDefW * kDefCols, kDefW * kDefW, kDefW * kDefW, kDefW * kDefW, kDefW * kDefW,
                                                 kDefW * kDefW, kDefW * kDefW, 3 * kDefW, kSigW * kSigIn, kSigOut * kSigW, kColW * kColCols, kColW * kColW, 3 * kColW};
    for (int i = 0; i < SDN_TRAIN_N_PARAMS; i++) if (s->params[i].n != expect[i]) return false;
    return true;
}


#define SDN_TRY(x) do { rc = (x); if (rc) return rc; } while (0)

Layout step_layout(const SdnTrainStep *s, bool fp32) { return make_layout(s->N, s->M, s->max_steps, (uint64_t)s->grid_offsets[kLevels] * 2, fp32); }

// phase 0 / 1 of either step: rays -> samples of the sample set at `set_off` (renderer.py:283-304; nothing of it has a dtype)
int march_samples(const SdnTrainStep *s, const Layout &L, uint64_t set_off, hipStream_t st) {
    const uint32_t N = s->N, M = s->M;
    unsigned char *ws = (unsigned char *)s->workspace;
    auto F = [&](uint64_t off) { return (float *)(ws + off); };
    float *xyzs = F(L.pts + set_off), *dirs = xyzs + (size_t)M * 3, *deltas = xyzs + (size_t)M * 6;
    int rc;
    hipLaunchKernelGGL(k_train_rays, dim3(sdn_div_up(N, 256u)), dim3(256), 0, st, F(L.noises + set_off), s->noises, N, s->noise_seed, s->perturb, s->counter);
    SDN_TRY(sdn_near_far_from_aabb(s->rays_o, s->rays_d, s->aabb, N, s->min_near, F(L.nears + set_off), F(L.fars + set_off), st));
    if (hipMemsetAsync(ws + L.pts + set_off, 0, (uint64_t)M * 32, st) != hipSuccess) return sdn_launch_status();
    return sdn_int::march_rays_train(s->rays_o, s->rays_d, s->bitfield, s->bound, s->dt_gamma, s->max_steps, N, s->cascade, s->grid_size, M,
                                     F(L.nears + set_off), F(L.fars + set_off), xyzs, dirs, deltas, (int32_t *)(ws + L.rays + set_off), s->counter,
                                     F(L.noises + set_off), ws + L.march + set_off, s->cull_grid, st);
}

// sdn_train_layout / _f32 (the fp32 step has no parameter copies: its w_* are 0)
int fill_layout(uint32_t N, uint32_t M, uint32_t max_steps, const int32_t *grid_offsets, SdnTrainLayout *out, bool fp32) {
    if (!grid_offsets || !out || N == 0 || M == 0 || max_steps == 0 || grid_offsets[kLevels] <= 0) return SDN_E_BADARG;
    const Layout L = make_layout(N, M, max_steps, (uint64_t)grid_offsets[kLevels] * 2, fp32);
    out->total_bytes = L.total;
    out->w_table = L.w_table; out->w_deform = L.w_deform; out->w_sigma0 = L.w_sigma0; out->w_sigma1 = L.w_sigma1; out->w_color = L.w_color;
    out->g_table = L.g_table; out->g_deform = L.g_deform; out->g_sigma0 = L.g_sigma0; out->g_sigma1 = L.g_sigma1; out->g_color = L.g_color;
    out->xyzs = L.pts; out->dirs = L.pts + (uint64_t)M * 12; out->deltas = L.pts + (uint64_t)M * 24; out->rays = L.rays;
    out->sample_set_stride = L.set_stride;
    out->sigmas = L.sigmas; out->weights_sum = L.weights_sum; out->depth = L.depth; out->image = L.image;
    out->found_inf = L.hyper + offsetof(Hyper, found_inf);
    out->enc_in = L.enc_in; out->def_hidden = L.def_hidden; out->def_out = L.def_out; out->xdef = L.xdef; out->grid_out = L.grid_out;
    out->enc_rm = L.enc_rm; out->h1 = L.h1; out->hout = L.hout; out->col_in = L.col_in; out->col_hidden = L.col_hidden; out->col_out = L.col_out;
    out->sq_err = L.sq_err; out->dcol_out = L.dcol_out; out->dh0 = L.dh0; out->col_bwd = L.col_bwd; out->dcol_in = L.dcol_in;
    out->dh = L.dh; out->dh1 = L.dh1; out->denc = L.denc; out->dx = L.dx; out->ddef = L.ddef; out->def_bwd = L.def_bwd;
    return 0;
}

}  // namespace

extern "C" {

int sdn_train_layout(uint32_t N, uint32_t M, uint32_t max_steps, const int32_t *grid_offsets, SdnTrainLayout *out) {
    return fill_layout(N, M, max_steps, grid_offsets, out, false);
}

int sdn_train_refresh(const SdnTrainStep *s, void *stream) {
    if (!workspace_ok(s)) return SDN_E_BADARG;
    for (int i = 0; i < SDN_TRAIN_N_PARAMS; i++) if (!s->params[i].param) return SDN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = table_wait(s, st)) return rc;
    const Layout L = step_layout(s, false);
    unsigned char *ws = (unsigned char *)s->workspace;
    // zero padding of the flat networks, and the table's gradient accumulator
    if (hipMemsetAsync(ws + L.w_deform, 0, kDefFlat * 2, st) != hipSuccess || hipMemsetAsync(ws + L.w_color, 0, kColFlat * 2, st) != hipSuccess ||
        hipMemsetAsync(ws + L.g_table, 0, (uint64_t)s->grid_offsets[kLevels] * 4, st) != hipSuccess || hipMemsetAsync(ws + L.hyper, 0, sizeof(Hyper), st) != hipSuccess)
        return sdn_launch_status();
    AdamArgs<_Float16> A{};
    const uint32_t blocks = build_segments(s, L, A);
    hipLaunchKernelGGL(k_train_copy16, dim3(blocks), dim3(256), 0, st, A);
    return sdn_launch_status();
}

int sdn_train_flush(const SdnTrainStep *s, void *stream) {
    if (!s) return SDN_E_BADARG;
    return table_wait(s, (hipStream_t)stream);
}

int sdn_train_step_f16(const SdnTrainStep *s, void *stream) {
    if (!step_ok(s, false)) return SDN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t N = s->N, M = s->M;
    const Layout L = step_layout(s, false);
    unsigned char *ws = (unsigned char *)s->workspace;
    auto F = [&](uint64_t off) { return (float *)(ws + off); };
    auto H = [&](uint64_t off) { return (_Float16 *)(ws + off); };
    Hyper *hyper = (Hyper *)(ws + L.hyper);
    const int zero_deform = s->time == 0.0f;
    const int no_deform_grad = zero_deform || s->deform_frozen;           // nothing flows back through x + deform
    const int freeze_deform = (zero_deform && !s->keep_deform) || s->deform_frozen;
    int rc;
    const uint64_t set_off = s->sample_set ? L.set_stride : 0;
    float *xyzs = F(L.pts + set_off), *dirs = xyzs + (size_t)M * 3, *deltas = xyzs + (size_t)M * 6;
    const int32_t *ray_table = (const int32_t *)(ws + L.rays + set_off);
    if (s->mode != 2 && s->phase != 2) SDN_TRY(march_samples(s, L, set_off, st));
    if (s->phase == 1) return sdn_launch_status();
    if (s->mode != 2) {
    // (dcol_out .. dh0 are cleared by k_train_encode below: both buffers are padded to 256 bytes, so rounding the range up to 16 is safe)
    const uint32_t zero_n16 = (uint32_t)(((L.dh0 - L.dcol_out) + (uint64_t)M * 2 + 15u) / 16u);
    static_assert(sizeof(uint4) == 16, "");
    if (s->mode == 1) {
        SDN_TRY(table_wait(s, st));
        if (hipMemsetAsync(ws + L.g_table, 0, (uint64_t)s->grid_offsets[kLevels] * 4, st) != hipSuccess) return sdn_launch_status();
    }

    // ---- this step's packed weights (both directions of both fused MLPs, one launch) ------------------------------------------------
    const sdn_ffh::PackJob packs[4] = {{ws + L.w_deform, ws + L.pk_def_f, kDefIn, kDefW, kDefL, 0, 1}, {ws + L.w_deform, ws + L.pk_def_b, kDefIn, kDefW, kDefL, 1, 0},
                                       {ws + L.w_color, ws + L.pk_col_f, kColIn, kColW, kColL, 0, 1}, {ws + L.w_color, ws + L.pk_col_b, kColIn, kColW, kColL, 1, 1}};
    SDN_TRY(sdn_ffh::pack_many(packs, 4, st));

    // ---- forward (network.py:123-169) ---------------------------------------------------------------------------------------------
    if (zero_n16 > M * 16u) return SDN_E_BADARG;     // (34 B per sample + padding: never more than one word per thread)
    hipLaunchKernelGGL(k_train_encode<_Float16>, dim3(sdn_div_up(M * 16u, 256u)), dim3(256), 0, st, xyzs, M, s->time, H(L.enc_in), hyper,
                       (uint4 *)(ws + L.dcol_out), zero_n16);
    SDN_TRY(sdn_ffh::forward_packed(H(L.enc_in), ws + L.pk_def_f, M, kDefIn, kDefW, kDefL, ACT_RELU, H(L.def_hidden), H(L.def_out), st));
    hipLaunchKernelGGL(k_train_xdef<_Float16>, dim3(sdn_div_up(M * 3u, 256u)), dim3(256), 0, st, xyzs, H(L.def_out), M, zero_deform, s->bound, F(L.xdef));
    SDN_TRY(table_wait(s, st));       // the previous step's pass over the table (fp16 copy, gradient accumulator), if it ran on table_stream
    SDN_TRY(sdn_grid_encode_forward(F(L.xdef), ws + L.w_table, s->grid_offsets, ws + L.grid_out, M, 3, 2, kLevels, s->grid_S, s->grid_H,
                                    no_deform_grad ? nullptr : ws + L.dy_dx, 1, 0, 0, SDN_F16, st));
    const SigmaFwd sf{H(L.grid_out), H(L.w_sigma0), H(L.w_sigma1), dirs, H(L.enc_rm), H(L.h1), H(L.hout), H(L.col_in), F(L.sigmas), M, s->density_scale};
    hipLaunchKernelGGL(k_train_sigma_fwd, dim3(sdn_div_up(M, 32u)), dim3(64), 0, st, sf);
    SDN_TRY(sdn_ffh::forward_packed(H(L.col_in), ws + L.pk_col_f, M, kColIn, kColW, kColL, ACT_RELU, H(L.col_hidden), H(L.col_out), st));
    // ---- compositing, loss, and their gradients (renderer.py:309-318, utils.py:85-125), one wave per ray ----------------------------
    const CompositeArgs<Fp16Net> ca{F(L.sigmas), deltas, H(L.col_out), H(L.hout), ray_table, s->bg_color, s->target, s->loss_scale, F(L.weights_sum),
                           F(L.depth), F(L.image), s->image_out, F(L.sq_err), H(L.dcol_out), H(L.dh0), M, N, s->T_thresh, s->bg_value, s->density_scale,
                           s->error_row, s->inds_coarse, s->ray_loss_out};
    hipLaunchKernelGGL(k_train_composite_fwd<Fp16Net>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(k_train_loss, dim3(1), dim3(1024), 0, st, F(L.sq_err), N, s->loss_out);

    // ---- backward through the field ---------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(k_train_composite_bwd<Fp16Net>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, ca);
    SDN_TRY(sdn_ffh::backward_packed(H(L.dcol_out), ws + L.pk_col_b, H(L.col_hidden), M, kColIn, kColW, kColL, ACT_RELU, 1, H(L.col_bwd), H(L.dcol_in), st));
    const SigmaBwd sb{H(L.dh0), H(L.dcol_in), H(L.h1), H(L.w_sigma0), H(L.w_sigma1), H(L.dh), H(L.dh1), H(L.denc), M};
    hipLaunchKernelGGL(k_train_sigma_bwd, dim3(sdn_div_up(M, 32u)), dim3(64), 0, st, sb);
    SDN_TRY(sdn_grid_encode_backward_det(ws + L.denc, F(L.xdef), s->grid_offsets, ws + L.g_table, M, 3, 2, kLevels, s->grid_S, s->grid_H,
                                         no_deform_grad ? nullptr : ws + L.dy_dx, no_deform_grad ? nullptr : ws + L.dx, 1, 0, 0, SDN_F16,
                                         s->det_scratch, st));
    sdn_ffh::DwJob jobs[16];
    uint32_t nj = 0;
    dw_job_list(L, ws, M, jobs, nj);
    if (!no_deform_grad) {
        hipLaunchKernelGGL(k_train_deform_grad<_Float16>, dim3(sdn_div_up(M, 256u)), dim3(256), 0, st, H(L.dx), M, s->bound, H(L.ddef));
        SDN_TRY(sdn_ffh::backward_packed(H(L.ddef), ws + L.pk_def_b, H(L.def_hidden), M, kDefIn, kDefW, kDefL, ACT_RELU, 0, H(L.def_bwd), nullptr, st));
        SDN_TRY(sdn_ffh::dw_jobs(jobs, nj, M, ws + L.dw_partial, st));
    } else {
        SDN_TRY(sdn_ffh::dw_jobs(jobs + (kDefL + 1), nj - (kDefL + 1), M, ws + L.dw_partial, st));   // canonical frame: the deformation MLP has no gradient
    }
    if (no_deform_grad && s->keep_deform && !s->deform_frozen && hipMemsetAsync(ws + L.g_deform, 0, kDefFlat * 2, st) != hipSuccess) return sdn_launch_status();
    }   // mode != 2
    if (s->mode == 1) return sdn_launch_status();

    // ---- optimizer (nerf/utils.py:889-906) --------------------------------------------------------------------------------------------
    const uint32_t table_n = (uint32_t)s->grid_offsets[kLevels] * 2u;
    CheckArgs ck{};
    ck.hyper = hyper;
    ck.g[0] = H(L.g_table); ck.n8[0] = table_n / 8;
    ck.g[1] = H(L.g_sigma0); ck.n8[1] = kSigW * kSigIn / 8;
    ck.g[2] = H(L.g_sigma1); ck.n8[2] = kSigOut * kSigW / 8;
    ck.g[3] = H(L.g_color); ck.n8[3] = kColFlat / 8; ck.col_seg = 3;
    ck.count = 4;
    if (!freeze_deform) { ck.g[4] = H(L.g_deform); ck.n8[4] = kDefFlat / 8; ck.count = 5; }
    const Prologue pr{hyper, s->adam_steps, s->loss_scale, s->growth_tracker, s->beta1, s->beta2, s->lr_table, s->lr_net, s->growth_factor, s->backoff_factor,
                      s->growth_interval, !freeze_deform, s->grad_divisor > 0.0f ? s->grad_divisor : 1.0f};
    hipLaunchKernelGGL(k_train_check, dim3(1024), dim3(256), 0, st, ck);
    hipLaunchKernelGGL(k_train_prologue<true>, dim3(1), dim3(1), 0, st, pr);
    AdamArgs<_Float16> A{};
    adam_args(s, L, hyper, freeze_deform, A);
    if (s->table_stream) {
        if (s->mode == 2) SDN_TRY(table_wait(s, st));           // (optimizer-only call: nothing above waited)
        hipStream_t ts = (hipStream_t)s->table_stream;
        if (hipEventRecord((hipEvent_t)s->table_ready, st) != hipSuccess || hipStreamWaitEvent(ts, (hipEvent_t)s->table_ready, 0) != hipSuccess)
            return sdn_launch_status();
        launch_adam(A, 0, 1, ts);                                // the table: 366 MB of traffic, beside whatever `stream` runs next
        if (hipEventRecord((hipEvent_t)s->table_done, ts) != hipSuccess) return sdn_launch_status();
        launch_adam(A, 1, SDN_TRAIN_N_PARAMS, st);               // the MLPs (the next step's first kernels read their fp16 copies)
    } else {
        launch_adam(A, 0, SDN_TRAIN_N_PARAMS, st);
    }
    return sdn_launch_status();
}

}  // extern "C"

// =====================================================================================================================================
// The training step in fp32 (the reference WITHOUT `-O`: the network in float32, the disabled GradScaler of nerf/utils.py:395):
// sdn_train_step_f32.  The same phases, modes and workspace contract as sdn_train_step_f16.  Shared with it above: the march
// (march_samples), the workspace (make_layout at 4-byte elements), the record checks (step_ok), and the encode, x + deform,
// compositing, loss, deformation-gradient, prologue and Adam kernels instantiated for fp32 (float, Fp32Net, no scaler).  What differs:
//   * every product and sum is fp32.  The three MLP chains run on v_mfma_f32_32x32x2_f32 (one wave = 32 samples, the sample on the
//     lane): accumulator register v of output tile mt IS the B operand of the next layer for the k-pair (row, row + 4), row =
//     32 mt + 8 (v / 4) + v % 4 -- the k-order is baked into the weight packing (k_f32_pack), as in field_f32.hip.  The backward chain
//     is the same kernel shape on the transposed packing, the ReLU' mask read from the stored activations.  All 13 weight gradients
//     are one split-K MFMA launch over 512-sample chunks plus one fixed-order reduction (deterministic).
//   * the grid encoder runs on the fp32 table IN PLACE (no copy) and accumulates an fp32 table gradient;
//   * the optimizer is Adam on the unscaled gradients: no loss scale, no non-finite check, no skip (the disabled scaler does neither);
//     there are no copies to write, the pass clears the fp32 table gradient.
// Launches of a full step: 5 to march (as fp16), pack, encode, 3 forward chains, x + deform, grid forward, compositing forward, loss,
// compositing backward, 2 backward chains (colour, sigma), dh, grid backward, deformation gradient row, deformation backward chain,
// dW + reduction, prologue, Adam.
// =====================================================================================================================================
namespace {

typedef float f32x16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16v mfma32(float a, float b, f32x16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float relu32(float x) { return x > 0.0f ? x : 0.0f; }

// ---- weight packing --------------------------------------------------------------------------------------------------------------
// A product Y[rows] = A[rows, K] x[K] on the matrix cores: packed[((t * S/4 + q) * 64 + lane) * 4 + j] = A[32 t + lane % 32][k(4 q + j,
// lane / 32)].  k(s, h) = 2 s + h when x is loaded from a row-major buffer ("row" order), or 32 (s / 16) + 8 ((s % 16) / 4) + 4 h + s % 4
// when x is the previous layer's accumulator ("acc" order).  A is a layer's weight W (forward) or its transpose (backward); W[r][c] of
// the flat layout reads the parameter with the colour MLP's log-density column (c == split) structurally zero.
struct Pack32 {
    const float *w;              // parameter [rows_w, cols_w]
    float *out;
    uint32_t rows_w, cols_w, split;   // split: flat column that is zero (columns behind it read cols - 1), or 0xFFFFFFFF
    uint32_t tiles, steps, transpose, acc_order, begin;   // begin: first thread of this job
};
struct Pack32Args { Pack32 job[30]; uint32_t n; };

__device__ __forceinline__ float flat_w(const Pack32 &J, uint32_t r, uint32_t c) {
    if (r >= J.rows_w) return 0.0f;
    if (J.split != 0xFFFFFFFFu) {
        if (c == J.split) return 0.0f;
        if (c > J.split) c -= 1;
    }
    return c < J.cols_w ? J.w[(size_t)r * J.cols_w + c] : 0.0f;
}

__global__ void __launch_bounds__(256) k_f32_pack(Pack32Args A) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s = 0;
    for (uint32_t k = 1; k < A.n; k++) s = t >= A.job[k].begin ? k : s;
    const Pack32 &J = A.job[s];
    const uint32_t i = t - J.begin;
    if (i >= J.tiles * J.steps * 64u) return;
    const uint32_t j = i & 3u, lane = (i >> 2) & 63u, q = (i >> 8) % (J.steps / 4u), tile = (i >> 8) / (J.steps / 4u);
    const uint32_t step = 4u * q + j, h = lane >> 5, r = 32u * tile + (lane & 31u);
    const uint32_t k = J.acc_order ? 32u * (step >> 4) + 8u * ((step & 15u) >> 2) + 4u * h + (step & 3u) : 2u * step + h;
    J.out[i] = J.transpose ? flat_w(J, k, r) : flat_w(J, r, k);
}

// one layer: STEPS k-steps of B operands (registers) against packed A operands, MT output tiles
template <uint32_t STEPS, uint32_t MT>
__device__ __forceinline__ void layer32(const float *__restrict__ pk, const float (&b)[STEPS], f32x16v (&acc)[MT], uint32_t lane) {
    #pragma unroll
    for (uint32_t mt = 0; mt < MT; mt++) acc[mt] = f32x16v{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    #pragma unroll
    for (uint32_t q = 0; q < STEPS / 4; q++) {
        float4 a[MT];
        #pragma unroll
        for (uint32_t mt = 0; mt < MT; mt++) a[mt] = reinterpret_cast<const float4 *>(pk)[((size_t)mt * (STEPS / 4) + q) * 64 + lane];
        #pragma unroll
        for (uint32_t mt = 0; mt < MT; mt++) {
            acc[mt] = mfma32(a[mt].x, b[4 * q + 0], acc[mt]);
            acc[mt] = mfma32(a[mt].y, b[4 * q + 1], acc[mt]);
            acc[mt] = mfma32(a[mt].z, b[4 * q + 2], acc[mt]);
            acc[mt] = mfma32(a[mt].w, b[4 * q + 3], acc[mt]);
        }
    }
}

// B operands of a row-major [*, LD] input row (k-step s, half h: element 2 s + h); 16-byte loads
template <uint32_t LD>
__device__ __forceinline__ void load_row_b(const float *__restrict__ row, bool live, uint32_t h, float (&b)[LD / 2]) {
    #pragma unroll
    for (uint32_t j = 0; j < LD / 4; j++) {
        const float4 v = live ? reinterpret_cast<const float4 *>(row)[j] : float4{0, 0, 0, 0};
        b[2 * j] = h ? v.y : v.x;
        b[2 * j + 1] = h ? v.w : v.z;
    }
}

// the 16 rows this lane holds of tile mt (rows 32 mt + 8 q + 4 h + 0..3) <-> a row-major [*, ld] row
template <uint32_t MT>
__device__ __forceinline__ void store_tiles(float *__restrict__ row, const f32x16v (&acc)[MT], uint32_t h) {
    #pragma unroll
    for (uint32_t mt = 0; mt < MT; mt++)
        #pragma unroll
        for (uint32_t q = 0; q < 4; q++)
            *reinterpret_cast<float4 *>(row + 32 * mt + 8 * q + 4 * h) = float4{acc[mt][4 * q], acc[mt][4 * q + 1], acc[mt][4 * q + 2], acc[mt][4 * q + 3]};
}

// ---- forward chain: X -> L hidden layers of width 32 MT (ReLU) -> 16 outputs (rows >= the real output count are zero) --------------
// X is row-major [M, IN] or, with LEVEL_MAJOR, the grid encoder's [IN / 2][M][2].  Hidden activations (after the ReLU) are kept
// row-major [L][M][32 MT] for the backward chain and the weight gradients; outputs row-major [M, 16].
template <uint32_t IN, uint32_t MT, uint32_t L, bool LEVEL_MAJOR>
__global__ void __launch_bounds__(64) k_f32_chain_fwd(const float *__restrict__ X, const float *__restrict__ pk, uint32_t M, float *__restrict__ hidden,
                                                      float *__restrict__ out) {
    constexpr uint32_t W = 32 * MT, S = 16 * MT;
    const uint32_t lane = threadIdx.x, n = lane & 31u, h = lane >> 5;
    const uint32_t b_raw = blockIdx.x * 32 + n;
    const bool live = b_raw < M;
    const uint32_t b = live ? b_raw : M - 1;
    f32x16v acc[MT];
    {
        float bin[IN / 2];
        if constexpr (LEVEL_MAJOR) {
            #pragma unroll
            for (uint32_t s = 0; s < IN / 2; s++) bin[s] = live ? X[((size_t)s * M + b) * 2 + h] : 0.0f;
        } else {
            load_row_b<IN>(X + (size_t)b * IN, live, h, bin);
        }
        layer32<IN / 2, MT>(pk, bin, acc, lane);
        pk += (size_t)MT * (IN / 2) * 64;
    }
    for (uint32_t l = 0; l < L; l++) {
        float bh[S];
        #pragma unroll
        for (uint32_t mt = 0; mt < MT; mt++)
            #pragma unroll
            for (uint32_t v = 0; v < 16; v++) { const float r = relu32(acc[mt][v]); bh[16 * mt + v] = r; acc[mt][v] = r; }
        if (live) store_tiles<MT>(hidden + ((size_t)l * M + b) * W, acc, h);
        if (l + 1 < L) {
            layer32<S, MT>(pk, bh, acc, lane);
            pk += (size_t)MT * S * 64;
        } else {
            f32x16v o[1];
            layer32<S, 1>(pk, bh, o, lane);
            if (live) {
                float *row = out + (size_t)b * 16;
                *reinterpret_cast<float4 *>(row + 4 * h) = float4{o[0][0], o[0][1], o[0][2], o[0][3]};
                *reinterpret_cast<float4 *>(row + 8 + 4 * h) = float4{o[0][4], o[0][5], o[0][6], o[0][7]};
            }
        }
    }
}

// ---- backward chain: dY [M, 16] -> G_l = (W_{l+1}^T G_{l+1}) * relu'(h_l) for l = L-1 .. 0 (row-major [L][M][32 MT]) -> optionally
// dX = W_0^T G_0, DXT tiles of 32 input features, row-major [M, 32 DXT] or (LEVEL_MAJOR) the grid encoder's [32 DXT / 2][M][2]
template <uint32_t MT, uint32_t L, uint32_t DXT, bool LEVEL_MAJOR>
__global__ void __launch_bounds__(64) k_f32_chain_bwd(const float *__restrict__ dY, const float *__restrict__ pk, const float *__restrict__ hidden, uint32_t M,
                                                      float *__restrict__ G, float *__restrict__ dX) {
    constexpr uint32_t W = 32 * MT, S = 16 * MT;
    const uint32_t lane = threadIdx.x, n = lane & 31u, h = lane >> 5;
    const uint32_t b_raw = blockIdx.x * 32 + n;
    const bool live = b_raw < M;
    const uint32_t b = live ? b_raw : M - 1;
    f32x16v acc[MT];
    {
        float bin[8];
        load_row_b<16>(dY + (size_t)b * 16, live, h, bin);
        layer32<8, MT>(pk, bin, acc, lane);
        pk += (size_t)MT * 8 * 64;
    }
    for (int l = (int)L - 1; l >= 0; l--) {
        const float *act = hidden + ((size_t)l * M + b) * W;
        float bh[S];
        #pragma unroll
        for (uint32_t mt = 0; mt < MT; mt++)
            #pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                const float4 a = live ? *reinterpret_cast<const float4 *>(act + 32 * mt + 8 * q + 4 * h) : float4{0, 0, 0, 0};
                const float av[4] = {a.x, a.y, a.z, a.w};
                #pragma unroll
                for (uint32_t e = 0; e < 4; e++) {
                    const float g = av[e] > 0.0f ? acc[mt][4 * q + e] : 0.0f;
                    acc[mt][4 * q + e] = g;
                    bh[16 * mt + 4 * q + e] = g;
                }
            }
        if (live) store_tiles<MT>(G + ((size_t)l * M + b) * W, acc, h);
        if (l > 0) {
            layer32<S, MT>(pk, bh, acc, lane);
            pk += (size_t)MT * S * 64;
        } else if constexpr (DXT > 0) {
            f32x16v d[DXT];
            layer32<S, DXT>(pk, bh, d, lane);
            if (live) {
                if constexpr (LEVEL_MAJOR) {
                    #pragma unroll
                    for (uint32_t t = 0; t < DXT; t++)
                        #pragma unroll
                        for (uint32_t q = 0; q < 4; q++) {
                            const uint32_t f = 32 * t + 8 * q + 4 * h;      // features f .. f + 3 = levels f / 2, f / 2 + 1
                            *reinterpret_cast<float2 *>(dX + ((size_t)(f / 2) * M + b) * 2) = float2{d[t][4 * q], d[t][4 * q + 1]};
                            *reinterpret_cast<float2 *>(dX + ((size_t)(f / 2 + 1) * M + b) * 2) = float2{d[t][4 * q + 2], d[t][4 * q + 3]};
                        }
                } else {
                    store_tiles<DXT>(dX + (size_t)b * 32 * DXT, d, h);
                }
            }
        }
    }
}

// ---- weight gradients: dW[R, C] = sum_b G[b][r] X[b][c], one wave per (job, 32 x 32 tile, 512-sample chunk), partial sums per chunk,
// then one reduction over the chunks in a fixed order
struct Dw32 {
    const float *G, *X;
    float *out;
    uint32_t ldg, ldx, R, C, x_level_major;
    uint32_t tiles_c, tile_begin, out_begin;       // tile_begin: first tile of this job; out_begin: offset in a chunk's partial row
};
struct Dw32Args { Dw32 job[13]; uint32_t n, tiles, total; };

__global__ void __launch_bounds__(64) k_f32_dw(Dw32Args A, uint32_t M, float *__restrict__ partial) {
    const uint32_t tile = blockIdx.x, chunk = blockIdx.y;
    uint32_t s = 0;
    for (uint32_t k = 1; k < A.n; k++) s = tile >= A.job[k].tile_begin ? k : s;
    const Dw32 &J = A.job[s];
    const uint32_t lane = threadIdx.x, n = lane & 31u, h = lane >> 5;
    const uint32_t t = tile - J.tile_begin, tr = t / J.tiles_c, tc = t - tr * J.tiles_c;
    const uint32_t r = 32 * tr + n, c = 32 * tc + n;
    const bool r_ok = r < J.R, c_ok = c < J.C;
    f32x16v acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t b0 = chunk * kDwChunk, b1 = min(b0 + kDwChunk, M);
    for (uint32_t bb = b0; bb < b1; bb += 8) {
        float a[4], x[4];
        #pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t b = bb + 2 * u + h;
            const bool ok = b < b1;
            a[u] = ok && r_ok ? J.G[(size_t)b * J.ldg + r] : 0.0f;
            x[u] = !(ok && c_ok) ? 0.0f : J.x_level_major ? J.X[((size_t)(c >> 1) * M + b) * 2 + (c & 1u)] : J.X[(size_t)b * J.ldx + c];
        }
        #pragma unroll
        for (uint32_t u = 0; u < 4; u++) acc = mfma32(a[u], x[u], acc);
    }
    float *dst = partial + (size_t)chunk * A.total + J.out_begin;
    #pragma unroll
    for (uint32_t v = 0; v < 16; v++) {
        const uint32_t row = 32 * tr + 8 * (v >> 2) + 4 * h + (v & 3u);
        if (row < J.R && c_ok) dst[(size_t)row * J.C + c] = acc[v];
    }
}

__global__ void __launch_bounds__(256) k_f32_dw_reduce(Dw32Args A, uint32_t chunks, const float *__restrict__ partial) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.total) return;
    uint32_t s = 0;
    for (uint32_t k = 1; k < A.n; k++) s = i >= A.job[k].out_begin ? k : s;
    float sum = 0.0f;
    for (uint32_t c = 0; c < chunks; c++) sum += partial[(size_t)c * A.total + i];
    A.job[s].out[i - A.job[s].out_begin] = sum;
}

// ---- glue -------------------------------------------------------------------------------------------------------------------------
// sigma = density_scale * exp(h[0]) (trunc_exp forward, activation.py:5-11); the colour MLP's input row [SH(d, 4) 16 | sigma-MLP output 16]
__global__ void __launch_bounds__(256) k_f32_sigma_post(const float *__restrict__ hout, const float *__restrict__ dirs, uint32_t M, float density_scale,
                                                        float *__restrict__ sigmas, float *__restrict__ col_in) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= M) return;
    float sh[16], u0[1], u1[1], u2[1];
    sh_eval<4, false>(dirs[(size_t)b * 3], dirs[(size_t)b * 3 + 1], dirs[(size_t)b * 3 + 2], sh, u0, u1, u2);
    float4 *row = reinterpret_cast<float4 *>(col_in + (size_t)b * kColIn);
    const float4 *o = reinterpret_cast<const float4 *>(hout + (size_t)b * 16);
    #pragma unroll
    for (int j = 0; j < 4; j++) { row[j] = float4{sh[4 * j], sh[4 * j + 1], sh[4 * j + 2], sh[4 * j + 3]}; row[4 + j] = o[j]; }
    sigmas[b] = density_scale * expf(hout[(size_t)b * 16]);
}

// d(sigma-MLP output) = [trunc_exp gradient | columns 17 .. 31 of the colour MLP's input gradient]
__global__ void __launch_bounds__(256) k_f32_dh(const float *__restrict__ dh0, const float *__restrict__ dcol_in, uint32_t M, float *__restrict__ dh) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * 16) return;
    const uint32_t b = t >> 4, c = t & 15u;
    dh[t] = c == 0 ? dh0[b] : dcol_in[(size_t)b * kColIn + 16 + c];
}

// the 13 weight-gradient products (deformation MLP first: the canonical frame launches only the rest)
uint32_t dw32_jobs(const Layout &L, unsigned char *ws, uint32_t M, bool with_deform, Dw32Args &A) {
    auto F = [&](uint64_t off) { return (float *)(ws + off); };
    const size_t mw = (size_t)M * kDefW, mc = (size_t)M * kColW;
    Dw32 j[13];
    uint32_t n = 0;
    if (with_deform) {
        j[n++] = {F(L.def_bwd), F(L.enc_in), F(L.g_deform), kDefW, kDefIn, kDefW, kDefIn, 0};
        for (uint32_t l = 1; l < kDefL; l++)
            j[n++] = {F(L.def_bwd) + l * mw, F(L.def_hidden) + (l - 1) * mw, F(L.g_deform) + kDefW * kDefIn + (l - 1) * kDefW * kDefW, kDefW, kDefW, kDefW, kDefW, 0};
        j[n++] = {F(L.ddef), F(L.def_hidden) + (kDefL - 1) * mw, F(L.g_deform) + kDefW * kDefIn + (kDefL - 1) * kDefW * kDefW, 16, kDefW, 16, kDefW, 0};
    }
    j[n++] = {F(L.dh1), F(L.grid_out), F(L.g_sigma0), kSigW, 0, kSigW, kSigIn, 1};
    j[n++] = {F(L.dh), F(L.h1), F(L.g_sigma1), kSigOut, kSigW, kSigOut, kSigW, 0};
    j[n++] = {F(L.col_bwd), F(L.col_in), F(L.g_color), kColW, kColIn, kColW, kColIn, 0};
    j[n++] = {F(L.col_bwd) + mc, F(L.col_hidden), F(L.g_color) + kColW * kColIn, kColW, kColW, kColW, kColW, 0};
    j[n++] = {F(L.dcol_out), F(L.col_hidden) + mc, F(L.g_color) + kColW * kColIn + kColW * kColW, 16, kColW, 16, kColW, 0};
    uint32_t tiles = 0, total = 0;
    for (uint32_t i = 0; i < n; i++) {
        j[i].tiles_c = sdn_div_up(j[i].C, 32u);
        j[i].tile_begin = tiles;
        j[i].out_begin = total;
        tiles += sdn_div_up(j[i].R, 32u) * j[i].tiles_c;
        total += j[i].R * j[i].C;
        A.job[i] = j[i];
    }
    A.n = n; A.tiles = tiles; A.total = total;
    return n;
}

// both directions of the three MLPs from the fp32 parameters (params 1 .. 13), one launch
void pack32_jobs(const SdnTrainStep *s, const Layout &L, unsigned char *ws, Pack32Args &A) {
    float *pk = (float *)(ws + L.pk);
    uint32_t n = 0, thr = 0;
    auto add = [&](uint32_t pi, uint64_t &at, uint32_t out_rows, uint32_t steps, int transpose, int acc, uint32_t rows_w, uint32_t cols_w, uint32_t split) {
        Pack32 &J = A.job[n++];
        J.w = s->params[pi].param; J.out = pk + at;
        J.rows_w = rows_w; J.cols_w = cols_w; J.split = split;
        J.tiles = sdn_div_up(out_rows, 32u); J.steps = steps; J.transpose = (uint32_t)transpose; J.acc_order = (uint32_t)acc; J.begin = thr;
        const uint32_t cnt = J.tiles * steps * 64u;
        thr += sdn_div_up(cnt, 256u) * 256u;                // every job starts on a workgroup boundary
        at += cnt;
    };
    const uint32_t NS = 0xFFFFFFFFu;
    // deformation: fwd first [128, 80 (76)], hidden [128,128] x 6, last [16 (3), 128]; bwd last^T, hidden^T (7 .. 2), no first^T
    uint64_t at = kPkDefF;
    add(1, at, kDefW, kDefIn / 2, 0, 0, kDefW, kDefCols, NS);
    for (uint32_t l = 1; l < kDefL; l++) add(1 + l, at, kDefW, kDefW / 2, 0, 1, kDefW, kDefW, NS);
    add(8, at, 16, kDefW / 2, 0, 1, 3, kDefW, NS);
    at = kPkDefB;
    add(8, at, kDefW, 8, 1, 0, 3, kDefW, NS);
    for (uint32_t l = kDefL - 1; l >= 1; l--) add(1 + l, at, kDefW, kDefW / 2, 1, 1, kDefW, kDefW, NS);
    // sigma: fwd [64, 32], [16, 64]; bwd [16, 64]^T, [64, 32]^T
    at = kPkSigF;
    add(9, at, kSigW, kSigIn / 2, 0, 0, kSigW, kSigIn, NS);
    add(10, at, 16, kSigW / 2, 0, 1, kSigOut, kSigW, NS);
    at = kPkSigB;
    add(10, at, kSigW, 8, 1, 0, kSigOut, kSigW, NS);
    add(9, at, kSigIn, kSigW / 2, 1, 1, kSigW, kSigIn, NS);
    // colour: input [SH 16 | zero column | geo 15]
    at = kPkColF;
    add(11, at, kColW, kColIn / 2, 0, 0, kColW, kColCols, 16);
    add(12, at, kColW, kColW / 2, 0, 1, kColW, kColW, NS);
    add(13, at, 16, kColW / 2, 0, 1, 3, kColW, NS);
    at = kPkColB;
    add(13, at, kColW, 8, 1, 0, 3, kColW, NS);
    add(12, at, kColW, kColW / 2, 1, 1, kColW, kColW, NS);
    add(11, at, kColIn, kColW / 2, 1, 1, kColW, kColCols, 16);
    A.n = n;
}

uint32_t pack32_threads(const Pack32Args &A) {
    const Pack32 &J = A.job[A.n - 1];
    return J.begin + J.tiles * J.steps * 64u;
}

}  // namespace

extern "C" {

int sdn_train_layout_f32(uint32_t N, uint32_t M, uint32_t max_steps, const int32_t *grid_offsets, SdnTrainLayout *out) {
    return fill_layout(N, M, max_steps, grid_offsets, out, true);
}

int sdn_train_refresh_f32(const SdnTrainStep *s, void *stream) {
    if (!workspace_ok(s) || s->N == 0 || s->M == 0 || s->max_steps == 0 || s->grid_offsets[kLevels] <= 0) return SDN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = step_layout(s, true);
    unsigned char *ws = (unsigned char *)s->workspace;
    if (hipMemsetAsync(ws + L.g_table, 0, (uint64_t)s->grid_offsets[kLevels] * 8, st) != hipSuccess || hipMemsetAsync(ws + L.hyper, 0, sizeof(Hyper), st) != hipSuccess)
        return sdn_launch_status();
    return sdn_launch_status();
}

int sdn_train_step_f32(const SdnTrainStep *s, void *stream) {
    if (!step_ok(s, true)) return SDN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t N = s->N, M = s->M;
    const Layout L = step_layout(s, true);
    unsigned char *ws = (unsigned char *)s->workspace;
    auto F = [&](uint64_t off) { return (float *)(ws + off); };
    Hyper *hyper = (Hyper *)(ws + L.hyper);
    const int zero_deform = s->time == 0.0f;
    const int no_deform_grad = zero_deform || s->deform_frozen;
    const int freeze_deform = zero_deform || s->deform_frozen;
    int rc;
    const uint64_t set_off = s->sample_set ? L.set_stride : 0;
    float *xyzs = F(L.pts + set_off), *dirs = xyzs + (size_t)M * 3, *deltas = xyzs + (size_t)M * 6;
    const int32_t *ray_table = (const int32_t *)(ws + L.rays + set_off);
    if (s->phase != 2) SDN_TRY(march_samples(s, L, set_off, st));
    if (s->phase == 1) return sdn_launch_status();
    const float *table = s->params[0].param;
    float *g_table = F(L.g_table);
    if (s->mode == 1 && hipMemsetAsync(g_table, 0, (uint64_t)s->grid_offsets[kLevels] * 8, st) != hipSuccess) return sdn_launch_status();
    // the gradient rows compositing fills only for the samples rays own, and dh0 behind them
    if (hipMemsetAsync(ws + L.dcol_out, 0, L.dh0 - L.dcol_out + (uint64_t)M * 4, st) != hipSuccess) return sdn_launch_status();

    // ---- this step's packed weights (both directions of the three MLPs, one launch) --------------------------------------------------
    Pack32Args pa{};
    pack32_jobs(s, L, ws, pa);
    hipLaunchKernelGGL(k_f32_pack, dim3(sdn_div_up(pack32_threads(pa), 256u)), dim3(256), 0, st, pa);
    const float *pk = F(L.pk);
    const dim3 waves(sdn_div_up(M, 32u));

    // ---- forward (network.py:123-169 in fp32) -------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(k_train_encode<float>, dim3(sdn_div_up(M * 16u, 256u)), dim3(256), 0, st, xyzs, M, s->time, F(L.enc_in), nullptr, nullptr, 0u);
    hipLaunchKernelGGL((k_f32_chain_fwd<kDefIn, kDefW / 32, kDefL, false>), waves, dim3(64), 0, st, F(L.enc_in), pk + kPkDefF, M, F(L.def_hidden), F(L.def_out));
    hipLaunchKernelGGL(k_train_xdef<float>, dim3(sdn_div_up(M * 3u, 256u)), dim3(256), 0, st, xyzs, F(L.def_out), M, zero_deform, s->bound, F(L.xdef));
    SDN_TRY(sdn_grid_encode_forward(F(L.xdef), table, s->grid_offsets, F(L.grid_out), M, 3, 2, kLevels, s->grid_S, s->grid_H,
                                    no_deform_grad ? nullptr : F(L.dy_dx), 1, 0, 0, SDN_F32, st));
    hipLaunchKernelGGL((k_f32_chain_fwd<kSigIn, kSigW / 32, 1, true>), waves, dim3(64), 0, st, F(L.grid_out), pk + kPkSigF, M, F(L.h1), F(L.hout));
    hipLaunchKernelGGL(k_f32_sigma_post, dim3(sdn_div_up(M, 256u)), dim3(256), 0, st, F(L.hout), dirs, M, s->density_scale, F(L.sigmas), F(L.col_in));
    hipLaunchKernelGGL((k_f32_chain_fwd<kColIn, kColW / 32, kColL, false>), waves, dim3(64), 0, st, F(L.col_in), pk + kPkColF, M, F(L.col_hidden), F(L.col_out));
    // ---- compositing, loss and their gradients, one wave per ray -------------------------------------------------------------------------
    const CompositeArgs<Fp32Net> ca{F(L.sigmas), deltas, F(L.col_out), F(L.hout), ray_table, s->bg_color, s->target, nullptr, F(L.weights_sum), F(L.depth),
                                    F(L.image), s->image_out, F(L.sq_err), F(L.dcol_out), F(L.dh0), M, N, s->T_thresh, s->bg_value,
                                    s->density_scale, s->error_row, s->inds_coarse, s->ray_loss_out};
    hipLaunchKernelGGL(k_train_composite_fwd<Fp32Net>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(k_train_loss, dim3(1), dim3(1024), 0, st, F(L.sq_err), N, s->loss_out);
    hipLaunchKernelGGL(k_train_composite_bwd<Fp32Net>, dim3(sdn_div_up(N, 4u)), dim3(256), 0, st, ca);

    // ---- backward through the field ----------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL((k_f32_chain_bwd<kColW / 32, kColL, 1, false>), waves, dim3(64), 0, st, F(L.dcol_out), pk + kPkColB, F(L.col_hidden), M,
                       F(L.col_bwd), F(L.dcol_in));
    hipLaunchKernelGGL(k_f32_dh, dim3(sdn_div_up(M * 16u, 256u)), dim3(256), 0, st, F(L.dh0), F(L.dcol_in), M, F(L.dh));
    hipLaunchKernelGGL((k_f32_chain_bwd<kSigW / 32, 1, 1, true>), waves, dim3(64), 0, st, F(L.dh), pk + kPkSigB, F(L.h1), M, F(L.dh1), F(L.denc));
    if (s->det_scratch)
        SDN_TRY(sdn_grid_encode_backward_det(F(L.denc), F(L.xdef), s->grid_offsets, g_table, M, 3, 2, kLevels, s->grid_S, s->grid_H,
                                             no_deform_grad ? nullptr : F(L.dy_dx), no_deform_grad ? nullptr : F(L.dx), 1, 0, 0, SDN_F32, s->det_scratch, st));
    else
        SDN_TRY(sdn_grid_encode_backward(F(L.denc), F(L.xdef), s->grid_offsets, g_table, M, 3, 2, kLevels, s->grid_S, s->grid_H,
                                         no_deform_grad ? nullptr : F(L.dy_dx), no_deform_grad ? nullptr : F(L.dx), 1, 0, 0, SDN_F32, st));
    if (!no_deform_grad) {
        hipLaunchKernelGGL(k_train_deform_grad<float>, dim3(sdn_div_up(M, 256u)), dim3(256), 0, st, F(L.dx), M, s->bound, F(L.ddef));
        hipLaunchKernelGGL((k_f32_chain_bwd<kDefW / 32, kDefL, 0, false>), waves, dim3(64), 0, st, F(L.ddef), pk + kPkDefB, F(L.def_hidden), M,
                           F(L.def_bwd), (float *)nullptr);
    } else if (hipMemsetAsync(ws + L.g_deform, 0, kDefFlat * 4, st) != hipSuccess) {      // no gradient: zeros, not last step's values
        return sdn_launch_status();
    }
    Dw32Args da{};
    dw32_jobs(L, ws, M, !no_deform_grad, da);
    const uint32_t chunks = sdn_div_up(M, kDwChunk);
    hipLaunchKernelGGL(k_f32_dw, dim3(da.tiles, chunks), dim3(64), 0, st, da, M, F(L.dw_partial));
    hipLaunchKernelGGL(k_f32_dw_reduce, dim3(sdn_div_up(da.total, 256u)), dim3(256), 0, st, da, chunks, F(L.dw_partial));
    if (s->mode == 1) return sdn_launch_status();

    // ---- optimizer: Adam on the unscaled gradients, every step counts (the disabled GradScaler) -------------------------------------------
    Prologue pr{};                     // (no scaler: loss scale, growth tracker and found_inf are not read)
    pr.hyper = hyper; pr.steps = s->adam_steps; pr.beta1 = s->beta1; pr.beta2 = s->beta2; pr.lr_table = s->lr_table; pr.lr_net = s->lr_net;
    pr.deform_active = !freeze_deform;
    hipLaunchKernelGGL(k_train_prologue<false>, dim3(1), dim3(1), 0, st, pr);
    AdamArgs<float> A{};
    const uint32_t blocks = adam_args(s, L, hyper, freeze_deform, A);
    hipLaunchKernelGGL(k_train_adam<float>, dim3(blocks), dim3(256), 0, st, A);
    return sdn_launch_status();
}

}  // extern "C"
