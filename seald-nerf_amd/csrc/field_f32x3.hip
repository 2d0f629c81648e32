// The fused field network with fp32 ACCURACY on the fp16 matrix pipes (field_f32_net.h has the network and the mapping): every fp32
// operand is split x = hi + lo (two fp16 values, 22 bits of mantissa) and a product is three MFMAs -- hi.hi + hi.lo + lo.hi, accumulated
// in fp32 (the dropped lo.lo term is 2^-22 relative).  v_mfma_f32_32x32x16_f16 does 16 k-steps in 32 cycles where v_mfma_f32_32x32x2_f32
// does 2 in 64: three of them are 3 / 16 of the fp32 MFMA time, paid for with three vector instructions per activation (max, convert,
// subtract-convert).  Same 1e-4 bar against the fp32 network as field_f32.hip.
//
// Operands.  The layout is the fp16 kernel's (field.hip): accumulator registers 8 s .. 8 s + 7 of output tile t are k-step (t, s) of
// the next layer's B operand, the k-order baked into the weight packing (dnerf_amd/fused.py kmaps, reused by fused_f32.py:
// pack_weights_f32_split).  Packed weights, per layer: [k-step][lane][m-tile][hi | lo][8 halves] -- one lane reads its 32 bytes per
// m-tile with two ds_read_b128.
//
// Scaling.  The fp16 MFMA flushes subnormal inputs, and the lo part of a value is 2^-12 of it: unscaled, every activation below 0.25 and
// every weight below 0.25 would lose its lo part (measured: 2e-4 relative errors).  Activations travel as 2^6 x and weights as 2^8 w
// (exact scalings), accumulators hold 2^14 times the layer's output and are brought back by the 2^-8 of the next split / the 2^-14 of an
// output: lo parts stay normal down to |x| = 4e-3 and |w| = 1e-3, the hi parts fit fp16 up to |x| = 1023 and |w| = 255.
// Above that the kernel is LOUD, not wrong: the packer refuses |w| > 255.875 (fused_f32.py), and an activation from 1023.75 on converts
// to hi = +inf, lo = -inf, every product with it is NaN, the ReLU keeps NaNs (relu1_keep_nan) and the point's sigma or rgb comes out
// NaN (tests/test_gpu_field_ranges.py); the other points of the launch are untouched.
#include "field_f32_net.h"

namespace {

using namespace sdn_f32;

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
struct Split { half8_t hi, lo; };

struct SplitF16 {
    using Operand = Split;                      // one k-step of 16: lane half h holds k = 8 h .. 8 h + 7 of it
    static constexpr int kPerOperand = 16;
    static constexpr bool kScaled = true;
    static constexpr float kXS = 64.0f, kWS = 256.0f;            // operand scales (see "Scaling"); accumulators carry kXS * kWS
    static constexpr float kAccScale = kXS * kWS, kAccToX = 1.0f / kWS, kAccToOut = 1.0f / (kXS * kWS);
    // offsets inside the tail stage (floats): [k-step][lane][m-tile][hi | lo][8 halves] blocks
    static constexpr int kBlk = 64 * 8;   // floats of one (k-step, m-tile): 64 lanes x 32 bytes
    static constexpr int kT_D7 = 0, kT_S0 = kT_D7 + 8 * kBlk, kT_S1 = kT_S0 + 2 * 2 * kBlk, kT_C0 = kT_S1 + 4 * kBlk, kT_C1 = kT_C0 + 2 * 2 * kBlk,
                         kT_C2 = kT_C1 + 4 * 2 * kBlk;
    static_assert(kT_C2 + 4 * kBlk == kTailFloats && 4 * 4 * kBlk == kD0Floats, "stage sizes");

    static __device__ __forceinline__ Split split8(const float (&x)[8], float scale) {      // x * scale = hi + lo
        Split r;
        #pragma unroll
        for (int j = 0; j < 8; j++) {
            r.hi[j] = (_Float16)(x[j] * scale);
            // (one fused multiply-add that reads the fp16 operand in place -- v_fma_mix_f32 -- instead of convert-back, multiply, subtract;
            //  the scaling is by a power of two, so the product is exact either way)
            r.lo[j] = (_Float16)__builtin_fmaf(x[j], scale, -(float)r.hi[j]);
        }
        return r;
    }

    // one layer: KS k-steps of 16 (B operands split in registers) against the staged split A operands, MT output tiles of 32 rows
    template <int KS, int MT>
    static __device__ __forceinline__ void layer(const float *s_w, const Split (&b)[KS], float16_t (&acc)[MT], uint32_t lane) {
        #pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const uint4 *src = reinterpret_cast<const uint4 *>(s_w) + ((size_t)ks * 64 + lane) * MT * 2;
            half8_t ah[MT], al[MT];
            #pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                ah[mt] = __builtin_bit_cast(half8_t, src[2 * mt]);
                al[mt] = __builtin_bit_cast(half8_t, src[2 * mt + 1]);
            }
            #pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], b[ks].hi, acc[mt], 0, 0, 0);
            #pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], b[ks].lo, acc[mt], 0, 0, 0);
            #pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], b[ks].hi, acc[mt], 0, 0, 0);
#ifdef SDN_X3_LOLO
            // (the fourth term, 2^-22 of the product: measured, changes no result at the test's resolution -- what separates this kernel from the
            //  fp32 one is the 22-bit operands, not the dropped term)
            #pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], b[ks].lo, acc[mt], 0, 0, 0);
#endif
        }
    }

    // accumulator registers 8 s .. 8 s + 7 of tile t -> k-step 2 t + s of the next layer (ReLU, then the split)
    template <int MT>
    static __device__ __forceinline__ void next(const float16_t (&acc)[MT], Split (&b)[2 * MT]) {
        #pragma unroll
        for (int t = 0; t < MT; t++)
            #pragma unroll
            for (int sh = 0; sh < 2; sh++) {
                float x[8];
                #pragma unroll
                for (int j = 0; j < 8; j++) x[j] = relu1_keep_nan(acc[t][8 * sh + j]);      // (an overflow upstream stays NaN)
                b[2 * t + sh] = split8(x, kAccToX);       // accumulators hold kXS kWS y: the next operand is kXS y
            }
    }

    // k position (k-step s, lane half h, j), q = 8 s + j: q < 30 -> pair (f, d) = (5 h + (q >> 1) / 3, (q >> 1) % 3), sine for even q, the
    // reference's phase-shifted sine (the cosine) for odd q; q = 30 -> x0 | x2; q = 31 -> x1 | -   (fused.py _d0_kmap)
    static __device__ __forceinline__ void deal_freq(const float (&x)[3], uint32_t h, Split (&b)[8]) {
        float f[32];
        #pragma unroll
        for (int q = 0; q < 30; q++) {
            const int pr = q >> 1;
            const float xa = h ? x[(15 + pr) % 3] : x[pr % 3];
            const int fa = pr / 3, fb = 5 + pr / 3;
            const float arg = h ? scalbnf(xa, fb) : scalbnf(xa, fa);
            f[q] = sinf(arg + (float)(q & 1) * (3.141592653589793f / 2));
        }
        f[30] = h ? x[2] : x[0];
        f[31] = h ? 0.0f : x[1];
        #pragma unroll
        for (int sk = 0; sk < 4; sk++) {
            float xs[8];
            #pragma unroll
            for (int j = 0; j < 8; j++) xs[j] = f[8 * sk + j];
            b[sk] = split8(xs, kXS);
        }
    }
    // lane half h owns levels 8 h .. 8 h + 7, both channels (fused.py _s0_kmap: k position (s, h, j) = level 8 h + 4 s + (j >> 1),
    // channel j & 1)
    static __device__ __forceinline__ void deal_grid(const float *table, const LevelParams &lp, const float (&in)[3], bool oob, uint32_t h,
                                                     Split (&b)[2]) {
        #pragma unroll
        for (int sk = 0; sk < 2; sk++) {
            float g[8];
            #pragma unroll
            for (int lv = 0; lv < 4; lv++) trilinear<true>(table, lp, 8u * h + 4u * sk + lv, in, oob, h, g[2 * lv], g[2 * lv + 1]);
            b[sk] = split8(g, kXS);
        }
    }
    // k-step 0 = the sigma net's 16 outputs in accumulator order, k-step 1 = SH coefficient 8 h + j (fused.py _c0_kmap)
    static __device__ __forceinline__ void deal_geo(const float16_t &a, Split (&b)[2]) {
        float xs[8];
        #pragma unroll
        for (int j = 0; j < 8; j++) xs[j] = a[j];
        b[0] = split8(xs, kAccToX);
    }
    static __device__ __forceinline__ void deal_sh(const float (&sh)[16], uint32_t h, Split (&b)[2]) {
        float xs[8];
        #pragma unroll
        for (int j = 0; j < 8; j++) xs[j] = h ? sh[8 + j] : sh[j];
        b[1] = split8(xs, kXS);
    }
};

__global__ void __launch_bounds__(64 * kWaves, 8 / kWaves) k_field_f32x3(F32Args P, LevelParams lp) {
    __shared__ __attribute__((aligned(16))) float s_w[kStageFloats];
    __shared__ float s_bias[kMaxFrames * 128];
    field_net<SplitF16, false>(P, lp, s_w, s_bias);
}

}  // namespace

namespace sdn_int {
int field_forward_f32x3(const FieldCall &f, hipStream_t st) { return sdn_f32::launch_field(k_field_f32x3, f, nullptr, st); }
}  // namespace sdn_int

extern "C" {

int sdn_field_forward_f32x3(const float *xyzs, const float *dirs, const uint32_t *live_idx, const uint32_t *live_count, uint32_t M,
                            const float *weights, const float *bias0, const float *table, const int32_t *offsets_host, float S, uint32_t H,
                            float bound, float density_scale, int zero_deform, float *sigmas, float *rgbs, float *deform, void *stream) {
    return sdn_int::field_forward_checked(2, {.xyzs = xyzs, .dirs = dirs, .live_idx = live_idx, .live_count = live_count, .M = M, .weights = weights,
                                              .bias0 = bias0, .table = table, .offsets_host = offsets_host, .S = S, .H = H, .bound = bound,
                                              .density_scale = density_scale, .zero_deform = zero_deform ? 1 : 0, .sigmas = sigmas, .rgbs = rgbs,
                                              .deform = deform},
                                          stream);
}

}  // extern "C"
