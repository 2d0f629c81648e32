// Persistent two-set ("ping-pong") form of the fused field kernel (included by field.hip inside its anonymous namespace; the same stages
// of field_f16_net.h, same packed weights, same QUAD table -- outputs bit-identical to k_field_f16).
//
// Why: k_field_f16 gives every wave the whole chain  point -> freq features -> 7 wide layers -> grid gathers -> small nets  and lets
// two workgroups per CU overlap by chance.  Its in-kernel stamps (profiles/r04_field_phase_stamps_*.jsonl) show a workgroup spending
// 40 % of its life in the wide layers -- where its matrix pipes are saturated -- and the rest in phases that use no matrix pipe at all
// (gather latency, encoder arithmetic, launch / load prologue).  Here the overlap is BUILT IN: one workgroup of 16 waves per CU (4 per
// SIMD) is two SETS of 8 waves that alternate roles every PERIOD of 7 barrier-separated slots:
//     set in role X:  slot 0 = layer D0 (16 MFMAs per wave), slots 1..6 = layers D1..D6 (32 MFMAs each) of its tile;
//     set in role Y:  the same 7 slots carry the vector-side work of its tiles in 7 chunks (table at y_period).
// A wave's life is  head(t0) X(t0) Y(tail t0, head t1) X(t1) ...  with set 1 one period behind set 0, so in every period each SIMD
// holds two waves streaming MFMAs and two waves doing encoder arithmetic / waiting on gathers -- the two sides of the kernel run
// beside each other by construction instead of by the luck of the dispatch order.  The workgroup is persistent: it walks the tiles
// blockIdx.x, blockIdx.x + G, ... (tile = 256 points = one set's 8 waves x 32), dealt to its two sets in turn, so weights D0 and the tail stage
// (D7 | S0 | S1 | C0 | C1 | C2) are loaded into LDS ONCE per workgroup and stay; D1..D6 stream through a ring of three 32-KiB buffers
// two uses ahead (the X set issues them between its MFMAs, counted vmcnt).  LDS: 48 KiB resident + 96 KiB ring + 4 KiB of bias rows
// (the frames' time-encoding contributions, D0's initial accumulators) + 8 KiB of per-wave point records.
//
// Slot protocol (all 16 waves pass the same 7 barriers per period, whatever their role):
//   use n = 6 (X period) + (slot - 1) of the D-stream reads ring n % 3 -- 6 uses per period, so the ring position of a slot is static:
//   slot l reads ring (l - 1) % 3 and refills ring (l + 1) % 3 with the stage of use n + 2 (D(l+2) for l <= 4, D1 / D2 again for
//   l = 5 / 6: the next X period's first uses -- after the workgroup's last X period nobody reads them), whose previous content
//   (use n - 1) every wave finished reading before the barrier that opened slot l.  An X wave ends slot l with vmcnt(4): its pieces
//   of use n + 1 have landed, the four it just issued stay in flight across the barrier.  When the roles swap, the pieces a wave issued
//   in slot 6 are waited for at the start of its chunk 0 (vmcnt(0)), i.e. before the barrier that opens the slot that reads them.
//
// Registers: 16 waves per CU leave 128 per lane.  X keeps the layer's 8 operand fragments, the 8 it produces, ONE accumulator tile and a
// two-deep fragment ring (88); everything a tile needs behind its wide layers (point, slot, frame) waits in LDS, not in registers.

// One 1-KiB refill piece, global -> LDS, as an asm statement hipcc does not count: lane l moves 16 bytes from gbase + 16 l to LDS byte
// address lds_dst + 16 l (saddr form: uniform 64-bit base in SGPRs + one shared 32-bit lane offset, no per-piece address registers).
// Hidden from the compiler's s_waitcnt bookkeeping on purpose (cdna_hip_programming.md, "When it pays"): hipcc would otherwise put a
// vmcnt(0) in front of every LDS read it cannot prove disjoint from the pending direct-to-LDS write and in front of every barrier's
// fence; the protocol's own counted waits are the `s_waitcnt vmcnt(N)` statements of x_period / y_period.  (A wait hipcc emits for a
// load of its own only ever waits for MORE than it intended: the counter completes in order and these pieces add to it.)
__device__ __forceinline__ void pp_piece(const unsigned char *gbase, uint32_t lds_dst, uint32_t lane16) {
    unsigned keep;
    lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);   // (wave-uniform by construction; makes the "s" constraint hold whatever register class
                                                          //  the compiler computed it in -- it only feeds the s_mov_b32 to m0, an SALU read)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane16), "s"(lds_dst), "s"(gbase) : "memory");
}
__device__ __forceinline__ uint32_t pp_lds_addr(const void *shared_ptr) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)shared_ptr;
}

#ifdef SDN_STAMPS
// Diagnostic build only: shader-clock stamp at the END of every slot (just before its barrier) for waves 0 (set 0) and 8 (set 1) of the
// first 256 workgroups: g_pp_stamps[(2 wg + set) * 128 + k], k = 0: kernel entry, 1: resident weights landed, 2 + 7 period + slot.
__device__ unsigned long long g_pp_stamps[256 * 2 * 128];
#define PPSTAMP() do { if (pp_stamp_on && pp_stamp_k < 128u) { pp_stamp_slot[pp_stamp_k] = __builtin_amdgcn_s_memtime(); } pp_stamp_k++; } while (0)
#else
#define PPSTAMP() ((void)0)
#endif

constexpr int kPPWaves = 16;
constexpr int kPPSetWaves = 8;
constexpr uint32_t kPPTile = 32u * kPPSetWaves;          // points per set tile
constexpr uint32_t kPPMaxFrames = 8;                     // bias rows kept in LDS (launches with more frames take k_field_f16)

// One wide layer, M-tile outer: the KS MFMAs of output tile mt run back to back into one accumulator tile, which is then converted
// (fp16 rounding + ReLU) into operand fragments 2 mt, 2 mt + 1 of the next layer -- while the SIMD's other X wave streams its MFMAs.
//   frag(blk) reads A fragment `blk` of the layer ((mt, ks) order = block order of the packed weights); piece(k) issues this wave's k-th
//   refill piece (or nothing); init(mt) supplies the initial accumulator.
template <int KS, int LA, int PIECES, bool PIN, typename Frag, typename Piece, typename Init>
__device__ __forceinline__ void pp_wide_layer(const half8 (&in)[8], half8 (&out)[8], Frag frag, Piece piece, Init init) {
    constexpr int N = 4 * KS;
    half8 ring[LA];
    #pragma unroll
    for (int j = 0; j < LA; j++) ring[j] = frag(j);
    #pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        f32x16 acc = init(mt);
        #pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const int i = mt * KS + ks;
            const half8 a = ring[i % LA];
            if (i + LA < N) ring[i % LA] = frag(i + LA);
            if (PIECES > 0 && (i % (N / (PIECES > 0 ? PIECES : 1))) == 1) piece(i / (N / (PIECES > 0 ? PIECES : 1)));
            acc = mfma(a, in[ks], acc);
        }
        acc_to_frags<true>(acc, out[2 * mt], out[2 * mt + 1]);
    }
    // pin the read / MFMA interleave (left alone, the scheduler hoists a dozen fragment reads to the top of the layer -- 48 registers the
    // 128-register budget does not have: spills, and a scratch reload drains vmcnt, i.e. the refill that is meant to stay in flight):
    // LA reads, then MFMA / read alternating; the conversions' VALU instructions and the refill pieces are left to fill the gaps
    if constexpr (PIN) {
        __builtin_amdgcn_sched_group_barrier(0x100, LA, 0);
        #pragma unroll
        for (int i = 0; i < N - LA; i++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, LA, 0);
    }
}

__global__ void __launch_bounds__(64 * kPPWaves) k_field_pp_f16(FieldArgs P, TiledLevels lv) {
    // Separate arrays, every access names its array at compile time (see k_field_f16).
    __shared__ __attribute__((aligned(4096))) uint4 s_lv[16][2];
    __shared__ __attribute__((aligned(16))) unsigned char s_d0[16 * 1024];
    __shared__ __attribute__((aligned(16))) unsigned char s_tail[kStageBytes];
    __shared__ __attribute__((aligned(16))) unsigned char s_r0[kStageBytes];
    __shared__ __attribute__((aligned(16))) unsigned char s_r1[kStageBytes];
    __shared__ __attribute__((aligned(16))) unsigned char s_r2[kStageBytes];
    __shared__ __attribute__((aligned(16))) uint4 s_pt[kPPWaves][32];          // per wave and point: {x0, x1, x2, slot | frame << 28}, kept across the wave's X period
    __shared__ __attribute__((aligned(16))) float s_bias[kPPMaxFrames][128];  // time-encoding bias rows of the launch's frames (D0's initial accumulators)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t set = wave >> 3, wv = wave & 7u;
#ifdef SDN_STAMPS
    const bool pp_stamp_on = wv == 0u && lane == 0u && blockIdx.x < 256u;
    unsigned long long *pp_stamp_slot = g_pp_stamps + ((size_t)blockIdx.x * 2 + set) * 128;
    uint32_t pp_stamp_k = 0;
    PPSTAMP();
#endif
    levels_to_lds(s_lv, lv);
    const uint32_t count = live_points(P);
    const uint32_t n_tiles = (count + kPPTile - 1u) / kPPTile;
    if (blockIdx.x >= n_tiles) return;                                   // workgroup-uniform, before any barrier
    // G workgroups share the tiles (the launch is sized before the live count is known).  Optional (pp_soft bit 31 clear): the fewest
    // that need no more rounds than the caller's soft count would -- unless every launched workgroup together saves a whole round
    uint32_t G = gridDim.x;
    if (!(P.pp_soft >> 31)) {
        const uint32_t want = P.pp_soft & 0x3FFFFFFFu;
        const uint32_t soft = (want && want < G) ? want : G;
        const uint32_t r_soft = (n_tiles + soft - 1u) / soft, r_hard = (n_tiles + G - 1u) / G;
        const uint32_t r = (r_hard < r_soft && !(P.pp_soft & 0x40000000u)) ? r_hard : r_soft;    // (bit 30: never more than `soft`)
        G = (n_tiles + r - 1u) / r;
    }
    if (blockIdx.x >= G) return;
    // tiles blockIdx.x, blockIdx.x + G, ... of this workgroup go to its two sets in turn: set 0 takes the even-numbered ones.  The
    // workgroup lasts cnt + 2 periods whatever the parity of cnt (a set without a tile left idles through the barriers)
    const uint32_t cnt = (n_tiles - blockIdx.x + G - 1u) / G;            // >= 1
    const uint32_t nq = set == 0u ? (cnt + 1u) >> 1 : cnt >> 1;          // tiles of this set

    // resident weights (D0, tail stage) and the first two uses of the stream (D1 -> ring 0, D2 -> ring 1): 112 KiB, 7 pieces per wave
    const uint32_t lane16 = lane << 4;
    {
        const unsigned char *w = P.weights;
        auto put = [&](const unsigned char *g, const void *lds, uint32_t n_kib) {
            const uint32_t dst = pp_lds_addr(lds);
            for (uint32_t c = wave; c < n_kib; c += (uint32_t)kPPWaves) pp_piece(g + c * 1024u, dst + c * 1024u, lane16);
        };
        put(w + (size_t)kBlkD0 * 1024, s_d0, 16u);
        put(w + (size_t)kBlkD7 * 1024, s_tail, 32u);
        put(w + (size_t)kBlkD1 * 1024, s_r0, 32u);
        put(w + (size_t)(kBlkD1 + 32) * 1024, s_r1, 32u);
    }
    {
        const uint32_t nf = P.n_frames ? (P.n_frames < kPPMaxFrames ? P.n_frames : kPPMaxFrames) : 1u;
        for (uint32_t k = threadIdx.x; k < 128u * nf; k += 64u * kPPWaves) s_bias[k >> 7][k & 127u] = P.bias0[k];
    }
    const uint32_t n = lane & 31u, h = lane >> 5;
    const unsigned char *__restrict__ table_bytes = reinterpret_cast<const unsigned char *>(P.table);

    half8 bfA[8], bfB[8];        // operand fragments, alternating between layers
    #pragma unroll
    for (int j = 0; j < 8; j++) { bfA[j] = (half8){0, 0, 0, 0, 0, 0, 0, 0}; bfB[j] = bfA[j]; }

    // The slot barrier is the bare instruction between two compiler-level memory barriers, NOT __syncthreads(): that one's workgroup
    // fence makes hipcc wait for vmcnt(0) whenever direct-to-LDS loads are pending, i.e. it would drain at every barrier the very
    // refill that is meant to stay in flight across two of them.  What the protocol needs is waited for explicitly: lgkmcnt(0) (this
    // wave's LDS reads and writes of the slot are done) in front, the counted vmcnt of the X waves where they refill.
    auto slot_barrier = [&]() {
        PPSTAMP();
        __builtin_amdgcn_sched_barrier(0);            // a slot's instructions stay in their slot
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    auto idle_period = [&]() {
        #pragma unroll 1
        for (int s = 0; s < 7; s++) slot_barrier();
    };

    // ---- X: the seven wide layers of the tile whose D0 operand is in bfA[0..3]; leaves D6's output in bfB ----
    auto x_period = [&]() {
        __builtin_amdgcn_s_setprio(1);
        const unsigned char *wsrc = P.weights;
        auto no_piece = [&](int) {};
        auto zero_init = [&](int) { return zero_tile(); };
        // slot 0: D0 (4 k-steps), resident buffer, nothing to refill; from the bias row of the point's frame
        f32x16 bias[4];
        bias_rows(s_bias[s_pt[wave][n].w >> 28], h, bias);
        auto bias_init = [&](int mt) { return bias[mt]; };
        pp_wide_layer<4, 2, 0, false>(bfA, bfB, [&](int blk) { return lds_frag(s_d0, blk, lane); }, no_piece, bias_init);
        slot_barrier();
        // slots 1..6: layer l reads ring (l - 1) % 3 and refills ring (l + 1) % 3 with the stage two uses ahead
        auto hidden = [&](auto l_c, const unsigned char *cur, unsigned char *dst, const half8 (&in)[8], half8 (&out)[8]) __attribute__((always_inline)) {
            constexpr int l = decltype(l_c)::value;
            constexpr int next_layer = (l + 1) % 6 + 1;                    // D(l+2) for l <= 4, D1 / D2 of the next X period for l = 5 / 6
            // this wave's pieces of the stage: wv, wv + 8, wv + 16, wv + 24 (KiB)
            const unsigned char *src = wsrc + (size_t)(kBlkD1 + (next_layer - 1) * 32) * 1024 + wv * 1024u;
            const uint32_t dst_lds = pp_lds_addr(dst) + wv * 1024u;
            pp_wide_layer<8, 2, 4, true>(in, out, [&](int blk) { return lds_frag(cur, blk, lane); },
                                   [&](int k) { pp_piece(src + k * (kPPSetWaves * 1024), dst_lds + (uint32_t)k * (kPPSetWaves * 1024u), lane16); }, zero_init);
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            slot_barrier();
        };
        hidden(std::integral_constant<int, 1>{}, s_r0, s_r2, bfB, bfA);
        hidden(std::integral_constant<int, 2>{}, s_r1, s_r0, bfA, bfB);
        hidden(std::integral_constant<int, 3>{}, s_r2, s_r1, bfB, bfA);
        hidden(std::integral_constant<int, 4>{}, s_r0, s_r2, bfA, bfB);
        hidden(std::integral_constant<int, 5>{}, s_r1, s_r0, bfB, bfA);
        hidden(std::integral_constant<int, 6>{}, s_r2, s_r1, bfA, bfB);
        __builtin_amdgcn_s_setprio(0);
    };

    // ---- Y: tail of the tile whose D6 outputs are in bfB (if has_tail), head of `next_tile` (if has_head), in 7 chunks ----
    //   chunk  tail of the finished tile                                             head of the next tile            vector instr. / MFMAs
    //     0    D7 + deformation, dirs load                                           slot index load                       ~25 /  8
    //     1    cells + gathers of levels 0-3, SH basis                               coordinates + frame load             ~170
    //     2    interpolation of levels 0-1, cells + gathers of levels 4-5                                                 ~150
    //     3    interpolation of levels 2-4, cells + gathers of levels 6-7                                                 ~195
    //     4    interpolation of levels 5-7, sigma net                                                                     ~195 /  8
    //     5    colour net, first two layers                                          base sines / cosines                 ~155 / 12
    //     6    colour net's last layer, stores                                       angle doubling, operand packing      ~175 /  4
    // (slot 0 is the X set's short one -- D0, 16 MFMAs -- and so is chunk 0; the chunks' MFMAs add to the X set's 64 per SIMD and slot)
    // A slot lasts as long as the longer of its layer and its chunk; every load is consumed at least one chunk after it was issued; the
    // 16 gathers of a point are spread over four chunks (a CU takes ~1 divergent lane address per cycle: 8 waves x 6 gathers x 64 lanes
    // are one slot's worth of that unit) and at most five levels' blocks are in registers at a time.  The chunks' own MFMAs (D7, sigma
    // net, colour net: dependent chains) run at a HIGHER priority than the X set's streams -- the X waves wait for this set at every
    // barrier anyway.  The stages themselves are field_f16_net.h's, the ones k_field_f16 calls.
    // (has_tail / has_head are COMPILE-TIME: with run-time flags every chunk is a conditional block of its own and the compiler sinks a
    //  chunk's arithmetic into the later block that first uses the result -- level 0's sixteen products waited, spilled, for chunk 5)
    // Pins (`asm volatile("" : "+v"(..))` behind a stage): a pure value first used chunks later is otherwise placed next to that use when
    // the block is linearised, and what it was computed from waits for it in scratch.
    auto pin = [&](half8 &f) {
        u32x4 w = __builtin_bit_cast(u32x4, f);
        asm volatile("" : "+v"(w));
        f = __builtin_bit_cast(half8, w);
    };
    auto y_period = [&](auto has_tail_c, uint32_t tail_tile, auto has_head_c, uint32_t head_tile) __attribute__((always_inline)) {
        constexpr bool has_tail = decltype(has_tail_c)::value, has_head = decltype(has_head_c)::value;
        float u[3] = {0, 0, 0};
        uint32_t keep = 0xFFFFFFFFu;     // 0 for a point outside [0, 1]^3: its rows collapse to row 0 and its features are zeroed (kernel_grid's early out)
        float fr[8][3];
        uint4 quads[8][2];
        uint32_t gfw[2][4];
        half8 cf[2], c2f[4];
        float sigma = 0;
        float d0 = 0, d1 = 0, d2 = 0;
        uint32_t tail_p = 0;
        uint32_t head_p = 0, head_frame = 0;
        float hx0 = 0, hx1 = 0, hx2 = 0;
        float sv0[3] = {0, 0, 0}, cv0[3] = {0, 0, 0};
        // cells of levels [first, last) of the lane-half and their gathers (QUAD table: the z and z + 1 blocks of a cell)
        auto cells_and_gathers = [&](int first, int last) {
            #pragma unroll
            for (int li = first; li < last; li++) {
                const uint4 k0 = s_lv[8 * h + li][0], k1 = s_lv[8 * h + li][1];
                const uint32_t base = level_cell(k0, k1, u, fr[li], false) & keep;
                #pragma unroll
                for (int d = 0; d < 3; d++) asm volatile("" : "+v"(fr[li][d]));
                __builtin_memcpy(&quads[li][0], table_bytes + ((k0.x + (base & k1.x)) << 4), 16);
                __builtin_memcpy(&quads[li][1], table_bytes + ((k0.x + ((base + k0.z) & k1.x)) << 4), 16);
                __builtin_amdgcn_sched_barrier(0);   // level by level: interleaving the levels' index arithmetic only lengthens live ranges (spills at 128 registers)
            }
        };
        auto interp_levels = [&](int first, int last) {
            #pragma unroll
            for (int li = first; li < last; li++) {
                uint32_t feat = interp_corners(fr[li], [&](uint32_t idx) { return quad_corner(quads[li], idx); }) & keep;
                asm volatile("" : "+v"(feat));
                gfw[li >> 2][li & 3] = feat;
                __builtin_amdgcn_sched_barrier(0);   // (as above: one level's 8 weights and 16 products at a time)
            }
        };
        // chunk 0.  The pieces this wave issued in slot 6 of its X period are waited for here (vmcnt(0) in front of the chunk's own loads).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (has_head) {
            const uint32_t i = head_tile * kPPTile + wv * 32u + n;
            const uint32_t ii = i < count ? i : (count - 1u);          // idle lanes recompute the last point and store nothing
            head_p = P.live_idx ? P.live_idx[ii] : ii;
        }
        if (has_tail) {
            const uint4 rec = s_pt[wave][n];
            tail_p = rec.w & 0x0FFFFFFFu;
            const uint32_t zero_def = (P.zero_deform >> (rec.w >> 28)) & 1u;
            d0 = P.dirs[(size_t)tail_p * 3]; d1 = P.dirs[(size_t)tail_p * 3 + 1]; d2 = P.dirs[(size_t)tail_p * 3 + 2];
            __builtin_amdgcn_s_setprio(3);
            const f32x16 o = deform_d7(s_tail, bfB, lane);
            __builtin_amdgcn_s_setprio(0);
            grid_coords(o, lane, __uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z), zero_def, P, u);
            #pragma unroll
            for (int c = 0; c < 3; c++) asm volatile("" : "+v"(u[c]));
            keep = out_of_grid(u) ? 0u : 0xFFFFFFFFu;
            asm volatile("" : "+v"(keep));
        }
        slot_barrier();
        // chunk 1
        if (has_head) {
            hx0 = P.xyzs[(size_t)head_p * 3]; hx1 = P.xyzs[(size_t)head_p * 3 + 1]; hx2 = P.xyzs[(size_t)head_p * 3 + 2];
            head_frame = P.slot_frame ? P.slot_frame[head_p] : 0u;
        }
        if (has_tail) {
            cells_and_gathers(0, 4);
            cf[1] = sh_operand(d0, d1, d2, h);
            pin(cf[1]);
        }
        slot_barrier();
        // chunk 2
        if (has_tail) {
            interp_levels(0, 2);
            cells_and_gathers(4, 6);
        }
        slot_barrier();
        // chunk 3
        if (has_tail) {
            interp_levels(2, 5);
            cells_and_gathers(6, 8);
        }
        slot_barrier();
        // chunk 4
        if (has_tail) {
            interp_levels(5, 8);
            half8 gf[2];
            grid_operand(gfw, gf);
            __builtin_amdgcn_s_setprio(3);
            const f32x16 hv = sigma_net(s_tail, gf, lane);
            __builtin_amdgcn_s_setprio(0);
            sigma = density(hv, P.density_scale);
            asm volatile("" : "+v"(sigma));
            cf[0] = geo_operand(hv);
            pin(cf[0]);
        }
        slot_barrier();
        // chunk 5
        if (has_tail) {
            f32x16 c1[2];
            __builtin_amdgcn_s_setprio(3);
            colour_hidden(s_tail, cf, lane, c1);
            __builtin_amdgcn_s_setprio(0);
            relu_frags(c1, c2f);
            #pragma unroll
            for (int k = 0; k < 4; k++) pin(c2f[k]);
        }
        if (has_head) {      // (the polynomial pair: a third of the frequency features' work)
            freq_base(hx0, hx1, hx2, h, sv0, cv0);
            #pragma unroll
            for (int dd = 0; dd < 3; dd++) asm volatile("" : "+v"(sv0[dd]), "+v"(cv0[dd]));
        }
        slot_barrier();
        // chunk 6
        if (has_tail) {
            __builtin_amdgcn_s_setprio(3);
            const f32x16 co = colour_out(s_tail, c2f, lane);
            __builtin_amdgcn_s_setprio(0);
            if (h == 0 && tail_tile * kPPTile + wv * 32u + n < count) store_sigma_rgb(P, tail_p, sigma, co);
        }
        if (has_head) {      // the next tile's record for its X period and tail, and its D0 operand
            if (h == 0) s_pt[wave][n] = make_uint4(__float_as_uint(hx0), __float_as_uint(hx1), __float_as_uint(hx2), head_p | (head_frame << 28));
            freq_operand(hx0, hx1, hx2, h, sv0, cv0, bfA);
        }
        slot_barrier();
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                  // resident weights, D1, D2, the bias rows and the level constants are in LDS
    PPSTAMP();
    if (set == 1u) idle_period();                     // set 1 runs one period behind set 0
    const uint32_t first_tile = blockIdx.x + set * G, tile_step = 2u * G;
    constexpr std::integral_constant<bool, true> yes{};
    constexpr std::integral_constant<bool, false> no{};
    if (nq) {
        y_period(no, 0u, yes, first_tile);
        #pragma unroll 1
        for (uint32_t j = 0; j + 1u < nq; j++) {
            const uint32_t tile = first_tile + j * tile_step;
            x_period();
            y_period(yes, tile, yes, tile + tile_step);
        }
        x_period();
        y_period(yes, first_tile + (nq - 1u) * tile_step, no, 0u);
    }
    // periods so far: set 0 -> 2 nq + 1, set 1 -> 1 + (nq ? 2 nq + 1 : 0); the workgroup's total is cnt + 2
    {
        const uint32_t done = (set == 0u ? 0u : 1u) + (nq ? 2u * nq + 1u : 0u);
        #pragma unroll 1
        for (uint32_t k = done; k < cnt + 2u; k++) idle_period();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the last X period's look-ahead pieces: nobody reads them, but they must have landed before the LDS is handed on)
}
