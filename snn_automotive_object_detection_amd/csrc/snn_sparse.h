// Structured-sparse matrix cores for the SPARSE period planes of the RPN's shared 3x3 convolution and the detector's fc6 (rounds 4-5).  Included by snn_kernels.hip
// after snn_bf16x3.h (Gemm3-style staging helpers, f2bf / bf2f, G3_SWZ).
//
// With period planes (snn_common.h) a conv row tile holds Tc row groups u_n = W e_n, and for n >= 3 the planes are nearly empty
// (densities 0.039, 0.019, 0.011, 0.007, 0.005 on the bench's pyramid) - yet each costs a full dense MFMA pass.  gfx950's
// v_smfmac_f32_16x16x64_bf16 multiplies an A operand with at most TWO non-zeros per four consecutive k at 64 k per instruction:
// 1.82 x the dense rate sustained in this kernel's LDS-fed shape (tools/sparse_probe.hip, profiles/r4_sparse_probe.txt).  So:
//   * planes e_1, e_2 (densities 0.25 / 0.12: nibbles with three spikes are common) stay on the dense v_mfma_f32_16x16x32_bf16;
//   * planes e_n, n >= 3, are COMPRESSED (by the encoder launches themselves since round 5 - snn_encode.h -, else by k_compress_planes): per 16 k of a row 8 value slots (occupied or not: the value is 1.0) +
//     8 two-bit positions.  The A fragment of a lane is table[occupancy byte] - the dense kernels' byte -> 8 bf16 table - plus 16 index
//     bits; operand layout and encoding were established on the hardware (sparse_probe A1 / A4);
//   * a nibble with three or four spikes of ONE period (rare: ~0.16 per position over the five sparse planes) keeps its first two in
//     the compressed plane; the others go into a SECONDARY compressed plane (two more value slots per nibble, at the constant
//     positions 2 and 3 - where a third / fourth spike can only be: one more dword per row and step, all four bits of a nibble
//     covered).  A wave whose 16 rows have an empty secondary block in a 64-k step (the rule: ~98 % of the (M-tile, step) pairs on the
//     bench's pyramid) skips it; otherwise it issues the structured-sparse instruction a second time for
//     that M-tile, right behind the step's other products.  Exactness is unchanged: every product is spike x (hi + mid + lo), fp32 sums
//     in a fixed order.  (Until late in round 4 the third and fourth spikes were per-tile fix-up lists applied in the epilogue, with a
//     dense fallback launch for inputs that overflowed them: 3.7 % of the conv launch, and a slow path for adversarial inputs.  The
//     secondary plane needs neither lists nor fallback, and reads its entries through the same 3x3 tap walk as everything else.)
//
// Row tile = pb positions x Tc planes as M-tiles of 16 rows (plane t, positions 16 j .. 16 j + 15), assigned to M-tile SLOTS of the
// waves (table in SparseConvArgs, dense ones first); a wave's K loop is instantiated for its (dense, sparse) counts.  K runs in steps
// of 64 (two 32-deep chunks of the packed weights, whose LDS image is the dense kernels'); ring = two step slots, one barrier per step,
// two work-groups per CU in every shape.  Shapes (k_gemm_lif_sparse<CONV, WN, FAT>; the launcher's planner picks, snn_kernels.hip):
//   8-wave (512 threads, 128 registers)    8 x 1 waves x 4 slots (conv) or 4 x 2 x 6 (linear layers); LIF through a tile image in LDS,
//                                          straight-line instances T = 5 .. 16, general (run-time) form for the linear layers beyond
//   FAT (round 5; 256 threads, <= 256 regs) four waves with twice the slots: half (conv 2 x 2: a quarter) of the weight-fragment reads per
//                                          matrix instruction, fragments requested two groups ahead.  Linear layers: 2 x 2 x 12.  Conv:
//                                          4 x 1 x 8 for T = 7 .. 9 (tiles of 64 positions), 2 x 2 x 16 for T = 12 .. 16 (tiles of 32) - every
//                                          (row-)wave holds ALL planes of its own 16 positions, so the LIF runs in REGISTERS (sp_lif_regs):
//                                          no tile image, no epilogue barrier; also for fc6 where a row-wave holds all planes of its RoIs
// All shapes give the same bits: every accumulator sees the same matrix instructions in the same order, and the LIF forms are the same
// operations in the same order (tests/test_gpu_sparse.py compares the spike planes in the workspace).
#pragma once

typedef __bf16 bfv8 __attribute__((ext_vector_type(8)));
typedef __bf16 bfv16 __attribute__((ext_vector_type(16)));

#define SP_MT 4                                     // M-tile slots per wave on the 8 x 1 wave grid (all waves span the 64 columns)
#define SP_MT2 6                                    // ... per ROW-wave on the 4 x 2 grid (two waves of 32 columns share a row-wave's slots)
#define SP_MT2_FAT 12                               // ... per row-wave of the FAT shape (linear layers): 2 x 2 waves of up to 256 registers, 32 columns per wave
#define SP_MT_FAT 8                                 // ... per wave of the FAT conv, T <= 9: 4 waves x all 64 columns, every wave ALL planes of its own 16 positions (register LIF)
#define SP_MT2_FAT_CONV 16                          // ... per row-wave of the FAT conv, T = 12 .. 16: 2 x 2 waves, a row-wave = all planes of its 16 positions, 32 columns per wave
#define SP_MTMAX 16
#define SP_ROWS (8 * SP_MT * 16)                    // physical tile rows (512; 4 x 6 x 16 = 384 on the 4 x 2 grid)
// (SP_A_ARR and sp_nibble_code live in snn_common.h: the RPN encoder writes the same compressed layout)
#define SP_A_BYTES (SP_A_ARR * SP_ROWS * 4)
#define SP_B_BYTES (2 * 3 * 64 * G3_ROWB)           // two chunks x three weight planes x 64 columns
#define SP_SLOT (SP_A_BYTES + SP_B_BYTES)           // one 64-k step: 32 KB
#define SP_LDS (G3_LUT_BYTES + 2 * SP_SLOT)         // 68 KB: two work-groups per CU
#ifdef SNN_EXP_SP_NO_BREAD                            // (timing experiment, see the K loop)
#define SNN_EXP_BSEL(g) 0
#else
#define SNN_EXP_BSEL(g) (g)
#endif
#ifndef SP_PRE_A
#define SP_PRE_A 1
#endif
#ifndef SP_PRE_B
#define SP_PRE_B 0                                  // (1: FAT shapes request a step's first weight fragments right behind the previous step's barrier -
                                                    // measured 0.9 % / 1.2 % SLOWER on the conv / fc6, profiles/r5_preb_ab.txt: off)
#endif
#ifndef SP_SEC_LATE
#define SP_SEC_LATE 1
#endif
#define SP_PITCH 36                                 // epilogue tile image: 32 columns + 4 floats of padding per row

struct SparseConvArgs {
    const uint32_t* enc;         // raw period planes, word-major [Tc][Cw][Pe] (zero halo); the dense planes are read from here
    const uint32_t* cmp;         // compressed planes [Tc - nd][Cw / 2][4][Pe]
    const uint16_t* wpk;         // [3][Kc][Np][32] bf16
    uint32_t* spk;               // spike planes out
    unsigned long long* tl;      // SNN_EXP_TIMELINE builds: 8 stamps per work-group
    // spike-rate side output (nullable; zeroed by the caller): spikes per row - RoI, or position (the conv's launcher sums them per
    // (level, image) afterwards: k_sum_pos_counts).  Integer atomics, one per (row, 32 columns): order-independent.
    uint32_t* cnt_row;
    unsigned long long plane_elems, spk_stride;
    unsigned int Pe;             // padded rows of a word plane
    int M, Kc, Np, Cw, n_blocks, n_tiles, n_levels;
    int T, Tc, nd, pb, q, out_split;
    signed char mt_plane[8][SP_MTMAX];   // plane of the row-wave's M-tile slot (-1: unused); dense planes (< nd) first
    unsigned char mt_j[8][SP_MTMAX];     // position block of the slot: local positions 16 j ..
    unsigned char w_nd[8], w_ns[8];      // dense / sparse M-tiles of the row-wave
    int xcd_contig, xcd_cpx;             // block order, as Gemm3Args
    // epi_general != 0: the LIF epilogue's general form (run-time T and window: the current of step t < Tc is the sum of the row groups in
    // div[t], ascending) - every (T, window) without a straight-line instance: linear layers at T > 16 and in spike-rate mode (window T - 1)
    int lif_regs;                // FAT shapes: every (row-)wave holds ALL planes of its own block of 16 positions / RoIs (slot s = plane s) and this
                                 // (T, window) has a register-LIF instance: the LIF runs in registers (sp_lif_regs), no tile image (host: sparse_plan_lif_regs)
    int epi_general;
    uint32_t div[SNN_MAX_STEPS];
    NeuronP p;
    ConvLevelDev lv[SNN_MAX_LEVELS];
    const int* gate;             // conv route, fc6 route (null everywhere else): as Gemm3Args.gate - the launch leaves at entry unless *gate == gate_want
    int gate_want;
};

// Reduction-index permutation of a linear layer's period planes (the detector's fc6).  The flattened RoI features run (channel, bin):
// k = c * S + s, so four consecutive k are four neighbouring BINS of one channel - strongly correlated values, hence often the same
// period: three or four spikes per nibble would be the rule in the sparse planes, not the exception.  With k' = s * C + c four consecutive
// k' are four CHANNELS at one bin (independent, as in the RPN's conv, whose reduction index is tap * C + channel).  The encoders keep
// writing planes in the reference's order; this kernel transposes the bits of every (plane, RoI) row, and fc6's weights are packed in
// the same order (snn_pack_linear_weight_bf16x3_perm): the contraction is the same sum in another order.
// Block = (32 RoIs, plane); word-major planes [T][Dw][R] in and out.  Thread task = (RoI, block of 32 channels): the channels' 32 x S bits are
// S words of the row, i.e. a 32 x S bit matrix (row = channel: S consecutive bits at bit offset j S) that leaves as its transpose (S words
// of 32 channel bits).  With S a compile-time constant: each channel's bits are cut out with two funnel shifts (v_alignbit) into a 32-bit
// and an (S - 32)-bit part, and the two 32 x 32 bit matrices are transposed in registers by the five-stage butterfly (Hacker's Delight
// 7-3, LSB-first form): ~1100 operations per task.  (First version: every bit gathered from LDS, 82 us for 2000 RoIs x 10 planes; second:
// one v_bfe + v_lshl_or per bit, 3136 operations per task, 38 us.)  Stores: 32 consecutive RoIs of one word.
__device__ __forceinline__ void bit_transpose32(uint32_t (&a)[32]) {          // out[s] bit j = in[j] bit s
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int jj = 16 >> st;
        const uint32_t m = st == 0 ? 0x0000ffffu : st == 1 ? 0x00ff00ffu : st == 2 ? 0x0f0f0f0fu : st == 3 ? 0x33333333u : 0x55555555u;
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (!(k & jj)) {
                const uint32_t t = ((a[k] >> jj) ^ a[k + jj]) & m;
                a[k] ^= t << jj;
                a[k + jj] ^= t;
            }
    }
}

#define PERM_CB 8                                   // channel blocks (of 32 channels) per pass: one per wave; LDS = PERM_CB * S * 33 words (51.7 KB at S = 49)
template <int S>
__global__ __launch_bounds__(256) void k_permute_planes(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int Dw, int R, int C) {
    static_assert(S > 32 && S <= 64, "two 32-column parts");
    __shared__ uint32_t pl[PERM_CB * S * 33];                 // [word of the pass][32 RoIs + 1]
    const int t = blockIdx.y, r0 = blockIdx.x * 32, rl = threadIdx.x & 31;
    const bool live = r0 + rl < R;
    const int cbn = C / 32;                                   // channel blocks = words per bin in the permuted order
    // passes of PERM_CB channel blocks (any channel count: round 5 - the whole row in LDS capped C at 320)
    for (int cb0 = 0; cb0 < cbn; cb0 += PERM_CB) {
        const int nw = min(PERM_CB, cbn - cb0) * S, wbase = cb0 * S;       // words [wbase, wbase + nw) of the row
        if (cb0) __syncthreads();
        // (the row's words are requested in batches of 7: one load in flight per thread made this kernel a chain of memory latencies)
        for (int w0 = threadIdx.x >> 5; w0 < nw; w0 += 8 * 7) {
            uint32_t v[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                const int w = w0 + 8 * i;
                v[i] = (live && w < nw) ? in[((size_t)t * Dw + wbase + w) * R + r0 + rl] : 0u;
            }
#pragma unroll
            for (int i = 0; i < 7; ++i)
                if (w0 + 8 * i < nw) pl[(w0 + 8 * i) * 33 + rl] = v[i];
        }
        __syncthreads();
        const int cl = threadIdx.x >> 5, cb = cb0 + cl;       // one channel block per wave-half
        if (cb >= cbn) continue;
        uint32_t w[S + 1];
#pragma unroll
        for (int i = 0; i < S; ++i) w[i] = pl[(cl * S + i) * 33 + rl];          // bits [32 cb S, 32 (cb + 1) S) of the row: channel j at bit j S + s
        w[S] = 0u;
        uint32_t lo[32], hi[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int o = j * S, i = o >> 5, sh = o & 31;                        // compile-time after unrolling
            lo[j] = sh ? __builtin_amdgcn_alignbit(w[i + 1], w[i], sh) : w[i];
            hi[j] = (sh ? __builtin_amdgcn_alignbit(w[i + 2 <= S ? i + 2 : S], w[i + 1], sh) : w[i + 1]) & ((1u << (S - 32)) - 1u);
        }
        bit_transpose32(lo);
        bit_transpose32(hi);
        if (live) {
#pragma unroll
            for (int s = 0; s < S; ++s)
                out[((size_t)t * Dw + (size_t)s * cbn + cb) * R + r0 + rl] = s < 32 ? lo[s] : hi[s - 32];
        }
    }
}

struct CompressArgs {
    const uint32_t* enc;
    uint32_t* cmp;
    unsigned int Pe;
    int Cw, nd;
};

// thread = (row, 64-k step w2 = blockIdx.y, sparse plane ts = blockIdx.z); row = padded position (conv) or RoI (linear layer).
// Out: four dwords per (row, step): primary occupancy / indices 0-1 / indices 2-3, then the secondary plane's occupancy (the third and
// fourth spike of a nibble: zero almost everywhere).  A third spike can only sit at bit 2 or 3 of its nibble and a fourth at bit 3, so
// the secondary slots are (value = leftover bit 2, position 2), (value = leftover bit 3, position 3): constant indices, nothing stored.
__global__ __launch_bounds__(256) void k_compress_planes(const CompressArgs a) {
    __shared__ uint16_t code[256];
    code[threadIdx.x] = sp_byte_code(threadIdx.x);
    __syncthreads();
    const unsigned int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= a.Pe) return;
    const int w2 = blockIdx.y, ts = blockIdx.z, t = a.nd + ts;
    uint32_t c4[4];
    sp_compress_pair(a.enc[((size_t)t * a.Cw + 2 * w2) * a.Pe + row], a.enc[((size_t)t * a.Cw + 2 * w2 + 1) * a.Pe + row], code, c4);
    uint32_t* out = a.cmp + ((size_t)ts * (a.Cw / 2) + w2) * SP_A_ARR * a.Pe + row;
    const size_t Pe = a.Pe;
    out[0] = c4[0]; out[Pe] = c4[1]; out[2 * Pe] = c4[2];
    out[3 * Pe] = c4[3];
}

// ---- conv route (snn_rpn_head_forward_routed) ----
// k_compress_planes' counting twin: the same four dwords per (row, step), and the density statistic the route is decided on.
// BLOCK = 16 consecutive rows (aligned to 16 in the Pe padded rows of a word plane: a quarter of a wave here) x one 64-k step x one
// compressed plane; HIT = a block in which some row's secondary-occupancy dword is non-zero - an M-tile on which the sparse launch's
// centre tap issues its second pass.  One ballot per wave, one LDS add per wave with a hit, one integer atomic per work-group with a hit -
// exact and order-independent.  The atomics go to `nslots` counters (zeroed by the launcher) a cache line apart, picked by the block index:
// on a dense input nearly every work-group has a hit, and 27 000 atomics on ONE address cost 0.2 ms (profiles/route_crossover.txt); k_route_decide sums them.
#define ROUTE_SLOT_STRIDE 32                        // ints between two counters: 128 bytes
#define ROUTE_SLOTS_MAX 64
__global__ __launch_bounds__(256) void k_compress_count_planes(const CompressArgs a, int* __restrict__ slots, const int nslots, const unsigned int n_rows) {
    __shared__ uint16_t code[256];
    __shared__ int wg_hits;
    code[threadIdx.x] = sp_byte_code(threadIdx.x);
    if (threadIdx.x == 0) wg_hits = 0;
    __syncthreads();
    const unsigned int row = blockIdx.x * 256 + threadIdx.x;
    const int w2 = blockIdx.y, ts = blockIdx.z, t = a.nd + ts;
    uint32_t c4[4] = {0u, 0u, 0u, 0u};
    if (row < a.Pe) {
        sp_compress_pair(a.enc[((size_t)t * a.Cw + 2 * w2) * a.Pe + row], a.enc[((size_t)t * a.Cw + 2 * w2 + 1) * a.Pe + row], code, c4);
        uint32_t* out = a.cmp + ((size_t)ts * (a.Cw / 2) + w2) * SP_A_ARR * a.Pe + row;
        const size_t Pe = a.Pe;
        out[0] = c4[0]; out[Pe] = c4[1]; out[2 * Pe] = c4[2];
        out[3 * Pe] = c4[3];
    }
    const unsigned long long sec = __ballot(c4[3] != 0u && row < n_rows);        // (rows past Pe: zero; n_rows <= Pe: rows past it belong to no block)
    if ((threadIdx.x & 63) == 0 && sec) {
        int n = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) n += ((sec >> (16 * g)) & 0xffffull) != 0ull;
        atomicAdd(&wg_hits, n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_hits)
        atomicAdd(slots + (size_t)ROUTE_SLOT_STRIDE * ((blockIdx.x + 3u * blockIdx.y + 5u * blockIdx.z) % (unsigned)nslots), wg_hits);
}

// one wave: route_stat = {hits, blocks, route, 0}.  fixed >= 0: the route the host chose ({0, 0, fixed, 0}); fixed < 0: hits = the sum of the
// counters, and the decision - dense (1) iff hits > crossover x blocks, in fp32 as stated in snn_hip.h.  stat[2] is the gate word of the two
// conv launches.
__global__ __launch_bounds__(64) void k_route_decide(int* __restrict__ stat, const int* __restrict__ slots, int nslots, int blocks, float crossover, int fixed) {
    if (blockIdx.x) return;
    if (fixed >= 0) {
        if (threadIdx.x == 0) { stat[0] = 0; stat[1] = 0; stat[2] = fixed; stat[3] = 0; }
        return;
    }
    int hits = 0;
    for (int i = threadIdx.x; i < nslots; i += 64) hits += slots[(size_t)ROUTE_SLOT_STRIDE * i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hits += __shfl_xor(hits, off);
    if (threadIdx.x == 0) {
        stat[0] = hits; stat[1] = blocks;
        stat[2] = (float)hits > crossover * (float)blocks ? 1 : 0;
        stat[3] = 0;
    }
}

// LIF over T steps of NP independent neurons per lane from the period sums in the LDS tile image: the straight-line form of
// k_gemm_bf16x3's epilogue (period planes, v_leak = 0, no spike at step 0, conv window T - 1), same operations in the same order per
// neuron.  NP = 2: the recurrence is one dependent chain of ~6 operations per step; two of them interleaved fill each other's latencies
// (LIF part of an epilogue pass 3.9 -> see profiles/r4_sparse_timeline.txt).
// COUNT: also the spikes per position (low / high half of the ballot = even / odd position of the pair): scalar popcounts.
template <int TS, int D, int NP, bool COUNT>
__device__ __forceinline__ void sp_lif_fixed(const float* const (&src)[NP], const int group_stride, const NeuronP& p, uint32_t (&my0)[NP], uint32_t (&my1)[NP],
                                             uint32_t (&cnt_lo)[NP], uint32_t (&cnt_hi)[NP]) {
    constexpr int TCS = TS - D;                          // currents of steps 0 .. T - 1 - D (conv: D = 1; fc6: D = 2 - dead time steps)
    float ug[NP][TCS];
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
        for (int g = 0; g < TCS; ++g) ug[u][g] = src[u][(size_t)g * group_stride];
    float vv[NP], ii[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) { vv[u] = 0.0f; ii[u] = 0.0f; }
#pragma unroll
    for (int t = 0; t < TS; ++t) {
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            float c = 0.0f;
            if (t < TCS) {
                c = ug[u][0];
#pragma unroll
                for (int n = 2; n <= t + 1; ++n)
                    if ((t + 1) % n == 0) c = __fadd_rn(c, ug[u][n - 1]);
            }
            if (t == 0) { ii[u] = __fadd_rn(0.0f, c); continue; }
            const float v_dec = __fadd_rn(vv[u], __fmul_rn(p.ca, __fsub_rn(ii[u], vv[u])));
            const float i_dec = __fadd_rn(ii[u], __fmul_rn(p.cb, ii[u]));
            const bool z = v_dec > p.v_th;
            vv[u] = z ? p.v_reset : v_dec;
            ii[u] = __fadd_rn(i_dec, c);
            const unsigned long long b = __ballot(z);
            G3_KEEP_BALLOT(my0[u], my1[u], b, t);
            if (COUNT) { cnt_lo[u] += (uint32_t)__builtin_popcount((uint32_t)b); cnt_hi[u] += (uint32_t)__builtin_popcount((uint32_t)(b >> 32)); }
        }
    }
}

// The same recurrence with T and the window at run time (one neuron per lane): u_1 .. u_3 are read once (terms of every / every second /
// every third step), the larger divisors where a step needs them - the order of k_gemm_bf16x3's tile_current (ascending n), so the sums
// are those of the straight-line instances bit for bit.  For the (T, window) pairs outside sp_lif_fixed's grid: a linear layer's tile
// then holds 16 or 32 RoIs, i.e. one or two of these per wave and column pass behind a 196-step K loop.
template <bool COUNT>
__device__ __forceinline__ void sp_lif_general(const float* src, const int group_stride, const NeuronP& p, const int T, const int Tcs, const uint32_t* div,
                                               const int lane, uint32_t& my0, uint32_t& my1, uint32_t& cnt_lo, uint32_t& cnt_hi) {
    const float u1 = src[0];
    const float u2 = Tcs > 1 ? src[(size_t)group_stride] : 0.0f;
    const float u3 = Tcs > 2 ? src[(size_t)2 * group_stride] : 0.0f;
    float vv = 0.0f, ii = 0.0f;
    for (int t = 0; t < T; ++t) {
        float c = 0.0f;
        if (t < Tcs) {
            uint32_t m = __builtin_amdgcn_readfirstlane(div[t]);                   // wave-uniform; divisors in ascending order
            c = u1;
            if (m & 2u) c = __fadd_rn(c, u2);
            if (m & 4u) c = __fadd_rn(c, u3);
            m &= ~7u;
            while (m) {
                const int g = __builtin_ctz(m);
                m &= m - 1;
                c = __fadd_rn(c, src[(size_t)g * group_stride]);
            }
        }
        if (t == 0) { ii = __fadd_rn(0.0f, c); continue; }
        const float v_dec = __fadd_rn(vv, __fmul_rn(p.ca, __fsub_rn(ii, vv)));
        const float i_dec = __fadd_rn(ii, __fmul_rn(p.cb, ii));
        const bool z = v_dec > p.v_th;
        vv = z ? p.v_reset : v_dec;
        ii = __fadd_rn(i_dec, c);
        const unsigned long long b = __ballot(z);
        my0 = lane == t ? (uint32_t)b : my0;
        my1 = lane == t ? (uint32_t)(b >> 32) : my1;
        if (COUNT) { cnt_lo += (uint32_t)__builtin_popcount((uint32_t)b); cnt_hi += (uint32_t)__builtin_popcount((uint32_t)(b >> 32)); }
    }
}

// spike-rate mode of the sparse conv: spikes per (level, image) slot from the per-position counts; block = (slot, chunk of the image's
// positions), one integer atomic per block (round 5: one block per slot took 71 us for the 73 728 positions of a level-0 image)
#define POSCNT_CHUNKS 32
struct PosCountArgs { const uint32_t* cnt_pos; unsigned long long* cnt_img; int n_levels, max_n; ConvLevelDev lv[SNN_MAX_LEVELS]; };
__global__ __launch_bounds__(256) void k_sum_pos_counts(const PosCountArgs a) {
    __shared__ unsigned long long part[4];
    const int l = blockIdx.x / a.max_n, n = blockIdx.x % a.max_n;
    unsigned long long sum = 0;
    if (n < a.lv[l].N) {
        const int hw = a.lv[l].H * a.lv[l].W;
        const uint32_t* src = a.cnt_pos + a.lv[l].pos_base + (size_t)n * hw;
        for (int i = blockIdx.y * 256 + threadIdx.x; i < hw; i += 256 * POSCNT_CHUNKS) sum += src[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = part[0] + part[1] + part[2] + part[3];
        if (tot) atomicAdd(a.cnt_img + blockIdx.x, tot);
    }
}

// LIF of the FAT conv in REGISTERS (round 5).  The wave's accumulators hold all TS - 1 period sums of its own 16 positions x 64 columns
// (slot s = plane s): lane (lg, lr) has, for r < 4 and nt < 4, the neuron (position 4 lg + r, column 16 nt + lr).  No tile image in LDS,
// no work-group barrier: the recurrence of sp_lif_fixed (same operations, same order of the divisor sums) runs on the four N-tiles of a
// row r at once (four independent chains), the ballot of N-tile nt holds in bits 16 lg .. 16 lg + 15 the half-word (columns 16 nt ..) of
// position 4 lg + r, and lane lr of group lg keeps the word (step 1 + (lr >> 1), columns 32 (lr & 1) ..) of its position - 16 (step, word)
// combinations per position for TS <= 9; step 0 never spikes (its plane is written as zeros).
template <int TS, int D, int NTL, int MTS_, bool COUNT>
__device__ __forceinline__ void sp_lif_regs(const f32x4 (&acc)[MTS_][NTL], const NeuronP& p, const int lane, uint32_t (&mine)[4], uint32_t (&cnt)[4]) {
    constexpr int TCS = TS - D;                          // conv: D = 1; fc6: D = 2 (dead time steps)
    static_assert(NTL == 4 || NTL == 2, "64 columns (two words per position) or 32 (one)");
    static_assert(TCS <= MTS_ && TS - 1 <= (NTL == 4 ? 8 : 16), "all planes of a block in one wave; 16 (step, word) lanes per position");
    const int sh = 16 * (lane >> 4), lr = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float vv[NTL], ii[NTL];
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) { vv[nt] = 0.0f; ii[nt] = 0.0f; }
        uint32_t keep = 0, count = 0;
#pragma unroll
        for (int t = 0; t < TS; ++t) {
            unsigned long long b[NTL];
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt) {
                b[nt] = 0;
                float c = 0.0f;
                if (t < TCS) {
                    c = acc[0][nt][r];
#pragma unroll
                    for (int n = 2; n <= t + 1; ++n)
                        if ((t + 1) % n == 0) c = __fadd_rn(c, acc[n - 1][nt][r]);
                }
                if (t == 0) { ii[nt] = __fadd_rn(0.0f, c); continue; }
                const float v_dec = __fadd_rn(vv[nt], __fmul_rn(p.ca, __fsub_rn(ii[nt], vv[nt])));
                const float i_dec = __fadd_rn(ii[nt], __fmul_rn(p.cb, ii[nt]));
                const bool z = v_dec > p.v_th;
                vv[nt] = z ? p.v_reset : v_dec;
                ii[nt] = __fadd_rn(i_dec, c);
                b[nt] = __ballot(z);
            }
            if (t == 0) continue;
            const uint32_t w0 = ((uint32_t)(b[0] >> sh) & 0xffffu) | ((uint32_t)(b[1] >> sh) << 16);
            uint32_t w1 = 0;
            if constexpr (NTL == 4) {                    // lane lr <-> (step 1 + (lr >> 1), word lr & 1)
                w1 = ((uint32_t)(b[2] >> sh) & 0xffffu) | ((uint32_t)(b[3] >> sh) << 16);
                keep = (lr >> 1) == t - 1 ? ((lr & 1) ? w1 : w0) : keep;
            } else {                                     // lane lr <-> step 1 + lr
                keep = lr == t - 1 ? w0 : keep;
            }
            if (COUNT) count += (uint32_t)__builtin_popcount(w0) + (uint32_t)__builtin_popcount(w1);     // (spike-rate mode: this position's spikes of the step)
        }
        mine[r] = keep;
        cnt[r] = count;
    }
}

// WN = waves along the 64 columns.  1: 8 row-waves x 4 slots, every wave reads the whole weight slot from LDS each step (192 KB per
// work-group and step).  2: 4 row-waves x 6 slots, a wave covers 32 columns and reads half of the slot (96 KB): the shape for launches whose
// matrix-pipe time per step is below what those LDS reads take - fc6, whose tiles hold 32 RoIs (tools: profiles/r4_sparse_timeline.txt).
// FAT (linear layers, WN = 2; round 5): the same tile run by FOUR waves - 2 x 2, twelve M-tile slots per row-wave, 256 threads with up to
// 256 registers per lane; still two work-groups per CU, i.e. two waves per SIMD from DIFFERENT work-groups.  Every weight fragment read
// from LDS feeds twice the matrix instructions (the what-if builds price those reads at 9 % of the detector head and 14 % of the conv
// launch, profiles/r5_sparse_whatif.txt), and the registers pay for a third weight-fragment buffer: fragments are requested two groups
// ahead of their matrix instructions (one group ahead the shape LOSES 2 %).  Measured (profiles/r5_fat_wave_ab.txt, same lease): detector
// head 0.780 -> 0.756 ms at T = 12.  For the conv (4 row-waves x 8 slots) the K loop gained 4.6 % and the LIF epilogue lost it again
// (one wave per SIMD and work-group issues a vector instruction every four cycles, two interleave at two): 1.955 -> 1.940 ms at T = 8,
// +2 % at T = 16 - not instantiated.  (The BIG shape tried first - 512 threads, 48 slots, ONE work-group per CU, 4-slot ring - was
// bit-identical and 34 % / 6 % SLOWER on the conv / detector head, profiles/r5_big_tile_ab.txt: two lock-stepped waves of one work-group per
// SIMD leave the pipe idle at every barrier.)
// The kernel's text lives in snn_sparse_kernel.h and is instantiated per weight-plane count: three planes (bf16x3), and one (precision "bf16")
#define SP_KERNEL k_gemm_lif_sparse
#define SP_NPL 3
#include "snn_sparse_kernel.h"
#undef SP_KERNEL
#undef SP_NPL
#define SP_KERNEL k_gemm_lif_sparse1
#define SP_NPL 1
#include "snn_sparse_kernel.h"
#undef SP_KERNEL
#undef SP_NPL
