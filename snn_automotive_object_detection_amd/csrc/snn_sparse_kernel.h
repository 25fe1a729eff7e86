// The structured-sparse GEMM + LIF kernel's text (see snn_sparse.h, which includes this file once per weight-plane count; no include guard).
//   SP_KERNEL  name of the __global__ template <CONV, WN, FAT>
//   SP_NPL     bf16 planes of the packed weights: 3 (k_gemm_lif_sparse: hi + mid + lo, exact) or 1 (k_gemm_lif_sparse1, precision "bf16": every weight
//              rounded once to the nearest bf16 by the packer, snn_pack_*_bf16 - a third of the matrix instructions, weight bytes and fragment reads)
// An accumulator sees the same instructions in the same k order at both counts, minus those of the mid / lo planes - so on bf16-representable
// weights both kernels give the same bits.  The ring slots keep their size (a single-plane slot uses a third of its weight part): same tiles, same
// occupancy.  (Instantiated as text and not through a shared __device__ body: behind a body function the optimiser schedules the three-plane
// kernels differently, and their measured instruction streams are to stay what they were - tools/symbol_diff.py.)
template <bool CONV, int WN, bool FAT = false>
__global__ __launch_bounds__(FAT ? 256 : 512, FAT ? 2 : 4) void SP_KERNEL(const SparseConvArgs args) {
    // (FAT: linear layers on 2 x 2 waves; the conv on 4 x 1 for T <= 9, on 2 x 2 beyond)
    constexpr int NPL = SP_NPL;
    static_assert(NPL == 3 || NPL == 1, "weight planes");
    constexpr int NWAVES = FAT ? 4 : 8;
    constexpr int MTS = FAT ? (WN == 1 ? SP_MT_FAT : CONV ? SP_MT2_FAT_CONV : SP_MT2_FAT) : WN == 1 ? SP_MT : SP_MT2, NT = 4 / WN;      // slots per (row-)wave, 16-column N-tiles per wave
    constexpr int ROWS = SP_ROWS;                                   // physical tile rows of a ring slot (row-waves x MTS x 16 <= 512 in every shape)
    static_assert((NWAVES / WN) * MTS * 16 <= SP_ROWS, "ring slot rows");
    constexpr int A_BYTES = SP_A_ARR * ROWS * 4, SLOT = A_BYTES + SP_B_BYTES;
    constexpr int NPASS = FAT ? 2 : 1;                              // A-staging passes of a wave (64 rows each) per step
#ifndef SP_FAT_BDEPTH
#define SP_FAT_BDEPTH 2
#endif
    constexpr int BDEPTH = FAT ? SP_FAT_BDEPTH : 1;                 // groups the weight-fragment reads run ahead of their matrix instructions
#ifdef SNN_EXP_TIMELINE     // diagnostic build: wall-clock stamps (s_memrealtime, 100 MHz) of the work-group's phases.  Each stamp is stored at once (thread 0): the
    // 512-thread shapes sit at their 128-register limit, and stamps kept in registers until the end made the round-5 builds spill (304 bytes per lane: a
    // K loop 35 % slower than the product's)
#define SP_TL_STAMP(i) do { if (threadIdx.x == 0) { unsigned long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
                                                   args.tl[(size_t)blockIdx.x * 8 + (i)] = t_; } } while (0)
    SP_TL_STAMP(0);
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t smem_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    unsigned char* const lut = smem;
    unsigned char* const ring = smem + G3_LUT_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lg = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;                       // row-wave, column-wave
    // block order: XCD x = blockIdx % 8 takes xcd_cpx column blocks on a contiguous range of row tiles (k_gemm_bf16x3: xcd_contig)
    // (xcd_contig == 0 - the linear layers: plain order, column block fastest: an XCD only ever sees two weight panels, and all
    // work-groups of a panel walk K together)
    int nb = blockIdx.x % args.n_blocks, mb = blockIdx.x / args.n_blocks;
    // conv / fc6 route: in the entry block, so that the gate's kernel arguments arrive with n_blocks / xcd_contig (as the kernel's very first statement the
    // test put one more kernarg round trip in front of every work-group: 0.2 % of the step over the conv launch's 24 rounds of work-groups)
    G3_GATE(args);
    if (args.xcd_contig) {
        const int x = blockIdx.x & 7, j = blockIdx.x >> 3, cpx = args.xcd_cpx, groups = args.n_blocks / cpx;
        nb = (x % groups) * cpx + j % cpx;
        mb = (x / groups) * args.xcd_contig + j / cpx;
        if (j / cpx >= args.xcd_contig || mb >= args.n_tiles) return;
    }
    nb = __builtin_amdgcn_readfirstlane(nb);
    mb = __builtin_amdgcn_readfirstlane(mb);
    const int pb = args.pb, M = args.M, Kc = args.Kc, Np = args.Np;
    const int m0 = mb * pb;
    if (tid < 256) {
        uint4 q;
        q.x = bf16_pair(tid, 0); q.y = bf16_pair(tid, 1); q.z = bf16_pair(tid, 2); q.w = bf16_pair(tid, 3);
        *reinterpret_cast<uint4*>(lut + tid * 16) = q;
    }
    const int nd_w = __builtin_amdgcn_readfirstlane((int)args.w_nd[wm]), ns_w = __builtin_amdgcn_readfirstlane((int)args.w_ns[wm]);
    // ---- A staging: lane L of the wave stages row L & 15 of one M-tile slot of its row-wave.  WN = 1: slot L >> 4 (64 rows per wave);
    // WN = 2: the two column-waves of a row-wave take three slots each (lanes 0 .. 47).  FAT: two passes - WN = 1: the wave's eight slots
    // (64 + 64 lanes); WN = 2: half the row-wave's slots per column-wave (six: 64 + 32 lanes; eight - the conv: 64 + 64)
    const void* a_base[SP_A_ARR];
#pragma unroll
    for (int j = 0; j < SP_A_ARR; ++j) a_base[j] = sgpr_ptr(reinterpret_cast<const char*>(args.enc) + (size_t)j * args.Pe * 4);
    uint32_t voff[NPASS], inc[NPASS];                       // byte offset from args.enc of the lane's first dword; array j of the step is
                                                            // j word planes further (dense lanes use two, the rest lands in unused LDS)
    bool a_lane[NPASS];
    uint32_t tap_fix[NPASS], row_fix[NPASS];
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const int xs = FAT ? (WN == 1 ? 4 * ps + (lane >> 4) : min((MTS / 2) * wn + 4 * ps + (lane >> 4), MTS - 1)) : WN == 1 ? (lane >> 4) : min(3 * wn + (lane >> 4), MTS - 1);
        a_lane[ps] = FAT ? (WN == 1 || lane < (ps == 0 ? 64 : (MTS / 2 - 4) * 16)) : (WN == 1 || lane < 48);
        const int xplane = args.mt_plane[wm][xs];
        const bool xused = xplane >= 0, xdense = xused && xplane < args.nd;
        const int lp = min(args.mt_j[wm][xs] * 16 + (lane & 15), pb - 1);
        const int p = min(m0 + (xused ? lp : 0), M - 1);
        uint32_t row0 = (uint32_t)p;                        // linear layer: the RoI
        int W = 0;
        if (CONV) {
            int l = 0;
            while (l + 1 < args.n_levels && p >= args.lv[l + 1].pos_base) ++l;
            const int H = args.lv[l].H;
            W = args.lv[l].W;
            const int local = p - args.lv[l].pos_base;
            const int n = local / (H * W), rem = local % (H * W);
            const int y = rem / W, x = rem % W;
            row0 = (uint32_t)args.lv[l].tile_begin + (uint32_t)((n * (H + 2) + y) * (W + 2) + x);      // tap (-1, -1)
        }
        const uint32_t Pe = args.Pe;
        const int Cw2 = args.Cw / 2;
        if (xdense || !xused) {
            const int t = xused ? xplane : 0;
            voff[ps] = (uint32_t)(((size_t)t * args.Cw * Pe + row0) * 4);
            inc[ps] = 2 * Pe * 4;
        } else {
            const uint32_t delta = (uint32_t)((const char*)args.cmp - (const char*)args.enc);
            voff[ps] = delta + (uint32_t)(((size_t)(xplane - args.nd) * Cw2 * SP_A_ARR * Pe + row0) * 4);
            inc[ps] = SP_A_ARR * Pe * 4;
        }
        tap_fix[ps] = 4u - (uint32_t)Cw2 * inc[ps];         // next tap of the row: one position on, back to channel word 0
        row_fix[ps] = (uint32_t)((W + 2 - 3) * 4);          // after the third tap of a row: one padded image row down
    }
    // physical row (wm MTS + slot) 16 + r; a pass covers four slots
    const uint32_t a_dst = smem_base + G3_LUT_BYTES + (FAT ? (wm * MTS + (WN == 1 ? 0 : (MTS / 2) * wn)) * 64 : WN == 1 ? wave * 256 : (wm * MTS + 3 * wn) * 64);
    const int cw2_s = __builtin_amdgcn_readfirstlane(args.Cw / 2);
    int f_c = 0, f_tap = 0;
    auto stage_a = [&](const uint32_t slot_off) __attribute__((always_inline)) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const uint32_t d = __builtin_amdgcn_readfirstlane(a_dst + slot_off + ps * 256);
            if (a_lane[ps]) {
                asm volatile("s_mov_b32 m0, %5\n\ts_nop 4\n\tglobal_load_lds_dword %0, %1\n\t"
                             "s_add_u32 m0, m0, %6\n\ts_nop 0\n\tglobal_load_lds_dword %0, %2\n\t"
                             "s_add_u32 m0, m0, %6\n\ts_nop 0\n\tglobal_load_lds_dword %0, %3\n\t"
                             "s_add_u32 m0, m0, %6\n\ts_nop 0\n\tglobal_load_lds_dword %0, %4"
                             :: "v"(voff[ps]), "s"(a_base[0]), "s"(a_base[1]), "s"(a_base[2]), "s"(a_base[3]), "s"(d), "s"((uint32_t)(ROWS * 4))
                             : "memory", "scc");
            }
            voff[ps] += inc[ps];
        }
        if (!CONV) return;
        f_c = __builtin_amdgcn_readfirstlane(f_c + 1);
        if (f_c == cw2_s) {
            f_c = 0;
            f_tap = __builtin_amdgcn_readfirstlane(f_tap + 1);
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) voff[ps] += tap_fix[ps] + (f_tap == 3 ? row_fix[ps] : 0u);
            if (f_tap == 3) f_tap = 0;
        }
    };

    // ---- B staging: 24 pieces of 1 KB per step (2 chunks x 3 planes x 4 blocks of 16 columns; 8 at one plane); wave w copies pieces w, w + NWAVES, ..
    constexpr int B_CHUNK = NPL * 64 * G3_ROWB;                                // LDS bytes of one 32-deep chunk's weight planes
    const int brow = (wave & 3) * 16 + (lane >> 2);
    const uint32_t b_off = (uint32_t)((nb * 64 + brow) * 64 + (((lane & 3) ^ G3_SWZ(brow)) << 4));
    const unsigned long long b_chunk = (unsigned long long)Np * 64, b_plane = args.plane_elems * 2;
    unsigned long long s_ptr = (unsigned long long)args.wpk;                  // chunk 2 * step, plane 0
    const uint32_t b_dst = smem_base + G3_LUT_BYTES + A_BYTES + (wave & 3) * 1024;
    auto stage_b = [&](const uint32_t slot_off) __attribute__((always_inline)) {
        const uint32_t d = __builtin_amdgcn_readfirstlane(b_dst + slot_off);
#pragma unroll
        for (int i = 0; i < 8 * NPL / NWAVES; ++i) {
            const int piece = wave + NWAVES * i;                               // wave-uniform; piece & 3 = wave & 3 = its block of 16 columns
            const int c2 = piece / (4 * NPL), pl = (piece % (4 * NPL)) / 4;
            glds16(sgpr_ptr(reinterpret_cast<const void*>(s_ptr + c2 * b_chunk + pl * b_plane)), b_off, d + c2 * B_CHUNK + pl * (64 * G3_ROWB));
        }
        s_ptr += 2 * b_chunk;
    };

    const unsigned char* const a_rd = ring + (wm * MTS * 16 + lr) * 4;                      // + slot offset, M-tile slot * 64
    const unsigned char* const b_rd = ring + A_BYTES + (wn * NT * 16 + lr) * G3_ROWB + ((lg ^ G3_SWZ(lr)) << 4);
    f32x4 acc[MTS][NT];
#pragma unroll
    for (int mt = 0; mt < MTS; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int n_steps = Kc / 2;
    stage_a(0); stage_b(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

#ifdef SNN_EXP_TIMELINE
    SP_TL_STAMP(1);
#endif
#if defined(SNN_EXP_SP_NO_AREAD) || defined(SNN_EXP_SP_NO_BREAD)
    const bfv8 exp_a = *reinterpret_cast<const bfv8*>(lut + ((lane * 5) & 255) * 16);
    const bfv8 exp_b0 = *reinterpret_cast<const bfv8*>(b_rd), exp_b1 = *reinterpret_cast<const bfv8*>(b_rd + B_CHUNK);
#endif
    auto step_loop = [&](auto nd_c, auto ns_c) __attribute__((always_inline)) {
        constexpr int ND = decltype(nd_c)::value, NS = decltype(ns_c)::value;
        // A AHEAD (FAT conv on 4 x 1 waves: a wave reads only the rows it staged itself): the next step's A fragments - occupancy bytes, table
        // fragments, indices, secondary ballots - are requested at the END of a step, once this wave's copies have landed and BEFORE the step
        // barrier, into the registers the step's own fragments have just left: the byte -> table-fragment chain runs while the wave would wait
        // at the barrier anyway, and the first matrix instruction behind it finds its operand
        constexpr bool PRE_A = SP_PRE_A && WN == 1 && FAT;     // (the 512-thread shapes have no register to spare: the 8 x 1 conv spills with it)
        bfv8 p_ad[ND > 0 ? ND : 1][2], p_as[NS > 0 ? NS : 1];
        int p_ix[NS > 0 ? NS : 1];
        unsigned long long p_sec[4] = {0, 0, 0, 0};
        auto load_a_all = [&](const uint32_t off) __attribute__((always_inline)) {
#pragma unroll
            for (int d = 0; d < ND; ++d)
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    const uint32_t byte = *reinterpret_cast<const uint8_t*>(a_rd + off + c2 * (ROWS * 4) + d * 64 + lg);
                    p_ad[d][c2] = *reinterpret_cast<const bfv8*>(lut + (byte << 4));
                }
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const unsigned char* r = a_rd + off + (ND + q) * 64;
                const uint32_t occ = *reinterpret_cast<const uint8_t*>(r + lg);
                p_as[q] = *reinterpret_cast<const bfv8*>(lut + (occ << 4));
                p_ix[q] = (int)*reinterpret_cast<const uint16_t*>(r + (1 + (lg >> 1)) * (ROWS * 4) + 2 * (lg & 1));
            }
#pragma unroll
            for (int b4 = 0; b4 < (NS + 3) / 4; ++b4) {
                const uint32_t o2 = *reinterpret_cast<const uint32_t*>(a_rd + off + 3 * (ROWS * 4) + min(ND + 4 * b4 + lg, MTS - 1) * 64);
                p_sec[b4] = __ballot(o2 != 0u) & (NS - 4 * b4 >= 4 ? ~0ull : ((1ull << (16 * (NS - 4 * b4))) - 1ull));
            }
        };
        // weight fragments of group g = (N-tile g / 3, plane 2 - g % 3: small terms first): both 32-deep chunks of the step as ONE
        // 16-element operand (the structured-sparse instruction's B; its halves are the dense instruction's B of chunk c, c + 1),
        // buffered by g modulo the depth - the loads land in the halves of the buffer a later group reads, no register copies
#ifndef SP_FAT_BDEPTH_LIN
#define SP_FAT_BDEPTH_LIN 5
#endif
#ifndef SP_FAT_BDEPTH_C41
#define SP_FAT_BDEPTH_C41 BDEPTH
#endif
        // (round 6) the FAT linear layers (2 x 2 waves, six groups per step, 211 registers at two ahead) have the registers to request ALL of a step's weight fragments at its
        // top - five groups ahead, six buffers: detector head 0.700 -> 0.685 ms at T_det = 12, 1.533 -> 1.519 at 24 (profiles/r6_fc6_bdepth_ab.txt), same bits
        // (one plane: a step has NT groups - the FAT shapes request all of them at its top, NT - 1 ahead; the others stay one ahead)
        constexpr int BD = NPL == 1 ? ((FAT && ND + NS <= 12) ? NT - 1 : 1)
                         : (FAT && ND + NS > 12) ? 1 : (FAT && !CONV) ? SP_FAT_BDEPTH_LIN : (FAT && CONV && WN == 1) ? SP_FAT_BDEPTH_C41 : BDEPTH;   // (the largest row-waves have no registers for a third buffer)
        constexpr bool TWO_PART = FAT && ND + NS > 14;
        // B HEAD START (-DSP_PRE_B=1, off: measured slower; FAT shapes whose step is one part): the first BD groups' fragments of step s + 1
        // requested right behind the barrier of step s - ahead of the copies' issue and the secondary-plane ballots of the step's top
        // (3 NT is a multiple of BD + 1: the ring carries over from step to step)
        constexpr bool PRE_B = SP_PRE_B && FAT && !TWO_PART;
        static_assert((NPL * NT) % (BD + 1) == 0, "fragment ring carries over");
        bfv16 bbuf[BD + 1];
        auto load_b = [&](bfv16& dst, const uint32_t off, const int gn) __attribute__((always_inline)) {
#ifdef SNN_EXP_SP_NO_BREAD                            // (timing experiment: the weight fragments stay what they were before the loop)
            const bfv8 lo = exp_b0, hi = exp_b1;
#else
            const bfv8 lo = *reinterpret_cast<const bfv8*>(b_rd + off + (NPL - 1 - gn % NPL) * (64 * G3_ROWB) + (gn / NPL) * 16 * G3_ROWB);
            const bfv8 hi = *reinterpret_cast<const bfv8*>(b_rd + off + B_CHUNK + (NPL - 1 - gn % NPL) * (64 * G3_ROWB) + (gn / NPL) * 16 * G3_ROWB);
#endif
            dst = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
        };
        if constexpr (PRE_A) load_a_all(0);
        if constexpr (PRE_B) {
#pragma unroll
            for (int g0 = 0; g0 < BD; ++g0) load_b(bbuf[g0], 0u, g0);
        }
        for (int s = 0; s < n_steps; ++s) {
            const uint32_t o_cur = (uint32_t)((s & 1) * SLOT), o_nxt = (uint32_t)(((s + 1) & 1) * SLOT);
            if (s + 1 < n_steps) {
#ifndef SNN_EXP_SP_NO_A                             // (timing experiments: what do the copies cost - wrong results)
                stage_a(o_nxt);
#endif
#ifndef SNN_EXP_SP_NO_B
                stage_b(o_nxt);
#endif
            }
            // which of the sparse M-tiles hold a third spike of a nibble in this step?  Lane L looks at the secondary occupancy dword of
            // row L & 15 of sparse slot L >> 4 (more than four sparse slots: a second / third / fourth look)
            unsigned long long sec[4] = {0, 0, 0, 0};             // bits 16 q .. 16 q + 15 of word b = sparse slot 4 b + q
#ifndef SNN_EXP_SP_NO_AREAD
            if constexpr (PRE_A) {
#pragma unroll
                for (int b4 = 0; b4 < 4; ++b4) sec[b4] = p_sec[b4];
            }
            // (round 6, FAT conv on 2 x 2 waves: the secondary occupancy words are REQUESTED here and looked at behind the step's products, where the answer is
            // first needed - the ballot right behind the read made every step open with a full LDS round trip: conv + LIF 3.789 -> 3.753 ms at T = 16; the
            // linear layers measured 0.4 % slower with it and keep the early look, profiles/r6_sec_late_ab.txt)
            constexpr bool SEC_LATE = SP_SEC_LATE && FAT && CONV && WN == 2;
            uint32_t o2_late[(NS + 3) / 4 > 0 ? (NS + 3) / 4 : 1];
            if constexpr (!PRE_A && SEC_LATE) {
#pragma unroll
                for (int b4 = 0; b4 < (NS + 3) / 4; ++b4)
                    o2_late[b4] = *reinterpret_cast<const uint32_t*>(a_rd + o_cur + 3 * (ROWS * 4) + min(ND + 4 * b4 + lg, MTS - 1) * 64);
            } else if constexpr (!PRE_A) {
#pragma unroll
                for (int b4 = 0; b4 < (NS + 3) / 4; ++b4) {
                    const uint32_t o2 = *reinterpret_cast<const uint32_t*>(a_rd + o_cur + 3 * (ROWS * 4) + min(ND + 4 * b4 + lg, MTS - 1) * 64);
                    sec[b4] = __ballot(o2 != 0u) & (NS - 4 * b4 >= 4 ? ~0ull : ((1ull << (16 * (NS - 4 * b4))) - 1ull));
                }
            }
#endif
            // The step's products, in one part or - the largest row-wave, 15 M-tiles: no registers for all A fragments at once - in two (each
            // reads the weight fragments; every accumulator still sees its instructions in the same order).  part = the dense M-tiles (if
            // DENSE) and the sparse slots Q0 .. Q1 - 1
            auto do_part = [&](auto q0_c, auto q1_c, auto dense_c) __attribute__((always_inline)) {
                constexpr int Q0 = decltype(q0_c)::value, Q1 = decltype(q1_c)::value, NQ = Q1 - Q0;
                constexpr bool DENSE = decltype(dense_c)::value && ND > 0;
                // A fragments of this part
                bfv8 ad[ND > 0 ? ND : 1][2], as[NQ > 0 ? NQ : 1];
                int ix[NQ > 0 ? NQ : 1];
#ifdef SNN_EXP_SP_NO_AREAD                            // (timing experiment: no LDS reads on the A side - wrong results)
#pragma unroll
                for (int d = 0; d < ND; ++d) { ad[d][0] = exp_a; ad[d][1] = exp_a; }
#pragma unroll
                for (int q = 0; q < NQ; ++q) { as[q] = exp_a; ix[q] = 0x4444; }
#else
                if constexpr (PRE_A) {                          // (requested at the end of the previous step)
#pragma unroll
                    for (int d = 0; d < ND; ++d) { ad[d][0] = p_ad[d][0]; ad[d][1] = p_ad[d][1]; }
#pragma unroll
                    for (int q = 0; q < NQ; ++q) { as[q] = p_as[Q0 + q]; ix[q] = p_ix[Q0 + q]; }
                } else {
                    if (DENSE) {
#pragma unroll
                        for (int d = 0; d < ND; ++d)
#pragma unroll
                            for (int c2 = 0; c2 < 2; ++c2) {
                                const uint32_t byte = *reinterpret_cast<const uint8_t*>(a_rd + o_cur + c2 * (ROWS * 4) + d * 64 + lg);
                                ad[d][c2] = *reinterpret_cast<const bfv8*>(lut + (byte << 4));
                            }
                    }
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const unsigned char* r = a_rd + o_cur + (ND + Q0 + q) * 64;
                        const uint32_t occ = *reinterpret_cast<const uint8_t*>(r + lg);
                        as[q] = *reinterpret_cast<const bfv8*>(lut + (occ << 4));
                        ix[q] = (int)*reinterpret_cast<const uint16_t*>(r + (1 + (lg >> 1)) * (ROWS * 4) + 2 * (lg & 1));
                    }
                }
#endif
                // weight fragments: the ring of the step loop (BD groups ahead of their matrix instructions)
                if constexpr (!PRE_B) {
#pragma unroll
                    for (int g0 = 0; g0 < BD; ++g0) load_b(bbuf[g0], o_cur, g0);
                }
#pragma unroll
                for (int g = 0; g < NPL * NT; ++g) {
#ifndef SNN_EXP_SP_NO_BREAD
                    if (g + BD < NPL * NT) load_b(bbuf[(g + BD) % (BD + 1)], o_cur, g + BD);
#endif
                    const bfv16 bb = bbuf[SNN_EXP_BSEL(g) % (BD + 1)];
#ifndef SNN_EXP_SP_NO_MFMA                            // (timing experiment: everything but the matrix instructions)
                    if (DENSE) {
                        const bfv8 b0 = __builtin_shufflevector(bb, bb, 0, 1, 2, 3, 4, 5, 6, 7), b1 = __builtin_shufflevector(bb, bb, 8, 9, 10, 11, 12, 13, 14, 15);
#pragma unroll
                        for (int d = 0; d < ND; ++d) {
                            acc[d][g / NPL] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad[d][0], b0, acc[d][g / NPL], 0, 0, 0);
                            acc[d][g / NPL] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad[d][1], b1, acc[d][g / NPL], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        acc[ND + Q0 + q][g / NPL] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(as[q], bb, acc[ND + Q0 + q][g / NPL], ix[q], 0, 0);
#else
                    asm volatile("" :: "v"(bb));
                    if (DENSE) {
#pragma unroll
                        for (int d = 0; d < ND; ++d) asm volatile("" :: "v"(ad[d][0]), "v"(ad[d][1]));
                    }
#pragma unroll
                    for (int q = 0; q < NQ; ++q) asm volatile("" :: "v"(as[q]), "v"(ix[q]));
#endif
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if constexpr (TWO_PART) {
                constexpr int QS = (NS - 2 * ND + 1) / 2;          // (two parts of about equal matrix work: a dense M-tile counts twice)
                do_part(std::integral_constant<int, 0>{}, std::integral_constant<int, QS>{}, std::true_type{});
                do_part(std::integral_constant<int, QS>{}, std::integral_constant<int, NS>{}, std::false_type{});
            } else {
                do_part(std::integral_constant<int, 0>{}, std::integral_constant<int, NS>{}, std::true_type{});
            }
#if !defined(SNN_EXP_SP_NO_AREAD)
            if constexpr (!PRE_A && SEC_LATE) {
#pragma unroll
                for (int b4 = 0; b4 < (NS + 3) / 4; ++b4)
                    sec[b4] = __ballot(o2_late[b4] != 0u) & (NS - 4 * b4 >= 4 ? ~0ull : ((1ull << (16 * (NS - 4 * b4))) - 1ull));
            }
#endif
#ifdef SNN_EXP_SP_NO_SEC                              // (timing experiment - wrong results: what does the secondary plane's second pass cost?)
            if (false) {
#else
            if (NS > 0 && (sec[0] | sec[1] | sec[2] | sec[3]) != 0ull) {   // (rare) the secondary plane of the M-tiles that have one in this step
#endif
#pragma unroll
                for (int q = 0; q < NS; ++q) {
                    if (((sec[q >> 2] >> (16 * (q & 3))) & 0xffffull) == 0ull) continue;
                    const unsigned char* r = a_rd + o_cur + (ND + q) * 64 + 3 * (ROWS * 4);
                    const uint32_t occ = *reinterpret_cast<const uint8_t*>(r + lg);
                    const bfv8 a2 = *reinterpret_cast<const bfv8*>(lut + (occ << 4));
                    const int i2 = 0xeeee;                   // every nibble: positions (2, 3)
#pragma unroll
                    for (int g = 0; g < NPL * NT; ++g) {
                        const bfv8 c0 = *reinterpret_cast<const bfv8*>(b_rd + o_cur + (NPL - 1 - g % NPL) * (64 * G3_ROWB) + (g / NPL) * 16 * G3_ROWB);
                        const bfv8 c1 = *reinterpret_cast<const bfv8*>(b_rd + o_cur + B_CHUNK + (NPL - 1 - g % NPL) * (64 * G3_ROWB) + (g / NPL) * 16 * G3_ROWB);
                        bfv16 bb;
#pragma unroll
                        for (int i = 0; i < 8; ++i) { bb[i] = c0[i]; bb[8 + i] = c1[i]; }
                        acc[ND + q][g / NPL] = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a2, bb, acc[ND + q][g / NPL], i2, 0, 0);
                    }
                }
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_waitcnt(0x0070);              // vmcnt(0) lgkmcnt(0): the next step's copies have landed
#ifndef SNN_EXP_SP_NO_AREAD
            if constexpr (PRE_A) {
                if (s + 1 < n_steps) load_a_all(o_nxt);       // (this wave's own rows; the table-fragment reads stay in flight across the barrier)
            }
#endif
#ifndef SNN_EXP_SP_NO_BAR                             // (timing experiment: waves run ahead of each other's copies - wrong results)
            __builtin_amdgcn_s_barrier();
#endif
            asm volatile("" ::: "memory");
            if constexpr (PRE_B) {
                if (s + 1 < n_steps) {
#pragma unroll
                    for (int g0 = 0; g0 < BD; ++g0) load_b(bbuf[g0], o_nxt, g0);
                }
            }
        }
    };
// (dense, sparse) M-tile counts of a row-wave the FAT shapes have loop instances for (host: sparse_plan_wn checks against the same lists)
// FAT conv: every wave (2 dense, Tc - 2 sparse), T = 7 .. 9 (T = 5 / 6 measured 9.5 % / 1.3 % SLOWER than the 8-wave shape, whose tiles
// hold 128 / 80 positions there against the FAT conv's 64: profiles/r5_fat_conv_ab.txt)
#define SP_FAT1_INSTANCES {2, 5}, {2, 4}, {2, 6}
#define SP_FAT1_CASES SP_CASE(2, 5) SP_CASE(2, 4) SP_CASE(2, 6)
// FAT conv on 2 x 2 waves, T = 12 .. 16 (instances from T = 10: 10 / 11 measured slower than the 8-wave shape): every row-wave (2 dense, Tc - 2 sparse)
#define SP_FAT1B_INSTANCES {2, 7}, {2, 8}, {2, 9}, {2, 10}, {2, 11}, {2, 12}, {2, 13}
#define SP_FAT1B_CASES SP_CASE(2, 7) SP_CASE(2, 8) SP_CASE(2, 9) SP_CASE(2, 10) SP_CASE(2, 11) SP_CASE(2, 12) SP_CASE(2, 13)
#define SP_FAT2_INSTANCES {2, 8}, {2, 7}, {2, 9}, {2, 10}, {2, 6}, {2, 5}, {2, 4}, {2, 3}, {2, 2}, {1, 10}, {1, 11}, {1, 9}, {1, 8}, {1, 7}, {1, 6}, {1, 5}
#define SP_FAT2_CASES SP_CASE(2, 8) SP_CASE(2, 7) SP_CASE(2, 9) SP_CASE(2, 10) SP_CASE(2, 6) SP_CASE(2, 5) SP_CASE(2, 4) SP_CASE(2, 3) SP_CASE(2, 2) \
                      SP_CASE(1, 10) SP_CASE(1, 11) SP_CASE(1, 9) SP_CASE(1, 8) SP_CASE(1, 7) SP_CASE(1, 6) SP_CASE(1, 5)
#define SP_CASE(ND_, NS_) if (nd_w == ND_ && ns_w == NS_) step_loop(std::integral_constant<int, ND_>{}, std::integral_constant<int, NS_>{}); else
    if constexpr (FAT && CONV && WN == 1) {
        SP_FAT1_CASES { step_loop(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}); }
    } else if constexpr (FAT && CONV) {
        SP_FAT1B_CASES { step_loop(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}); }
    } else if constexpr (FAT) {
        SP_FAT2_CASES { step_loop(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}); }
    } else if constexpr (WN == 1) {
        SP_CASE(1, 3) SP_CASE(1, 2) SP_CASE(2, 2) SP_CASE(0, 4) SP_CASE(0, 3) SP_CASE(1, 1) SP_CASE(2, 1) SP_CASE(0, 2) SP_CASE(0, 1)
        SP_CASE(2, 0) SP_CASE(1, 0)
        {   // a wave without M-tiles still stages and keeps the barriers
            step_loop(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        }
    } else {
        SP_CASE(1, 4) SP_CASE(1, 5) SP_CASE(2, 4) SP_CASE(2, 3) SP_CASE(1, 3) SP_CASE(0, 6) SP_CASE(0, 5) SP_CASE(2, 2) SP_CASE(0, 4)
        SP_CASE(1, 2) SP_CASE(0, 3)
        {
            step_loop(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        }
    }
#undef SP_CASE

#ifdef SNN_EXP_TIMELINE
    SP_TL_STAMP(2);
#endif
    if (FAT && (CONV || args.lif_regs)) {                          // (block-uniform; the FAT conv has no other epilogue: its launcher plans it only where an instance exists)
        // ---- epilogue of the FAT shapes: the LIF in registers (sp_lif_regs), each (row-)wave for its own 16 positions / RoIs; no LDS, no barrier
        if constexpr (FAT) {
            const int T = args.T;
            uint32_t mine[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
            const bool counting = args.cnt_row != nullptr;
#define SP_R(n) case n: if (counting) sp_lif_regs<n, CONV ? 1 : 2, NT, MTS, true>(acc, args.p, lane, mine, cnt); \
                        else sp_lif_regs<n, CONV ? 1 : 2, NT, MTS, false>(acc, args.p, lane, mine, cnt); break;
            if constexpr (CONV && WN == 1) { switch (T) { SP_R(7) SP_R(8) SP_R(9) default: break; } }
            else if constexpr (CONV) { switch (T) { SP_R(10) SP_R(11) SP_R(12) SP_R(13) SP_R(14) SP_R(15) SP_R(16) default: break; } }
            else { switch (T) { SP_R(6) SP_R(7) SP_R(8) SP_R(9) SP_R(10) SP_R(11) SP_R(12) SP_R(13) SP_R(14) default: break; } }
#undef SP_R
            // this lane's (step, word): 64 columns per wave = two words per position (lane lr <-> step 1 + (lr >> 1), word lr & 1), 32 columns per
            // column-wave = one (lane lr <-> step 1 + lr)
            const int t_mine = 1 + (NT == 4 ? ((lane & 15) >> 1) : (lane & 15)), word = NT == 4 ? nb * 2 + (lane & 1) : nb * 2 + wn;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lp = 16 * wm + 4 * lg + r, pos = m0 + lp;
                if (pos >= M || lp >= pb) continue;
                uint32_t* dst;
                if (!CONV) dst = args.spk + (size_t)word * M + pos;                     // word-major spike planes [T][word][RoI] (fc6 -> fc7)
                else if (args.out_split) dst = args.spk + ((size_t)(word >> 2) * M + pos) * 4 + (word & 3);
                else dst = args.spk + (size_t)pos * (Np >> 5) + word;
                if (t_mine < T) dst[(size_t)t_mine * args.spk_stride] = mine[r];
                if ((lane & 15) < (NT == 4 ? 2 : 1)) dst[0] = 0u;                      // step 0: no spike
                if (counting && (lane & 15) == 0 && cnt[r]) atomicAdd(args.cnt_row + pos, cnt[r]);      // (this wave's 32 / 64 columns of the position / RoI)
            }
#ifdef SNN_EXP_TIMELINE
            SP_TL_STAMP(7); SP_TL_STAMP(3);
            if (tid == 0) {
                unsigned long long tl_exit;
                uint32_t hw, xcc;
                asm volatile("s_memrealtime %0\n\ts_getreg_b32 %1, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %2, hwreg(HW_REG_XCC_ID)\n\ts_waitcnt lgkmcnt(0)"
                             : "=s"(tl_exit), "=s"(hw), "=s"(xcc) :: "memory");
                unsigned long long* o = args.tl + (size_t)blockIdx.x * 8;
                o[4] = tl_exit; o[5] = hw; o[6] = xcc;
            }
#endif
        }
        return;
    }
    // ---- epilogue: currents -> LDS tile image (two passes of 32 columns), LIF over the T steps, spike words out
    const int T = args.T, Tc = args.Tc;
    float* const tile = reinterpret_cast<float*>(smem);
    const int rows_l = Tc * pb;
    __syncthreads();                                           // ring reads done
    const int group_stride = pb * SP_PITCH;
    const bool counting = args.cnt_row != nullptr;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
        if (WN == 1 || wn == h) {                              // (4 x 2 grid: the column-wave that holds this pass's 32 columns)
#pragma unroll
            for (int mt = 0; mt < MTS; ++mt) {
                const int plane = args.mt_plane[wm][mt];       // wave-uniform
                if (plane < 0) continue;
                const int lp0 = args.mt_j[wm][mt] * 16 + lg * 4;
#pragma unroll
                for (int nq = 0; nq < 2; ++nq)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float val;
                        if constexpr (WN == 1) val = h == 0 ? acc[mt][nq][r] : acc[mt][2 + nq][r];
                        else val = acc[mt][nq][r];
                        if (lp0 + r < pb) tile[(plane * pb + lp0 + r) * SP_PITCH + nq * 16 + lr] = val;
                    }
            }
        }
        __syncthreads();
#ifdef SNN_EXP_TIMELINE
        if (h == 0) SP_TL_STAMP(7);
#endif
        const int word0 = (nb * 64 + h * 32) >> 5;
        const int par = lane >> 5, col = lane & 31;
        // position pairs per wave and iteration (see sp_lif_fixed): two up to T = 10, one beyond (registers: T - 1 period sums per neuron);
        // the FAT shape's waves have the registers for twice that - and half the waves to hide the recurrence's latencies with
        constexpr int NP_SHORT = FAT ? 4 : 2, NP_LONG = FAT ? 2 : 1;
        auto lif_pass = [&](auto np_c, auto count_c) __attribute__((always_inline)) {
        constexpr int NP = decltype(np_c)::value;
        constexpr bool COUNT = decltype(count_c)::value;
        for (int pp0 = wave; 2 * pp0 < pb; pp0 += NWAVES * NP) {
            if (m0 + 2 * pp0 >= M) break;
            uint32_t my0[NP], my1[NP], cnt_lo[NP], cnt_hi[NP];
            const float* src[NP];
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                const int pi = 2 * (pp0 + NWAVES * u) + par;
                const bool live = pi < pb && m0 + pi < M;
                my0[u] = 0; my1[u] = 0; cnt_lo[u] = 0; cnt_hi[u] = 0;
                src[u] = tile + (live ? pi : 2 * pp0) * SP_PITCH + col;    // (dead lanes / pairs recompute a live row: never stored)
            }
#define SP_T(n) case n: sp_lif_fixed<n, CONV ? 1 : 2, NP, COUNT>(src, group_stride, args.p, my0, my1, cnt_lo, cnt_hi); break;
            if (NP == 1 && !CONV && args.epi_general) {               // (block-uniform; linear layers only: the conv's launcher keeps to the fixed grid)
                if constexpr (NP == 1 && !CONV) sp_lif_general<COUNT>(src[0], group_stride, args.p, T, Tc, args.div, lane, my0[0], my1[0], cnt_lo[0], cnt_hi[0]);
            } else if constexpr (COUNT) {
                switch (T) { SP_T(5) SP_T(6) SP_T(7) SP_T(8) SP_T(9) SP_T(10) SP_T(11) SP_T(12) SP_T(13) SP_T(14) SP_T(15) SP_T(16) default: break; }
            } else if constexpr (NP == NP_SHORT) {
                switch (T) { SP_T(5) SP_T(6) SP_T(7) SP_T(8) SP_T(9) SP_T(10) default: break; }
            } else {
                switch (T) { SP_T(11) SP_T(12) SP_T(13) SP_T(14) SP_T(15) SP_T(16) default: break; }
            }
#undef SP_T
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                const int pp = pp0 + NWAVES * u;
                if (2 * pp >= pb || m0 + 2 * pp >= M) continue;
                const bool odd_ok = 2 * pp + 1 < pb && m0 + 2 * pp + 1 < M;
                if (COUNT && lane == 0) {                                  // (dead odd rows recompute the even one: not counted)
                    if (cnt_lo[u]) atomicAdd(args.cnt_row + m0 + 2 * pp, cnt_lo[u]);
                    if (odd_ok && cnt_hi[u]) atomicAdd(args.cnt_row + m0 + 2 * pp + 1, cnt_hi[u]);
                }
                if (lane < T) {
                    if (!CONV) {                                           // linear layer: word-major spike planes [T][word][RoI] (fc6 -> fc7)
                        uint32_t* dst = args.spk + (size_t)lane * args.spk_stride + (size_t)word0 * M + (m0 + 2 * pp);
                        dst[0] = my0[u];
                        if (odd_ok) dst[1] = my1[u];
                    } else if (args.out_split) {
                        uint32_t* dst = args.spk + (size_t)lane * args.spk_stride + ((size_t)(word0 >> 2) * M + m0 + 2 * pp) * 4 + (word0 & 3);
                        dst[0] = my0[u];
                        if (odd_ok) dst[4] = my1[u];
                    } else {
                        uint32_t* dst = args.spk + (size_t)lane * args.spk_stride + (size_t)(m0 + 2 * pp) * (Np >> 5) + word0;
                        dst[0] = my0[u];
                        if (odd_ok) dst[Np >> 5] = my1[u];
                    }
                }
            }
        }
        };
        if (args.epi_general) {                                    // (linear layers outside the straight-line grid: one run-time recurrence per lane)
            if (counting) lif_pass(std::integral_constant<int, 1>{}, std::true_type{});
            else lif_pass(std::integral_constant<int, 1>{}, std::false_type{});
        } else if (counting) {                                     // (the counters take the registers of one recurrence)
            lif_pass(std::integral_constant<int, NP_LONG>{}, std::true_type{});
        } else {
            if (T <= 10) lif_pass(std::integral_constant<int, NP_SHORT>{}, std::false_type{});
            else lif_pass(std::integral_constant<int, NP_LONG>{}, std::false_type{});
        }
#ifdef SNN_EXP_TIMELINE
        if (h == 0) SP_TL_STAMP(3);
#endif
    }
#ifdef SNN_EXP_TIMELINE
    if (tid == 0) {
        unsigned long long tl_exit;
        uint32_t hw, xcc;
        asm volatile("s_memrealtime %0\n\ts_getreg_b32 %1, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %2, hwreg(HW_REG_XCC_ID)\n\ts_waitcnt lgkmcnt(0)"
                     : "=s"(tl_exit), "=s"(hw), "=s"(xcc) :: "memory");
        unsigned long long* o = args.tl + (size_t)blockIdx.x * 8;       // (behind the compressed planes: tools/sparse_timeline.py allocates more)
        o[4] = tl_exit; o[5] = hw; o[6] = xcc;                          // (o[7] != 0 marks the record)
    }
#endif
}
