// The text of the two row encoders that exist for fp32 and for half-precision features (see snn_encode.h, which includes this file once per
// element kind; no include guard).  The includer defines, and this file undefines at its end:
//   ENC_HALF             0: fp32 features, 1: fp16 / bf16 features (elements of type FT = feat_f16 | feat_bf16, widened in registers)
//   ENC_KERNEL(stem)     name of the __global__: stem (fp32) or stem_h (typed)
//   ENC_TEMPLATE(...)    its template header: template <...> (fp32) or template <..., typename FT> (typed)
//   ENC_FT               element type of the features: float or FT
// An element load is feat_widen(src[..]) (the identity on float).
// (Instantiated as text and not through a shared __device__ body: behind a body function the optimiser schedules the fp32 kernels differently,
// and their measured instruction streams are to stay what they were: tools/symbol_diff.py, profiles/encoder_text_symbol_diff.txt.)

// K1b'': the same encoder writing WORD-MAJOR planes [T][Dw][R] (what the linear-layer kernels stream best): a work-group takes
// 32 rows x 8 words (32 x 1 KB of x, 16-byte coalesced loads through LDS), thread = (row tid & 31, word tid >> 5), so the 32
// lanes of a half-wave store 32 consecutive rows of one word plane: 128-byte runs.  D % 32 == 0, x 16-byte aligned.
ENC_TEMPLATE(int EM)
__global__ __launch_bounds__(256) void ENC_KERNEL(k_encode_rows_wm)(const ENC_FT* __restrict__ x, int R, int D, int T, NeuronP p, const EncTh eth,
                                                        uint32_t* __restrict__ planes, size_t plane_stride) {
    constexpr bool ZR = EM != ENC_GENERIC;
    __shared__ __attribute__((aligned(16))) float tile[32 * ENC_WM_PITCH];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * 32, w0 = blockIdx.x * 8;
#if ENC_HALF                                                    // (eight halves per 16-byte piece against four floats; x 16-byte aligned as well)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = tid + 256 * j;                            // 16-byte piece: row q / 32, halves 8 (q % 32) .. of the 256-element run, widened on the way into LDS
        const int row = q >> 5, col = w0 * 32 + (q & 31) * 8;
        u32x4 h = {0u, 0u, 0u, 0u};
        if (r0 + row < R && col < D) h = *reinterpret_cast<const u32x4*>(x + (size_t)(r0 + row) * D + col);
        float* d = tile + row * ENC_WM_PITCH + (q & 31) * 8;
        const f32x4 lo = {feat_widen_bits<FT>(h.x & 0xffffu), feat_widen_bits<FT>(h.x >> 16), feat_widen_bits<FT>(h.y & 0xffffu), feat_widen_bits<FT>(h.y >> 16)};
        const f32x4 hi = {feat_widen_bits<FT>(h.z & 0xffffu), feat_widen_bits<FT>(h.z >> 16), feat_widen_bits<FT>(h.w & 0xffffu), feat_widen_bits<FT>(h.w >> 16)};
        *reinterpret_cast<f32x4*>(d) = lo;
        *reinterpret_cast<f32x4*>(d + 4) = hi;
    }
#else
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int q = tid + 256 * j;                            // 16-byte piece: row q / 64, floats 4 (q % 64) .. of the 256-float run
        const int row = q >> 6, col = w0 * 32 + (q & 63) * 4;
        f32x4 v4 = {0.f, 0.f, 0.f, 0.f};
        if (r0 + row < R && col < D) v4 = *reinterpret_cast<const f32x4*>(x + (size_t)(r0 + row) * D + col);
        *reinterpret_cast<f32x4*>(tile + row * ENC_WM_PITCH + (q & 63) * 4) = v4;
    }
#endif
    __syncthreads();
    const int row = tid & 31, wd = tid >> 5;
    if (r0 + row >= R || (w0 + wd) * 32 >= D) return;
    float xv[32], v[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(tile + row * ENC_WM_PITCH + wd * 32 + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) { xv[4 * q + r] = t4[r]; v[4 * q + r] = 0.0f; }      // v = 0: faster_rcnn.py:484
    }
    uint32_t* dst = planes + (size_t)(w0 + wd) * R + r0 + row;
    uint32_t prev = 0;
    for (int t = 0; t < T; ++t) {
        uint32_t word = 0;
        if (EM == ENC_QUANT) {                      // period planes by thresholds (snn_common.h)
            const float th = eth.th[t];
#pragma unroll
            for (int b = 31; b >= 0; --b) enc_quant_word(xv[b], th, word);
            const uint32_t cum = word;
            word = cum & ~prev;
            prev = cum;
        } else {
#pragma unroll
            for (int b = 31; b >= 0; --b) enc_step_word<ZR>(xv[b], v[b], p, word);          // bit 31 first
        }
        dst[(size_t)t * plane_stride] = word;
    }
}

// K1d (round 5): the detector's encoder for the structured-sparse fc6 in ONE launch - period planes by thresholds, written straight in
// fc6's reduction order k' = bin * C + channel (what k_permute_planes made of the reference-order planes) and, for the planes e_3 ..,
// COMPRESSED (what k_compress_planes made of those): three launches and two HBM round trips of the planes become one.
// x [R][C * S] fp32 in the reference's flatten order k = c * S + bin (faster_rcnn.py:473).  Block = ENCP_RB RoIs x 64 channels (two channel
// blocks cb = 2 cp, 2 cp + 1: a compressed step is a pair of words (bin, cb), (bin, cb + 1)).  Encode: a wave takes (RoI, channel block)
// tasks, lane = bin (S of 64 lanes), the lane's 32 channels are 32 loads at stride S floats - every load instruction reads one S-float run of
// the RoI's row - and the T words go to LDS [t][cb][RoI][bin] (odd pitch S: conflict-free both ways).  Store: thread = (RoI, item): the dense planes' words as they are, a sparse
// plane's pair through sp_compress_pair - runs of ENCP_RB consecutive RoIs of one word plane / array.
ENC_TEMPLATE(int S, int RB, int NW)                   // NW waves per block (4 or 8: 2 RB tasks over NW waves, two at a time)
__global__ __launch_bounds__(64 * NW) void ENC_KERNEL(k_encode_rows_perm)(const ENC_FT* __restrict__ x, int R, int C, int T, int nd, const EncTh eth,
                                                          uint32_t* __restrict__ planes, uint32_t* __restrict__ cmp) {
    static_assert(S <= 64, "one lane per bin");
    extern __shared__ uint32_t pw[];                          // [min(T, TMAX)][2][RB][S]
    constexpr int TMAX = ENCP_LDS_WORDS / (2 * S * RB);
    static_assert((2 * RB) % (2 * NW) == 0, "tasks two at a time per wave");
    __shared__ uint16_t code[256];
    if (threadIdx.x < 256) code[threadIdx.x] = sp_byte_code(threadIdx.x);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * RB, cp = blockIdx.y, cbn = C / 32, D = C * S, Dw = D / 32;
    const size_t plane_words = (size_t)Dw * R, cmp_plane = (size_t)(Dw / 2) * SP_A_ARR * R;
    for (int t0 = 0; t0 < T; t0 += TMAX) {
        const int tn = min(TMAX, T - t0);
        if (t0) __syncthreads();
        // ---- encode: tasks (RoI, cb) over the waves; the next task's 32 loads are in flight while this one's words are formed
        auto load_task = [&](float (&xv)[32], const int task) __attribute__((always_inline)) {
            const int row = r0 + (task >> 1), cb = task & 1;
            const ENC_FT* src = x + (size_t)min(row, R - 1) * D + (size_t)((2 * cp + cb) * 32) * S + min(lane, S - 1);
#ifdef SNN_EXP_ENCP_NOLOAD                             // (timing experiments - wrong results: which phase bounds the launch?)
#pragma unroll
            for (int j = 0; j < 32; ++j) xv[j] = (float)(j + lane) * 0.01f + (float)((size_t)src & 4);
#else
#pragma unroll
            for (int j = 0; j < 32; ++j) xv[j] = feat_widen(src[j * S]);
#endif
        };
        auto encode_task = [&](const float (&xv)[32], const int task) __attribute__((always_inline)) {
            const int rl = task >> 1, cb = task & 1;
            if (lane < S) {
                uint32_t prev = 0;
                for (int t = 0; t < t0 + tn; ++t) {          // (cumulative words from step 0: a later pass re-derives what it needs)
                    uint32_t word = 0;
                    const float th = eth.th[t];
#ifdef SNN_EXP_ENCP_NOENC
                    word = __float_as_uint(xv[t & 31] + xv[(t + 7) & 31]) & (th > 0.0f ? 0x11111111u : 0u);
#else
#pragma unroll
                    for (int j = 31; j >= 0; --j) enc_quant_word(xv[j], th, word);
#endif
                    const uint32_t cum = word;
                    word = cum & ~prev;
                    prev = cum;
                    if (t >= t0) pw[(((t - t0) * 2 + cb) * RB + rl) * S + lane] = word;
                }
            }
        };
        float xa[32], xb[32];
        load_task(xa, wave);
#pragma unroll 1
        for (int task = wave; task < 2 * RB; task += 2 * NW) {     // (2 RB / NW tasks per wave: even)
            load_task(xb, task + NW);
            encode_task(xa, task);
            if (task + 2 * NW < 2 * RB) load_task(xa, task + 2 * NW);
            encode_task(xb, task + NW);
        }
        __syncthreads();
        // ---- store: thread = (RoI tid % RB, item tid / RB)
        const int rl = tid & (RB - 1), row = r0 + rl;                    // (RB = 8 or 16)
#ifdef SNN_EXP_ENCP_NOSTORE
        if (row < R && pw[tid] == 0x12345678u) {
#else
        if (row < R) {
#endif
            for (int t = t0; t < t0 + tn; ++t) {
                const uint32_t* pt = pw + (size_t)(t - t0) * 2 * S * RB;
                if (t < nd || !cmp) {                         // raw words (bin, cb) -> word plane bin * cbn + 2 cp + cb
                    for (int it = tid / RB; it < 2 * S; it += 64 * NW / RB) {
                        const int cb = it / S, bin = it % S;
                        planes[(size_t)t * plane_words + (size_t)(bin * cbn + 2 * cp + cb) * R + row] = pt[(cb * RB + rl) * S + bin];
                    }
                } else {                                      // compressed step (bin, cp): pair index (bin * cbn + 2 cp) / 2
                    for (int bin = tid / RB; bin < S; bin += 64 * NW / RB) {
                        uint32_t c4[4];
                        sp_compress_pair(pt[rl * S + bin], pt[(RB + rl) * S + bin], code, c4);
                        uint32_t* o = cmp + (size_t)(t - nd) * cmp_plane + (size_t)(bin * (cbn / 2) + cp) * SP_A_ARR * R + row;
#pragma unroll
                        for (int j = 0; j < SP_A_ARR; ++j) o[(size_t)j * R] = c4[j];
                    }
                }
            }
        }
    }
}

#undef ENC_HALF
#undef ENC_KERNEL
#undef ENC_TEMPLATE
#undef ENC_FT
