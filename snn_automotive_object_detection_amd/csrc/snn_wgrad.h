// Readout weight gradients (include/snn_hip.h: snn_li_heads_wgrad): the exact gradients of the two LI heads' weights from the
// spike planes a head pass left behind.
//
// The LI cell and the bias-free 1x1 conv / linear in front of it are linear, and the hidden spike train does not depend on the readout weights:
//     out[r][j] = sum_k W[j][k] S[r][k],   S[r][k] = sum_{t < T'} kappa_t bit_t(r, k)      (kappa = li_kappa(p, T').last, as the forward folds it)
// so  dL/dW[j][k] = sum_r g[r][j] S[r][k]  with g = dL/dout.  No surrogate, no threshold: the only roundings are fp32 sums.
//
// Two launches, no floating-point atomics, the same bits on every run:
//   k_li_wgrad_partial  grid (slabs, chunks of WG_WORDS words, groups of WG_JW outputs).  A work-group owns a slab of rows - the tiles slab,
//                       slab + n_slabs, .. of WG_ROWS rows - one chunk of 128 columns and 16 outputs.  Per tile:
//                         A  thread = (row, word), addressed as the taps address the three layouts (tap_word; a wave's loads are contiguous in
//                            each of them): its T' words are folded bit by bit into 32 fp32 sums S[row][32 w + b], t ascending, and stored to LDS
//                            column-major; bits at or above n_cols are masked off, words past them are never loaded;
//                         -  the tile's 64 x 16 gradients go to LDS (zero for rows past the end and outputs past NA + NB);
//                         B  thread = (column, half of the outputs): acc[8] += g[row][j] * S[row][column] over the tile's rows, ascending
//                            (S: one conflict-free LDS read per row; g: two 16-byte LDS broadcasts).
//                       The accumulators live in registers over all tiles of the slab and leave once: part[slab][j][column].
//   k_li_wgrad_reduce   thread = (16 consecutive elements, sixteenth of the slabs): sums its slabs in ascending order, the sixteen partial sums
//                       meet in LDS and are added in ascending order; gw = or += the sum.  Every element of gw_a / gw_b is written by this
//                       launch, so accumulate = 0 needs nothing cleared in front.
// Every element of `part` the second launch reads is written by the first (a slab is never empty: n_slabs <= tiles), so the scratch may
// hold anything.  FLOPs are trivial at both head shapes (15 and 45 outputs); the cost is the plane read and the bit fold of phase A, which
// a matrix-core product would not shorten: the product runs on the VALU.
#ifndef SNN_WGRAD_H
#define SNN_WGRAD_H

#define WG_ROWS 64                   // rows of a tile
#define WG_WORDS 4                   // words of a column chunk (one block of a SPLIT4 plane)
#define WG_COLS (32 * WG_WORDS)
#define WG_JT 8                      // outputs per thread
#define WG_JW (2 * WG_JT)            // outputs per work-group: two halves of 128 threads
#define WG_PITCH (WG_ROWS + 1)
#define WG_MAX_SLABS 512
#define WG_MAX_OUT 480               // NA + NB (96 classes)
#define WG_RED 16                    // the reduction's split of the slabs, and elements per work-group

struct WgradArgs {
    TapView v;
    const float* ga;                 // [rows][NA]
    const float* gb;                 // [rows][NB]
    int NA, NB, n_cols, T;
    int tiles, n_slabs;
    float kappa[SNN_MAX_STEPS];      // li_kappa(p, T').last
};

__global__ __launch_bounds__(256) void k_li_wgrad_partial(const WgradArgs a, float* __restrict__ part) {
    __shared__ float S[WG_COLS][WG_PITCH];
    __shared__ __attribute__((aligned(16))) float G[WG_ROWS][WG_JW];
    __shared__ float kap[SNN_MAX_STEPS];
    const int tid = threadIdx.x, slab = blockIdx.x, w0 = blockIdx.y * WG_WORDS, j0 = blockIdx.z * WG_JW;
    if (tid < SNN_MAX_STEPS) kap[tid] = a.kappa[tid];
    // phase A: (row, word) of the tile, neighbours in memory in the view's layout
    int r, w;
    if (a.v.layout == TAP_LAYOUT_WORD_MAJOR) { w = tid >> 6; r = tid & 63; }
    else { r = tid >> 2; w = tid & 3; }
    const int n_words = (a.n_cols + 31) >> 5, wg = w0 + w;                      // (n_cols <= 32 * words: a word below n_words exists)
    const uint32_t mask = wg >= n_words ? 0u : (wg == n_words - 1 && (a.n_cols & 31)) ? (1u << (a.n_cols & 31)) - 1u : ~0u;
    // phase B: (column, half of the outputs)
    const int c = tid & (WG_COLS - 1), h = tid >> 7;
    float acc[WG_JT];
#pragma unroll
    for (int k = 0; k < WG_JT; ++k) acc[k] = 0.0f;
    __syncthreads();
    for (int tile = slab; tile < a.tiles; tile += a.n_slabs) {
        const long long r0 = (long long)tile * WG_ROWS;
        const int nr = (int)(a.v.rows - r0 < WG_ROWS ? a.v.rows - r0 : WG_ROWS);
        float s[32];
#pragma unroll
        for (int b = 0; b < 32; ++b) s[b] = 0.0f;
        if (r < nr && mask) {
            const uint32_t* src = a.v.planes + tap_word(a.v, r0 + r, wg);
            for (int t = 0; t < a.T; ++t) {
                const uint32_t x = src[(size_t)t * a.v.step_stride] & mask;
                const float kt = kap[t];
#pragma unroll
                for (int b = 0; b < 32; ++b) s[b] += ((x >> b) & 1u) ? kt : 0.0f;
            }
        }
#pragma unroll
        for (int b = 0; b < 32; ++b) S[32 * w + b][r] = s[b];
        for (int e = tid; e < WG_ROWS * WG_JW; e += 256) {
            const int gr = e / WG_JW, jj = e % WG_JW, j = j0 + jj;
            float g = 0.0f;
            if (gr < nr) {
                if (j < a.NA) g = a.ga[(size_t)(r0 + gr) * a.NA + j];
                else if (j < a.NA + a.NB) g = a.gb[(size_t)(r0 + gr) * a.NB + (j - a.NA)];
            }
            G[gr][jj] = g;
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < WG_ROWS; ++rr) {
            const float sv = S[c][rr];
            const float4 ga = *reinterpret_cast<const float4*>(&G[rr][h * WG_JT]), gb = *reinterpret_cast<const float4*>(&G[rr][h * WG_JT + 4]);
            acc[0] = fmaf(ga.x, sv, acc[0]); acc[1] = fmaf(ga.y, sv, acc[1]); acc[2] = fmaf(ga.z, sv, acc[2]); acc[3] = fmaf(ga.w, sv, acc[3]);
            acc[4] = fmaf(gb.x, sv, acc[4]); acc[5] = fmaf(gb.y, sv, acc[5]); acc[6] = fmaf(gb.z, sv, acc[6]); acc[7] = fmaf(gb.w, sv, acc[7]);
        }
        __syncthreads();
    }
    const int col = 32 * w0 + c, NO = a.NA + a.NB;
    if (col < a.n_cols) {
#pragma unroll
        for (int k = 0; k < WG_JT; ++k) {
            const int j = j0 + h * WG_JT + k;
            if (j < NO) part[((size_t)slab * NO + j) * a.n_cols + col] = acc[k];
        }
    }
}

// part [n_slabs][NA + NB][n_cols] -> gw_a [NA][n_cols], gw_b [NB][n_cols]; grid: ceil((NA + NB) n_cols / WG_RED)
__global__ __launch_bounds__(256) void k_li_wgrad_reduce(const float* __restrict__ part, int n_slabs, int NA, int NB, int n_cols, float* __restrict__ gw_a,
                                                         float* __restrict__ gw_b, int accumulate) {
    __shared__ float red[WG_RED][WG_RED + 1];
    const int e = threadIdx.x & (WG_RED - 1), q = threadIdx.x / WG_RED;
    const size_t n = (size_t)(NA + NB) * n_cols, i = (size_t)blockIdx.x * WG_RED + e;
    const int per = (n_slabs + WG_RED - 1) / WG_RED;
    float s = 0.0f;
    if (i < n) {
        const int s1 = min(n_slabs, (q + 1) * per);
        for (int sl = q * per; sl < s1; ++sl) s += part[(size_t)sl * n + i];
    }
    red[q][e] = s;
    __syncthreads();
    if (q == 0 && i < n) {
        float t = red[0][e];
#pragma unroll
        for (int k = 1; k < WG_RED; ++k) t += red[k][e];
        const size_t na = (size_t)NA * n_cols;
        float* dst = i < na ? gw_a + i : gw_b + (i - na);
        *dst = accumulate ? *dst + t : t;
    }
}

#endif  // SNN_WGRAD_H
