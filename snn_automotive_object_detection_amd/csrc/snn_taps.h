// Spike taps (include/snn_hip.h: snn_planes_counts, snn_planes_raster_nchw, snn_planes_raster_rows): the hidden LIF layers'
// bit-planes, read where a head pass left them in the caller's workspace, as integer activity statistics and as byte rasters.
//
// A plane set is T steps of `rows` x `words` 32-bit words (bit b of word w = spike of column 32 w + b) in one of three layouts; every
// kernel here addresses all three itself (tap_word), so no re-layout launch runs in front:
//   SNN_PLANES_ROWS        [T][rows][words]
//   SNN_PLANES_SPLIT4      [T][words / 4][rows][4]     (the RPN's shared LIF at C = 256: blocks of four words)
//   SNN_PLANES_WORD_MAJOR  [T][words][rows]            (lif6 of the fused bf16x3 detector head)
// A work-group takes a tile of TAP_ROWS rows and walks its words in the order the layout keeps them in memory (tap_elem), so that the
// loads of a wave are contiguous in every layout.
//
// Counting scheme: integer atomics, summed on chip first.  A work-group belongs to ONE group (a contiguous row range: an image of a level,
// an image's RoIs); it keeps the group's per-column and per-step counters in LDS over all its tiles and adds them to memory once, one
// atomic per non-zero counter.  Per-row sums go through LDS too and are stored, not added (a row belongs to one tile).  Every sum is an
// integer, so the order of the adds does not matter: the results are exact and the same on every run.
//
// Rasters: a tile of TAP_ROWS rows x TAP_TW words is staged in LDS and written out so that the stores of a wave are contiguous - along a
// row's columns (raster_rows), or along H x W of one channel (raster_nchw: the bit transposition - a wave holds one word of 64 positions,
// 32 ballots turn it into 32 channel masks of 64 positions each).  Sixteen bits become sixteen bytes per store where the output is aligned
// for it, single bytes (still contiguous per wave) where it is not.
#ifndef SNN_TAPS_H
#define SNN_TAPS_H

#define TAP_ROWS 64                  // rows (positions, RoIs) of a tile
#define TAP_TW 4                     // words of a raster tile (one block of a SPLIT4 plane)
#define TAP_MAX_GROUPS 512           // groups of one snn_planes_counts call (the row starts travel as kernel arguments)
#define TAP_MAX_WORDS 256            // words per row (8192 columns: 32 KB of per-column counters in LDS)
#define TAP_LAYOUT_ROWS 0            // == SNN_PLANES_ROWS / _SPLIT4 / _WORD_MAJOR (static_assert in snn_kernels.hip)
#define TAP_LAYOUT_SPLIT4 1
#define TAP_LAYOUT_WORD_MAJOR 2

struct TapView {
    const uint32_t* planes;          // workspace + view.offset_bytes
    unsigned long long step_stride;  // words from one step's plane to the next
    long long rows;
    int words, layout;
};
struct TapGroups {
    int n;
    int start[TAP_MAX_GROUPS + 1];   // group g = rows start[g] .. start[g + 1] - 1 (non-decreasing)
};

// word w of `row` inside one step's plane
__device__ __forceinline__ size_t tap_word(const TapView& v, long long row, int w) {
    if (v.layout == TAP_LAYOUT_SPLIT4) return ((size_t)(w >> 2) * v.rows + row) * 4 + (w & 3);
    if (v.layout == TAP_LAYOUT_WORD_MAJOR) return (size_t)w * v.rows + row;
    return (size_t)row * v.words + w;
}

// element e of a tile of nr rows x nw words -> (row, word) of the tile, consecutive e being neighbours in memory
__device__ __forceinline__ void tap_elem(int layout, int e, int nr, int nw, int* r, int* w) {
    if (layout == TAP_LAYOUT_WORD_MAJOR) { *w = e / nr; *r = e - *w * nr; }
    else if (layout == TAP_LAYOUT_SPLIT4) { const int q = e / (4 * nr), i = e - q * 4 * nr; *r = i >> 2; *w = q * 4 + (i & 3); }      // (nw % 4 == 0)
    else { *r = e / nw; *w = e - *r * nw; }
}

// ---- counts ------------------------------------------------------------------------------------------------------------------------
// grid (tiles of the largest group, capped; groups); LDS: per-step counters [32] (64-bit), per-row sums [TAP_ROWS], per-column counters
// [32 * words].  per_step [T][n_groups] / per_col [n_groups][n_cols] / per_row [rows] were zeroed on the stream by the caller; any of them null:
// not wanted.  Bits at or above n_cols are masked off before anything is counted.
#define TAP_COUNTS_LDS(words) ((size_t)(32 * 8 + TAP_ROWS * 4) + (size_t)(words) * 32 * 4)
// the call's own clearing launch (a kernel, not memset nodes: the same work eagerly and in a replayed graph); null: not wanted
__global__ __launch_bounds__(256) void k_planes_clear(unsigned long long* __restrict__ per_step, size_t n_step, uint32_t* __restrict__ per_col,
                                                      size_t n_col, uint32_t* __restrict__ per_row, size_t n_row) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (per_step) for (size_t i = i0; i < n_step; i += stride) per_step[i] = 0;
    if (per_col) for (size_t i = i0; i < n_col; i += stride) per_col[i] = 0;
    if (per_row) for (size_t i = i0; i < n_row; i += stride) per_row[i] = 0;
}
__global__ __launch_bounds__(256) void k_planes_counts(const TapView v, const TapGroups g, int n_cols, int T,
                                                       unsigned long long* __restrict__ per_step, uint32_t* __restrict__ per_col,
                                                       uint32_t* __restrict__ per_row) {
    extern __shared__ unsigned long long tap_lds[];
    unsigned long long* const step = tap_lds;                                   // [32]
    uint32_t* const rsum = reinterpret_cast<uint32_t*>(tap_lds + 32);           // [TAP_ROWS]
    uint32_t* const col = rsum + TAP_ROWS;                                      // [32 * words]
    const int grp = blockIdx.y, tid = threadIdx.x;
    const long long g0 = g.start[grp], g1 = g.start[grp + 1];
    const int tiles = (int)((g1 - g0 + TAP_ROWS - 1) / TAP_ROWS);
    if ((int)blockIdx.x >= tiles) return;                                       // (block-uniform, in front of every barrier)
    const int words = v.words, n_words = (n_cols + 31) >> 5;                   // words that hold a counted column
    for (int c = tid; c < 32 * words; c += 256) col[c] = 0;
    if (tid < 32) step[tid] = 0;
    const uint32_t last_mask = (n_cols & 31) ? (1u << (n_cols & 31)) - 1u : ~0u;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r0 = g0 + (long long)tile * TAP_ROWS;
        const int nr = (int)(g1 - r0 < TAP_ROWS ? g1 - r0 : TAP_ROWS);
        if (tid < TAP_ROWS) rsum[tid] = 0;
        __syncthreads();
        for (int e = tid; e < nr * words; e += 256) {
            int r, w;
            tap_elem(v.layout, e, nr, words, &r, &w);
            if (w >= n_words) continue;
            const uint32_t mask = w == n_words - 1 ? last_mask : ~0u;
            const uint32_t* src = v.planes + tap_word(v, r0 + r, w);
            uint32_t acc = 0;
            for (int t = 0; t < T; ++t) {
                uint32_t x = src[(size_t)t * v.step_stride] & mask;
                const uint32_t pc = __popc(x);
                if (!pc) continue;
                acc += pc;
                if (per_step) atomicAdd(&step[t], (unsigned long long)pc);
                if (per_col)
                    while (x) {
                        atomicAdd(&col[32 * w + (__ffs(x) - 1)], 1u);
                        x &= x - 1;
                    }
            }
            if (acc) atomicAdd(&rsum[r], acc);
        }
        __syncthreads();
        if (per_row && tid < nr) per_row[r0 + tid] = rsum[tid];
        __syncthreads();
    }
    if (per_col)
        for (int c = tid; c < n_cols; c += 256)
            if (col[c]) atomicAdd(&per_col[(size_t)grp * n_cols + c], col[c]);
    if (per_step && tid < T && step[tid]) atomicAdd(&per_step[(size_t)tid * g.n + grp], step[tid]);
}

// ---- rasters -----------------------------------------------------------------------------------------------------------------------
#define TAP_PITCH (TAP_ROWS + 1)
// words w0 .. w0 + 3 of rows r0 .. r0 + nr - 1 of one step's plane -> tile[word][row]; zero outside the plane (256 threads, one word each)
__device__ __forceinline__ void tap_stage(const TapView& v, const uint32_t* __restrict__ plane, long long r0, int nr, int w0,
                                          uint32_t (*tile)[TAP_PITCH]) {
    const int e = threadIdx.x;
    int r, w;
    if (v.layout == TAP_LAYOUT_WORD_MAJOR) { w = e >> 6; r = e & 63; }
    else { r = e >> 2; w = e & 3; }
    uint32_t x = 0;
    if (r < nr && w0 + w < v.words) x = plane[tap_word(v, r0 + r, w0 + w)];
    tile[w][r] = x;
}
// four bits -> four bytes {0, 1}, lowest bit first
__device__ __forceinline__ uint32_t tap_spread4(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }
__device__ __forceinline__ uint4 tap_spread16(uint32_t h) {
    return make_uint4(tap_spread4(h & 15u), tap_spread4((h >> 4) & 15u), tap_spread4((h >> 8) & 15u), tap_spread4((h >> 12) & 15u));
}

// out [T][rows][n_cols] bytes.  grid (row tiles, word groups, T); vec: n_cols % 16 == 0 and out 16-byte aligned
__global__ __launch_bounds__(256) void k_planes_raster_rows(const TapView v, int n_cols, uint8_t* __restrict__ out, int vec) {
    __shared__ uint32_t tile[TAP_TW][TAP_PITCH];
    const long long r0 = (long long)blockIdx.x * TAP_ROWS;
    const int nr = (int)(v.rows - r0 < TAP_ROWS ? v.rows - r0 : TAP_ROWS), w0 = blockIdx.y * TAP_TW, t = blockIdx.z;
    tap_stage(v, v.planes + (size_t)t * v.step_stride, r0, nr, w0, tile);
    __syncthreads();
    uint8_t* const o = out + ((size_t)t * v.rows + r0) * n_cols;
    if (vec) {
        for (int k = threadIdx.x; k < TAP_ROWS * 8; k += 256) {
            const int r = k >> 3, q = k & 7, c = 32 * w0 + 16 * q;
            if (r < nr && c < n_cols)
                *reinterpret_cast<uint4*>(o + (size_t)r * n_cols + c) = tap_spread16((tile[q >> 1][r] >> (16 * (q & 1))) & 0xffffu);
        }
    } else {
        for (int k = threadIdx.x; k < TAP_ROWS * 32 * TAP_TW; k += 256) {
            const int r = k >> 7, cl = k & 127, c = 32 * w0 + cl;
            if (r < nr && c < n_cols) o[(size_t)r * n_cols + c] = (uint8_t)((tile[cl >> 5][r] >> (cl & 31)) & 1u);
        }
    }
}

// out [T][N][C][H][W] bytes from rows row0 + (n H + y) W + x of the view: position-major bits -> channel-major bytes.
// grid (position tiles of an image, word groups, T * N); vec: H W % 16 == 0 and out 16-byte aligned
__global__ __launch_bounds__(256) void k_planes_raster_nchw(const TapView v, long long row0, int N, int C, int HW, uint8_t* __restrict__ out,
                                                            int vec) {
    __shared__ uint32_t tile[TAP_TW][TAP_PITCH];
    __shared__ unsigned long long masks[32 * TAP_TW];              // [channel of the tile]: bit p = spike at position p0 + p
    const int p0 = blockIdx.x * TAP_ROWS, np = HW - p0 < TAP_ROWS ? HW - p0 : TAP_ROWS, w0 = blockIdx.y * TAP_TW;
    const int t = blockIdx.z / N, n = blockIdx.z - t * N;
    tap_stage(v, v.planes + (size_t)t * v.step_stride, row0 + (long long)n * HW + p0, np, w0, tile);
    __syncthreads();
    {
        const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;  // wave wv: word w0 + wv of the tile's 64 positions, one per lane
        const uint32_t x = tile[wv][lane];
        unsigned long long mine = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const unsigned long long m = __ballot((x >> b) & 1u);
            if (lane == b) mine = m;
        }
        if (lane < 32) masks[wv * 32 + lane] = mine;
    }
    __syncthreads();
    uint8_t* const o = out + ((size_t)blockIdx.z * C) * HW + p0;
    if (vec) {
        for (int k = threadIdx.x; k < 32 * TAP_TW * 4; k += 256) {
            const int cl = k >> 2, q = k & 3, c = 32 * w0 + cl;
            if (c < C && 16 * q < np)
                *reinterpret_cast<uint4*>(o + (size_t)c * HW + 16 * q) = tap_spread16((uint32_t)(masks[cl] >> (16 * q)) & 0xffffu);
        }
    } else {
        for (int k = threadIdx.x; k < 32 * TAP_TW * TAP_ROWS; k += 256) {
            const int cl = k >> 6, pos = k & 63, c = 32 * w0 + cl;
            if (c < C && pos < np) o[(size_t)c * HW + pos] = (uint8_t)((masks[cl] >> pos) & 1ull);
        }
    }
}

#endif  // SNN_TAPS_H
