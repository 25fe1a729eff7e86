// The spike-fed weight gradient on the bf16 matrix cores (include/snn_hip.h: snn_spike_wgrad_bf16x3):
//     gw[n][k] (+)= sum_m d_cur[m][n] bit(m, k)   over the M = T' rows reduction rows
// with every d_cur element split ON THE FLY into three bf16 values hi + mid + lo (the split k_bf16x3_split_check of snn_bf16x3.h describes:
// hi = rn(x), mid = rn(x - hi), lo = rn(x - hi - mid), exact for every fp32 of magnitude below 2^128 - 2^119 whose lowest set bit is >= 2^-133;
// at or above that magnitude hi rounds up to bf16 infinity and the whole output row becomes non-finite), the spike operand
// 0.0 / 1.0 in bf16, and fp32 accumulation of exact products inside v_mfma_f32_32x32x16_bf16.
//
//   k_wgrad3_partial   work-group = 4 waves = W3_TN x W3_TK = 128 outputs (d_cur columns n) x 256 inputs (plane bits k) of one slab of the
//                      reduction; a wave owns 64 x 128 of it (2 x 4 accumulators of 16 registers).  The reduction runs in stages of
//                      W3_MB = 32 rows:
//                        global -> registers   thread (n = tid & 127, g = tid >> 7) loads d_cur[m + 8 g' + j][n], j = 0 .. 7, for g' = g and g + 2:
//                                              16 loads, each contiguous over the lanes; thread (row = tid >> 3, w = tid & 7) one plane word
//                        split  -> LDS         ONCE PER WORK-GROUP: each thread splits its 16 elements and writes the three planes of 8
//                                              consecutive reduction rows as one 16-byte store each, image A_p[n][m] (80-byte rows: 64 + 16 of
//                                              padding, so 16 lanes with consecutive n hit 64 different banks); the plane word goes to the
//                                              TRANSPOSED word image Wt[w][m] (36-word rows)
//                        LDS -> matrix cores   the operand maps of v_mfma_f32_32x32x16_bf16 are then plain 16-byte reads:
//                                                A[i = lane & 31][kk = 8 (lane >> 5) + j] = d_p[n0 + i][m + kk]       one ds_read_b128 of A_p
//                                                B[kk = 8 (lane >> 5) + j][c = lane & 31] = bit c of Wt[w][m + kk]     two ds_read_b128 (all lanes of a half
//                                                                                          on one address) + 16 vector instructions, reused by 3 planes x 2 blocks
//                                                D[i][c]                                 = gw[n0 + i][32 w + c]
//                      Two LDS buffers: the loads of stage s + 1 are in flight under the products of stage s, its split follows them, one
//                      barrier per stage.  Planes reach an accumulator in the order lo, mid, hi - (lo + mid) + hi is exact, so a one-hot
//                      column returns d_cur bit for bit.  Indices past N, past a row's last plane word and past K are CLAMPED for the loads
//                      (they feed accumulators that are never stored); a row past the slab's end is loaded from the slab's last row and its
//                      gradient replaced by +0.  __launch_bounds__(256, 2): two work-groups per CU, 2 x 63744 bytes of LDS.
//                      One slab: the epilogue writes (or adds to) gw itself.  Several: it writes its valid partial tile to scratch[slab][n][k].
//   k_wgrad3_reduce    scratch [n_slabs][N K] -> gw [N K], the slabs in ascending order.
//
// The slab count is a pure function of (M, K, N): with tiles = ceil(N / 128) ceil(K / 256),
//     want = 1 if tiles >= 256 else min(ceil(256 / tiles), ceil(M / 256), 32);  rows per slab = ceil(ceil(M / want) / 32) 32;  slabs = ceil(M / rows per slab)
// - one when the output tiles alone fill the 256 CUs, otherwise as many as it takes to fill them.
// Rounding: against exact arithmetic every element is within (3 T' rows + slabs + 4) 2^-24 sum_m |d_cur[m][n]| bit(m, k) + T' rows 2^-133.
// No floating-point atomics, nothing cleared in front: every element read is written by a launch of the same call.
#ifndef SNN_SPIKE_WGRAD_X3_H
#define SNN_SPIKE_WGRAD_X3_H

#define W3_TN 128                    // outputs of a work-group's tile (2 waves x 2 blocks of 32)
#define W3_TK 256                    // inputs of a work-group's tile (2 waves x 4 plane words)
#define W3_MB 32                     // reduction rows per stage (2 matrix instructions deep)
#define W3_AROW 80                   // bytes of one (plane, output) row of the A image: W3_MB bf16 + 16 bytes of padding
#define W3_APLANE (W3_TN * W3_AROW)
#define W3_WROW 36                   // words of one row of the transposed word image: W3_MB + 4 of padding
#define W3_BUF (3 * W3_APLANE + (W3_TK / 32) * W3_WROW * 4)        // 31872 bytes; two of them per work-group
#define W3_SLAB_ROWS 256             // reduction rows a slab owns at least (but for the last)
#define W3_MAX_SLABS 32
#define W3_FILL 256                  // work-groups the grid should reach: the CUs of the device
#define W3_MAX_K 16384
#define W3_MAX_N 8192

struct Wgrad3Args {
    const uint32_t* a;               // [M][Kw]
    const float* d;                  // [M][ldd]
    long long M, slab_rows;          // reduction rows; rows of a slab (a multiple of W3_MB)
    int ldd, K, Kw, N, n_slabs, accumulate;
};

// the top 16 bits of the result are bf16 rn(u) (f2bf_rn of snn_bf16x3.h without its shift)
__device__ __forceinline__ uint32_t w3_rn(uint32_t u) { return u + 0x7FFFu + ((u >> 16) & 1u); }

// grid (tiles over K, tiles over N, slabs); part [n_slabs][N][K] (n_slabs > 1) or gw [N][K] (n_slabs == 1)
__global__ __launch_bounds__(256, 2) void k_wgrad3_partial(const Wgrad3Args g, float* __restrict__ part, float* __restrict__ gw) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][W3_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int n_base = blockIdx.y * W3_TN, w_base = blockIdx.x * (W3_TK / 32);
    const long long m0 = (long long)blockIdx.z * g.slab_rows, m1 = min(g.M, m0 + g.slab_rows);
    const int n_stages = (int)((m1 - m0 + W3_MB - 1) / W3_MB);
    // staging roles
    const int sn = tid & 127, sg = tid >> 7, wr = tid >> 3, ww = tid & 7;
    const int snc = min(n_base + sn, g.N - 1), wwc = min(w_base + ww, g.Kw - 1);
    float xs[2][8];
    uint32_t xw;
    auto load = [&](int stage) {
        const long long base = m0 + (long long)stage * W3_MB;
        if (base + W3_MB <= m1) {                                    // (wave-uniform) a stage wholly inside the slab: every load unconditional
            const float* dp = g.d + (size_t)(base + 8 * sg) * g.ldd + snc;
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int j = 0; j < 8; ++j) xs[q][j] = dp[(size_t)(16 * q + j) * g.ldd];
            xw = g.a[(size_t)(base + wr) * g.Kw + wwc];
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long long row = base + 8 * (sg + 2 * q) + j;
                    const bool in = row < m1;
                    const float x = g.d[(size_t)(in ? row : m1 - 1) * g.ldd + snc];
                    xs[q][j] = in ? x : 0.0f;
                }
            xw = g.a[(size_t)min(base + wr, m1 - 1) * g.Kw + wwc];
        }
    };
    auto store = [&](int buf) {
        unsigned char* img = lds[buf];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint32_t th[8], tm[8], tl[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = xs[q][j];
                th[j] = w3_rn(__float_as_uint(x));
                const float r1 = __fsub_rn(x, __uint_as_float(th[j] & 0xFFFF0000u));
                tm[j] = w3_rn(__float_as_uint(r1));
                const float r2 = __fsub_rn(r1, __uint_as_float(tm[j] & 0xFFFF0000u));
                tl[j] = w3_rn(__float_as_uint(r2));
            }
            uint4 ph, pm, pl;                                        // element j of a fragment in the low half of register j / 2 for even j
            ph.x = __builtin_amdgcn_perm(th[1], th[0], 0x07060302u); ph.y = __builtin_amdgcn_perm(th[3], th[2], 0x07060302u);
            ph.z = __builtin_amdgcn_perm(th[5], th[4], 0x07060302u); ph.w = __builtin_amdgcn_perm(th[7], th[6], 0x07060302u);
            pm.x = __builtin_amdgcn_perm(tm[1], tm[0], 0x07060302u); pm.y = __builtin_amdgcn_perm(tm[3], tm[2], 0x07060302u);
            pm.z = __builtin_amdgcn_perm(tm[5], tm[4], 0x07060302u); pm.w = __builtin_amdgcn_perm(tm[7], tm[6], 0x07060302u);
            pl.x = __builtin_amdgcn_perm(tl[1], tl[0], 0x07060302u); pl.y = __builtin_amdgcn_perm(tl[3], tl[2], 0x07060302u);
            pl.z = __builtin_amdgcn_perm(tl[5], tl[4], 0x07060302u); pl.w = __builtin_amdgcn_perm(tl[7], tl[6], 0x07060302u);
            unsigned char* at = img + sn * W3_AROW + (sg + 2 * q) * 16;
            *reinterpret_cast<uint4*>(at) = pl;                      // plane 0 = lo, 1 = mid, 2 = hi: the order they reach an accumulator in
            *reinterpret_cast<uint4*>(at + W3_APLANE) = pm;
            *reinterpret_cast<uint4*>(at + 2 * W3_APLANE) = ph;
        }
        *reinterpret_cast<uint32_t*>(img + 3 * W3_APLANE + (ww * W3_WROW + wr) * 4) = xw;
    };
    // the wave's tile
    const int wn = wave >> 1, wk = wave & 1;
    const int n0 = n_base + wn * 64, w0 = w_base + wk * 4;
    const bool live = n0 < g.N && w0 < g.Kw;                         // (wave-uniform; a wave wholly past an edge still stages and meets the barriers)
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    auto compute = [&](int buf) {
        const unsigned char* img = lds[buf];
        const unsigned char* ap = img + (wn * 64 + col) * W3_AROW + half * 16;
        const unsigned char* wp = img + 3 * W3_APLANE + (wk * 4 * W3_WROW + half * 8) * 4;
#pragma unroll
        for (int sub = 0; sub < W3_MB / 16; ++sub) {
            bf16x8 af[3][2];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int i = 0; i < 2; ++i) af[p][i] = *reinterpret_cast<const bf16x8*>(ap + p * W3_APLANE + i * 32 * W3_AROW + sub * 32);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint4 x0 = *reinterpret_cast<const uint4*>(wp + (j * W3_WROW + sub * 16) * 4);
                const uint4 x1 = *reinterpret_cast<const uint4*>(wp + (j * W3_WROW + sub * 16 + 4) * 4);
                union { uint32_t u[4]; bf16x8 v; } b;
                b.u[0] = (((x0.x >> col) & 1u) | (((x0.y >> col) & 1u) << 16)) * 0x3F80u;        // 1.0 in bf16 per set bit
                b.u[1] = (((x0.z >> col) & 1u) | (((x0.w >> col) & 1u) << 16)) * 0x3F80u;
                b.u[2] = (((x1.x >> col) & 1u) | (((x1.y >> col) & 1u) << 16)) * 0x3F80u;
                b.u[3] = (((x1.z >> col) & 1u) | (((x1.w >> col) & 1u) << 16)) * 0x3F80u;
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[p][i], b.v, acc[i][j], 0, 0, 0);
            }
        }
    };
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < n_stages; ++s) {
        const bool more = s + 1 < n_stages;                          // (uniform over the work-group)
        if (more) load(s + 1);
        if (live) compute(s & 1);
        if (more) store((s + 1) & 1);
        __syncthreads();
    }
    if (!live) return;
    // D[i][c]: c = lane & 31, i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const bool direct = g.n_slabs == 1;
    float* dst = direct ? gw : part + (size_t)blockIdx.z * g.N * g.K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 32 * (w0 + j) + col;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = n0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * half;
                if (n < g.N && k < g.K) {
                    float* at = dst + (size_t)n * g.K + k;
                    *at = (direct && g.accumulate) ? *at + acc[i][j][e] : acc[i][j][e];
                }
            }
        }
}

// part [n_slabs][N K] -> gw [N K]: the slabs in ascending order
__global__ __launch_bounds__(256) void k_wgrad3_reduce(const float* __restrict__ part, int n_slabs, size_t n, float* __restrict__ gw, int accumulate) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        float s = part[e];
        for (int sl = 1; sl < n_slabs; ++sl) s += part[(size_t)sl * n + e];
        gw[e] = accumulate ? gw[e] + s : s;
    }
}

#endif  // SNN_SPIKE_WGRAD_X3_H
