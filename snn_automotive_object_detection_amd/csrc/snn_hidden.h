// Hidden-layer gradients of the detector's fc7 -> lif7 (include/snn_hip.h: snn_planes_to_rows, snn_lif_surrogate_bwd, snn_spike_linear_wgrad;
// DESIGN.md 4.15): what lies between the readout gradients (snn_wgrad.h) and dL/dW7.
//
//   k_planes_to_rows     thread = one word of the result [T'][rows][words] (the stores of a wave are contiguous); the word is fetched through
//                        tap_word, as the taps address the three layouts.  The "save" of a pass's planes and the [M][Kw] operand of the un-fused GEMMs.
//   k_lif_surrogate_bwd  thread = one neuron (row, column).  Norse's lif_feed_forward_step with a SuperSpike threshold, differentiated:
//                          forward  vd_t = v + a ((v_leak - v) + i);  v = z_t ? v_reset : vd_t;  i = (i + b i) + cur_t      z_t = the SAVED bit
//                          reverse  s = 1 / (alpha |vd_t - th| + 1)^2;  dz = gz_t + G_v (v_reset - vd_t);  dvd = G_v (1 - z_t) + dz s;
//                                   d_cur_t = G_i (t <= Tc - 1);  G_i = dvd a + G_i (1 + b);  G_v = dvd (1 - a)
//                        The forward sweep parks vd_{t + 1} in d_cur[t] (vd_0 = v_leak needs no slot), the reverse sweep reads vd_t from
//                        d_cur[t - 1] and writes d_cur[t] after step t + 1 has consumed that slot: no register array, no extra buffer, and a
//                        thread touches its own column only, so no barrier.  The T spike bits of the neuron travel in one register.
//   k_spike_wgrad_partial / k_spike_wgrad_reduce
//                        gw[n][k] (+)= sum_m d_cur[m][n] bit(m, k) over the M = T' rows reduction rows (both operands are contiguous in
//                        (t, row)), on v_mfma_f32_32x32x2_f32 WITHOUT LDS: the instruction's operand maps are the memory layouts.
//                          A[i = lane & 31][kk = lane >> 5] = d_cur[m + kk][n0 + i]   32 consecutive floats per half-wave, straight from global memory
//                          B[kk][j = lane & 31]              = bit j of ONE plane word of row m + kk: one word per half-wave (a vector load, 32 lanes on one address), then v_bfe + v_cvt
//                          D[i][j]                           = gw[n0 + i][32 w + j]    (rows of D are outputs n, its columns are input bits k)
//                        A wave owns SW_WN x SW_WK = 64 outputs x 128 inputs (2 x 4 accumulators of 16 registers), a work-group 2 x 2 waves =
//                        128 x 256.  Per pair of reduction rows a wave issues 2 + 4 loads, 8 vector instructions and 8 matrix instructions (512
//                        matrix-pipe cycles); the loads of the next SW_U pairs are in flight while the current ones are multiplied (a
//                        second register set, copied over after the products), and every load of a full batch is unconditional (a load
//                        behind a branch makes the compiler wait for all loads in flight before the products).  __launch_bounds__(256, 2)
//                        holds the kernel to 256 registers - two work-groups per CU, two waves per SIMD; without it the compiler takes 264.  Indices past N, past the last plane word and past K
//                        are CLAMPED for the loads (they feed accumulators that are never stored); a row past the slab's end - in its last,
//                        partial batch only - is loaded from the slab's last row and its gradient replaced by +0.
//                        The reduction is split into row slabs (a function of M alone); every work-group writes its valid partial tile to
//                        scratch[slab][n][k], the second launch adds the slabs in ascending order and writes (or adds to) every element of gw.
// No floating-point atomics, nothing cleared in front: every element read is written by a launch of the same call.
#ifndef SNN_HIDDEN_H
#define SNN_HIDDEN_H

#define SW_WN 64                     // outputs (d_cur columns) of a wave's tile: 2 blocks of 32
#define SW_WK 128                    // inputs (plane bits) of a wave's tile: 4 words
#define SW_TN (2 * SW_WN)            // work-group tile: 2 x 2 waves
#define SW_TK (2 * SW_WK)
#define SW_U 4                       // pairs of reduction rows per batch (the depth of the register prefetch)
#define SW_BATCH (2 * SW_U)
#define SW_SLAB_ROWS 512             // reduction rows a slab owns at least (but for the last)
#define SW_MAX_SLABS 16
#define SW_MAX_DIM 8192
#define HB_MAX_N 8192

__global__ __launch_bounds__(256) void k_planes_to_rows(const TapView v, int T, uint32_t* __restrict__ out) {
    const long long per_step = v.rows * v.words, total = per_step * T;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int t = (int)(e / per_step);
        const long long q = e - t * per_step, r = q / v.words;
        const int w = (int)(q - r * v.words);
        out[e] = v.planes[(size_t)t * v.step_stride + tap_word(v, r, w)];
    }
}

struct LifBwdArgs {
    const float* cur;                // [Tc][R][ldc]
    const uint32_t* z;               // [Tc + 1][R][Nw]
    const float* gz;                 // [Tc + 1][R][N] or null
    const float* gu;                 // [R][N] or null
    float* d_cur;                    // [Tc][R][N]
    int ldc, Tc, R, N, Nw;
    float a, b, v_leak, v_reset, th, alpha;
    float kappa[SNN_MAX_STEPS];      // li_kappa(p, Tc + 1).last
};

__global__ __launch_bounds__(256) void k_lif_surrogate_bwd(const LifBwdArgs g) {
    __shared__ float kap[SNN_MAX_STEPS];
    if (threadIdx.x < SNN_MAX_STEPS) kap[threadIdx.x] = g.kappa[threadIdx.x];
    __syncthreads();
    const long long total = (long long)g.R * g.N;
    const size_t plane = (size_t)g.R * g.N;
    const float one_b = 1.0f + g.b, one_a = 1.0f - g.a;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / g.N;
        const int n = (int)(e - r * g.N);
        const float* cur = g.cur + (size_t)r * g.ldc + n;
        const uint32_t* zp = g.z + (size_t)r * g.Nw + (n >> 5);
        float* dc = g.d_cur + e;
        // forward: vd_1 .. vd_Tc parked in d_cur[0 .. Tc - 1], the saved bits of steps 0 .. Tc gathered in `bits`
        uint32_t bits = 0;
        float v = g.v_leak, i = 0.0f;
        for (int t = 0; t < g.Tc; ++t) {
            const float vd = t ? v + g.a * ((g.v_leak - v) + i) : g.v_leak;     // (vd_0: the initial state is v_leak, i = 0)
            const uint32_t zt = (zp[(size_t)t * g.R * g.Nw] >> (n & 31)) & 1u;
            bits |= zt << t;
            v = zt ? g.v_reset : vd;
            i = (i + g.b * i) + cur[(size_t)t * g.R * g.ldc];
            if (t) dc[(size_t)(t - 1) * plane] = vd;
        }
        {
            const float vd = v + g.a * ((g.v_leak - v) + i);                    // vd_Tc (Tc >= 1)
            bits |= ((zp[(size_t)g.Tc * g.R * g.Nw] >> (n & 31)) & 1u) << g.Tc;
            dc[(size_t)(g.Tc - 1) * plane] = vd;
        }
        // reverse
        const float gu = g.gu ? g.gu[e] : 0.0f;
        float Gv = 0.0f, Gi = 0.0f;
        for (int t = g.Tc; t >= 0; --t) {
            const float vd = t ? dc[(size_t)(t - 1) * plane] : g.v_leak;
            if (t < g.Tc) dc[(size_t)t * plane] = Gi;
            float up = g.gz ? g.gz[(size_t)t * plane + e] : 0.0f;
            if (g.gu) up = up + kap[t] * gu;
            const float zt = (float)((bits >> t) & 1u);
            const float d = g.alpha * fabsf(vd - g.th) + 1.0f;
            const float s = 1.0f / (d * d);
            const float dz = up + Gv * (g.v_reset - vd);
            const float dvd = Gv * (1.0f - zt) + dz * s;
            Gi = dvd * g.a + Gi * one_b;
            Gv = dvd * one_a;
        }
    }
}

struct SpikeWgradArgs {
    const uint32_t* a;               // [M][Kw]
    const float* d;                  // [M][ldd]
    long long M, slab_rows;          // reduction rows; rows of a slab (a multiple of SW_BATCH)
    int ldd, K, Kw, N, n_slabs;
};

// grid (tiles over K, tiles over N, slabs); part [n_slabs][N][K]
__global__ __launch_bounds__(256, 2) void k_spike_wgrad_partial(const SpikeWgradArgs g, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
    const int n0 = blockIdx.y * SW_TN + (wave >> 1) * SW_WN, w0 = (blockIdx.x * SW_TK + (wave & 1) * SW_WK) >> 5;
    const long long m0 = (long long)blockIdx.z * g.slab_rows, m1 = min(g.M, m0 + g.slab_rows);
    if (n0 >= g.N || w0 >= g.Kw) return;                             // (a wave wholly past an edge stores nothing; no barrier follows)
    int nc[2], wc[4];               // clamped column / word of each operand block (what lies past the edge is never stored)
#pragma unroll
    for (int i = 0; i < 2; ++i) nc[i] = min(n0 + 32 * i + col, g.N - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) wc[j] = min(w0 + j, g.Kw - 1);
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    float fa[SW_U][2], na[SW_U][2];
    uint32_t fb[SW_U][4], nb[SW_U][4];
    // a batch that lies wholly inside the slab: every load unconditional, so the loads of the next batch stay in flight under this one's products;
    // the address is a wave-uniform 64-bit base (scalar registers, advanced by scalar adds) plus a 32-bit byte offset per lane that never changes
    // (the offset carries the half-wave's row: two rows, and so two plane-word addresses, per wave and load)
    uint32_t dlo[2], alo[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) dlo[i] = ((uint32_t)half * (uint32_t)g.ldd + (uint32_t)nc[i]) * 4u;          // (ldd < 2^28: the host checks)
#pragma unroll
    for (int j = 0; j < 4; ++j) alo[j] = ((uint32_t)half * (uint32_t)g.Kw + (uint32_t)wc[j]) * 4u;
    auto load_full = [&](long long off, float (&xa)[SW_U][2], uint32_t (&xb)[SW_U][4]) {
        const char* db = reinterpret_cast<const char*>(g.d) + (size_t)(m0 + off) * g.ldd * 4;
        const char* ab = reinterpret_cast<const char*>(g.a) + (size_t)(m0 + off) * g.Kw * 4;
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            const char* du = db + (size_t)(2 * u) * g.ldd * 4;
            const char* au = ab + (size_t)(2 * u) * g.Kw * 4;
#pragma unroll
            for (int i = 0; i < 2; ++i) xa[u][i] = *reinterpret_cast<const float*>(du + dlo[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) xb[u][j] = *reinterpret_cast<const uint32_t*>(au + alo[j]);
        }
    };
    // the slab's last, partial batch: a row past the end is loaded from the slab's last row (a valid address) and its gradient replaced by +0
    auto load_tail = [&](long long off, float (&xa)[SW_U][2], uint32_t (&xb)[SW_U][4]) {
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            const long long row = m0 + off + 2 * u + half;
            const bool in = row < m1;
            const long long rc = in ? row : m1 - 1;
            const float* dp = g.d + (size_t)rc * g.ldd;
            const uint32_t* ap = g.a + (size_t)rc * g.Kw;
#pragma unroll
            for (int i = 0; i < 2; ++i) { const float x = dp[nc[i]]; xa[u][i] = in ? x : 0.0f; }
#pragma unroll
            for (int j = 0; j < 4; ++j) xb[u][j] = ap[wc[j]];
        }
    };
    auto mma = [&](const float (&xa)[SW_U][2], const uint32_t (&xb)[SW_U][4]) {
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = (float)((xb[u][j] >> col) & 1u);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[u][i], b[j], acc[i][j], 0, 0, 0);
        }
    };
    const long long n_full = (m1 - m0) / SW_BATCH;
    const bool tail = ((m1 - m0) % SW_BATCH) != 0;                     // (wave-uniform, as every branch below)
    if (n_full) {
        load_full(0, fa, fb);
        for (long long b = 0; b + 1 < n_full; ++b) {
            load_full((b + 1) * SW_BATCH, na, nb);
            mma(fa, fb);
#pragma unroll
            for (int u = 0; u < SW_U; ++u) {
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[u][i] = na[u][i];
#pragma unroll
                for (int j = 0; j < 4; ++j) fb[u][j] = nb[u][j];
            }
        }
        mma(fa, fb);
    }
    if (tail) {                                                      // (a slab is never empty: n_full or tail)
        load_tail(n_full * SW_BATCH, na, nb);
        mma(na, nb);
    }
    // D[i][j]: j = lane & 31, i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* dst = part + (size_t)blockIdx.z * g.N * g.K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 32 * (w0 + j) + col;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = n0 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * half;
                if (n < g.N && k < g.K) dst[(size_t)n * g.K + k] = acc[i][j][e];
            }
        }
}

// part [n_slabs][N K] -> gw [N K]: the slabs in ascending order
__global__ __launch_bounds__(256) void k_spike_wgrad_reduce(const float* __restrict__ part, int n_slabs, size_t n, float* __restrict__ gw, int accumulate) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        float s = part[e];
        for (int sl = 1; sl < n_slabs; ++sl) s += part[(size_t)sl * n + e];
        gw[e] = accumulate ? gw[e] + s : s;
    }
}

#endif  // SNN_HIDDEN_H
