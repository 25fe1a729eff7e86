// Readout fine-tuning, the part between the head outputs and a scalar (include/snn_hip.h: snn_match_targets, snn_rpn_loss_grad,
// snn_det_loss_grad): IoU matching with labels and encoded regression targets, and the two heads' losses with their
// gradients with respect to the head outputs - what snn_li_heads_wgrad takes as g.
//
// Nothing here uses a floating-point atomic and nothing is cleared by a memset: every output element and every scratch element that is read
// is written by a launch of the same call, so the calls are capturable and two calls on the same data are bit-equal.
//
//   snn_match_targets   a thread owns a box, the image's ground-truth boxes (at most LS_MAX_GT) sit in LDS.  A work-group belongs to one
//                       image (blk_start).  With allow_low_quality, three launches:
//     k_match_partial     per-GT maxima of the work-group's 256 boxes: an integer max on the bit pattern of the non-negative IoU in LDS
//                         (order-independent), written to part[blk][g];
//     k_match_gtmax       one work-group per image: thread g takes the maximum over the image's work-groups;
//     k_match_finish      recomputes the box's IoU row (the same instructions, the same bits), takes the arg-max (lowest index on a tie),
//                         applies the two thresholds and the restore, and writes matched_idx, label and the encoded target.
//                       Without allow_low_quality only the last launch runs.  IoU follows stock/boxes.box_iou operation by operation
//                       (-ffp-contract=off, IEEE division), so every decision is torch's; logf is the one operation that is not torch's bit for bit.
//   snn_*_loss_grad     three launches each: k_*_loss<false> writes per-work-group partial sums {count, first loss, box loss} in fp64,
//                       k_loss_finish adds them in a fixed order, writes loss[2] and leaves n in the scratch, k_*_loss<true> reads n and
//                       writes every gradient element (zeros included).
//     k_rpn_loss          a thread owns one anchor of the head's own order (level, image, y, x, a) and computes its index in the reference's
//                         order (image, level, y, x, a), where label / sampled / reg_target live; nothing is permuted in memory.  deltas,
//                         reg_target and g_deltas move as 16-byte vectors;
//     k_det_loss          a work-group owns DL_ROWS rows: their logits come to LDS as one flat run of 16-byte vectors (the tile starts on a
//                         64-byte boundary whatever K is), 16 lanes share a row (maximum, then the sum of exponentials in fp64, butterfly),
//                         the gradients go back through LDS as flat vectors; g_box is written one (row, class) vector per thread.
#ifndef SNN_LOSS_H
#define SNN_LOSS_H

#define LS_MAX_GT 256                 // ground-truth boxes per image (LDS: 16 B box + area + maximum each)
#define LS_MAX_IMAGES 64
#define LS_MAX_LEVELS 8
#define LS_MAX_K 256                  // classes of snn_det_loss_grad
#define LS_MAX_A 64                   // anchors per position of snn_rpn_loss_grad
#define LS_BLOCK 256
#define DL_ROWS 16                    // rows of a work-group of k_det_loss
#define LS_HEADER 64                  // bytes in front of the partial sums: n (int32)

struct MatchArgs {
    const float4* boxes;
    const float4* gt;
    const long long* gt_labels;       // null: RPN mode
    int N, allow_lq;
    float high, low, wx, wy, ww, wh;
    int box_start[LS_MAX_IMAGES + 1], gt_start[LS_MAX_IMAGES + 1], blk_start[LS_MAX_IMAGES + 1];
};

__device__ __forceinline__ int match_image(const MatchArgs& a, int blk) {
    int n = 0;
    while (n + 1 < a.N && blk >= a.blk_start[n + 1]) ++n;
    return n;
}

__device__ __forceinline__ float ls_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }

// stock/boxes.box_iou(gt, boxes)[g][i], operation by operation
__device__ __forceinline__ float ls_iou(float4 g, float ag, float4 b, float ab) {
    const float w = fmaxf(fminf(g.z, b.z) - fmaxf(g.x, b.x), 0.0f), h = fmaxf(fminf(g.w, b.w) - fmaxf(g.y, b.y), 0.0f);
    const float inter = w * h;
    return inter / ((ag + ab) - inter);
}

__global__ __launch_bounds__(LS_BLOCK) void k_match_partial(const MatchArgs a, uint32_t* __restrict__ part) {
    __shared__ float4 sg[LS_MAX_GT];
    __shared__ float sa[LS_MAX_GT];
    __shared__ uint32_t smax[LS_MAX_GT];
    const int tid = threadIdx.x, blk = blockIdx.x, n = match_image(a, blk);
    const int g0 = a.gt_start[n], G = a.gt_start[n + 1] - g0;
    if (tid < G) {
        const float4 g = a.gt[g0 + tid];
        sg[tid] = g; sa[tid] = ls_area(g); smax[tid] = 0u;
    }
    __syncthreads();
    const int i = a.box_start[n] + (blk - a.blk_start[n]) * LS_BLOCK + tid;
    if (i < a.box_start[n + 1]) {
        const float4 b = a.boxes[i];
        const float ab = ls_area(b);
        for (int g = 0; g < G; ++g) {
            const float iou = ls_iou(sg[g], sa[g], b, ab);
            const uint32_t bits = __float_as_uint(iou);
            if (iou > 0.0f && bits > smax[g]) atomicMax(&smax[g], bits);       // (non-negative floats order as their bit patterns)
        }
    }
    __syncthreads();
    if (tid < G) part[(size_t)blk * LS_MAX_GT + tid] = smax[tid];
}

// grid: N; gtmax[gt_start[n] + g] = the maximum of part[blk][g] over the image's work-groups (0 for an image without boxes)
__global__ __launch_bounds__(LS_BLOCK) void k_match_gtmax(const MatchArgs a, const uint32_t* __restrict__ part, uint32_t* __restrict__ gtmax) {
    const int n = blockIdx.x, g = threadIdx.x, g0 = a.gt_start[n];
    if (g >= a.gt_start[n + 1] - g0) return;
    uint32_t m = 0u;
    for (int blk = a.blk_start[n]; blk < a.blk_start[n + 1]; ++blk) m = max(m, part[(size_t)blk * LS_MAX_GT + g]);
    gtmax[g0 + g] = m;
}

__global__ __launch_bounds__(LS_BLOCK) void k_match_finish(const MatchArgs a, const uint32_t* __restrict__ gtmax, int32_t* __restrict__ matched_idx,
                                                           int32_t* __restrict__ label, float4* __restrict__ reg_target) {
    __shared__ float4 sg[LS_MAX_GT];
    __shared__ float sa[LS_MAX_GT];
    __shared__ float sm[LS_MAX_GT];
    const int tid = threadIdx.x, blk = blockIdx.x, n = match_image(a, blk);
    const int g0 = a.gt_start[n], G = a.gt_start[n + 1] - g0;
    if (tid < G) {
        const float4 g = a.gt[g0 + tid];
        sg[tid] = g; sa[tid] = ls_area(g);
        sm[tid] = a.allow_lq ? __uint_as_float(gtmax[g0 + tid]) : 0.0f;
    }
    __syncthreads();
    const int i = a.box_start[n] + (blk - a.blk_start[n]) * LS_BLOCK + tid;
    if (i >= a.box_start[n + 1]) return;
    const float4 b = a.boxes[i];
    const float ab = ls_area(b);
    float best = -1.0f;
    int bi = 0;
    bool restore = false;
    for (int g = 0; g < G; ++g) {
        const float iou = ls_iou(sg[g], sa[g], b, ab);
        if (iou > best) { best = iou; bi = g; }                                // (strict: the lowest index keeps a tie)
        restore = restore || iou == sm[g];
    }
    int m = bi, lb = 0;
    float4 gb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (G > 0) {
        if (best < a.low) m = -1;
        else if (best < a.high) m = -2;
        if (a.allow_lq && restore) m = bi;
        lb = m >= 0 ? (a.gt_labels ? (int)a.gt_labels[g0 + m] : 1) : (m == -1 ? 0 : -1);
        gb = sg[m > 0 ? m : 0];
    }
    // BoxCoder.encode, operation by operation
    const float ew = b.z - b.x, eh = b.w - b.y, ecx = b.x + 0.5f * ew, ecy = b.y + 0.5f * eh;
    const float gw = gb.z - gb.x, gh = gb.w - gb.y, gcx = gb.x + 0.5f * gw, gcy = gb.y + 0.5f * gh;
    float4 t;
    t.x = a.wx * (gcx - ecx) / ew;
    t.y = a.wy * (gcy - ecy) / eh;
    t.z = a.ww * logf(gw / ew);
    t.w = a.wh * logf(gh / eh);
    matched_idx[i] = m;
    label[i] = lb;
    reg_target[i] = t;
}

// ---- the two losses ----
// sum of three per-thread values over the work-group in a fixed tree; the totals are red[k][0] afterwards
__device__ __forceinline__ void block_sum3(double (*red)[LS_BLOCK], double x, double y, double z) {
    const int tid = threadIdx.x;
    red[0][tid] = x; red[1][tid] = y; red[2][tid] = z;
    __syncthreads();
    for (int s = LS_BLOCK / 2; s >= 1; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s]; }
        __syncthreads();
    }
}

#define LS_BETA (1.0f / 9.0f)
// smooth L1 at beta = 1/9 as torch's CPU kernel forms it, and its derivative
__device__ __forceinline__ float sl1(float d) {
    const float z = fabsf(d);
    return z < LS_BETA ? 0.5f * z * z / LS_BETA : z - 0.5f * LS_BETA;
}
__device__ __forceinline__ float sl1_grad(float d) { return fabsf(d) < LS_BETA ? d / LS_BETA : (d > 0.0f ? 1.0f : -1.0f); }
__device__ __forceinline__ double sl1_sum(float4 p, float4 t) {
    return (double)sl1(p.x - t.x) + (double)sl1(p.y - t.y) + (double)sl1(p.z - t.z) + (double)sl1(p.w - t.w);
}
__device__ __forceinline__ float4 sl1_grad4(float4 p, float4 t, float nf) {
    return make_float4(sl1_grad(p.x - t.x) / nf, sl1_grad(p.y - t.y) / nf, sl1_grad(p.z - t.z) / nf, sl1_grad(p.w - t.w) / nf);
}

// part [nb][3] -> loss[2] = sums / count (0 / 0 = NaN, as torch's mean over nothing), *n_dev = count
__global__ __launch_bounds__(LS_BLOCK) void k_loss_finish(const double* __restrict__ part, int nb, float* __restrict__ loss, int* __restrict__ n_dev) {
    __shared__ double red[3][LS_BLOCK];
    double c = 0.0, x = 0.0, y = 0.0;
    for (int b = threadIdx.x; b < nb; b += LS_BLOCK) { c += part[3 * (size_t)b]; x += part[3 * (size_t)b + 1]; y += part[3 * (size_t)b + 2]; }
    block_sum3(red, c, x, y);
    if (threadIdx.x == 0) {
        const double n = red[0][0];
        *n_dev = (int)n;
        loss[0] = (float)(red[1][0] / n);
        loss[1] = (float)(red[2][0] / n);
    }
}

struct RpnLossArgs {
    int n_levels, A, per_image, total;                   // per_image: anchors of an image; total = P * A
    int row_start[LS_MAX_LEVELS], hw[LS_MAX_LEVELS], anc_off[LS_MAX_LEVELS];     // first row, H * W, first anchor inside an image
};

template <bool GRAD>
__global__ __launch_bounds__(LS_BLOCK) void k_rpn_loss(const RpnLossArgs a, const float* __restrict__ logits, const float4* __restrict__ deltas,
                                                       const int32_t* __restrict__ label, const uint8_t* __restrict__ sampled,
                                                       const float4* __restrict__ tgt, double* __restrict__ part, const int* __restrict__ n_dev,
                                                       float* __restrict__ g_logits, float4* __restrict__ g_deltas) {
    __shared__ double red[3][LS_BLOCK];
    const int e = blockIdx.x * LS_BLOCK + threadIdx.x;
    const bool valid = e < a.total;
    int lb = 0, ref = 0;
    bool sm = false;
    if (valid) {
        const int p = e / a.A, an = e - p * a.A;
        int rs = 0, hw = 1, ao = 0;
#pragma unroll
        for (int l = 0; l < LS_MAX_LEVELS; ++l)
            if (l < a.n_levels && p >= a.row_start[l]) { rs = a.row_start[l]; hw = a.hw[l]; ao = a.anc_off[l]; }
        const int loc = p - rs, n = loc / hw, yx = loc - n * hw;
        ref = n * a.per_image + ao + yx * a.A + an;
        lb = label[ref];
        sm = sampled[ref] != 0;
    }
    if (!GRAD) {
        double cnt = 0.0, ob = 0.0, bx = 0.0;
        if (sm) {
            const float x = logits[e], y = (float)lb;
            cnt = 1.0;
            ob = (double)((fmaxf(x, 0.0f) - x * y) + log1pf(expf(-fabsf(x))));
            if (lb == 1) bx = sl1_sum(deltas[e], tgt[ref]);
        }
        block_sum3(red, cnt, ob, bx);
        if (threadIdx.x == 0) { part[3 * (size_t)blockIdx.x] = red[0][0]; part[3 * (size_t)blockIdx.x + 1] = red[1][0]; part[3 * (size_t)blockIdx.x + 2] = red[2][0]; }
    } else {
        if (!valid) return;
        float gl = 0.0f;
        float4 gd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (sm) {
            const float nf = (float)*n_dev, x = logits[e], ex = expf(-fabsf(x));
            const float s = x >= 0.0f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
            gl = (s - (float)lb) / nf;
            if (lb == 1) gd = sl1_grad4(deltas[e], tgt[ref], nf);
        }
        g_logits[e] = gl;
        g_deltas[e] = gd;
    }
}

template <bool GRAD>
__global__ __launch_bounds__(LS_BLOCK) void k_det_loss(const float* __restrict__ logits, const float4* __restrict__ box, const int32_t* __restrict__ label,
                                                       const float4* __restrict__ tgt, int R, int K, double* __restrict__ part,
                                                       const int* __restrict__ n_dev, float* __restrict__ g_logits, float4* __restrict__ g_box) {
    __shared__ __attribute__((aligned(16))) float sl[DL_ROWS * LS_MAX_K];
    __shared__ int slab[DL_ROWS];
    __shared__ double red[3][LS_BLOCK];
    const int tid = threadIdx.x, r0 = blockIdx.x * DL_ROWS, nr = min(DL_ROWS, R - r0), ne = nr * K, nv = ne >> 2;
    const size_t e0 = (size_t)r0 * K;                                          // (r0 is a multiple of 16: the tile starts on a 64-byte boundary)
    for (int v = tid; v < nv; v += LS_BLOCK) reinterpret_cast<float4*>(sl)[v] = reinterpret_cast<const float4*>(logits + e0)[v];
    for (int e = 4 * nv + tid; e < ne; e += LS_BLOCK) sl[e] = logits[e0 + e];
    if (tid < DL_ROWS) {
        int lb = tid < nr ? label[r0 + tid] : -1;
        slab[tid] = (lb < -1 || lb >= K) ? -1 : lb;                            // (a label that is no class is left out like -1)
    }
    __syncthreads();
    const int r = tid >> 4, q = tid & 15;
    const bool row = r < nr;
    const int lb = slab[r];
    float m = -INFINITY;
    if (row) for (int j = q; j < K; j += 16) m = fmaxf(m, sl[r * K + j]);
    for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
    double s = 0.0;
    if (row) for (int j = q; j < K; j += 16) s += (double)expf(sl[r * K + j] - m);
    for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 16);
    const float sf = (float)s;
    if (!GRAD) {
        double cnt = 0.0, ce = 0.0, bx = 0.0;
        if (row && q == 0 && lb >= 0) {
            cnt = 1.0;
            ce = (double)((m - sl[r * K + lb]) + logf(sf));
            if (lb > 0) bx = sl1_sum(box[e0 + (size_t)r * K + lb], tgt[r0 + r]);
        }
        block_sum3(red, cnt, ce, bx);
        if (tid == 0) { part[3 * (size_t)blockIdx.x] = red[0][0]; part[3 * (size_t)blockIdx.x + 1] = red[1][0]; part[3 * (size_t)blockIdx.x + 2] = red[2][0]; }
    } else {
        const float nf = (float)*n_dev;
        if (row)
            for (int j = q; j < K; j += 16)                                    // (a lane reads and writes its own columns only)
                sl[r * K + j] = lb >= 0 ? (expf(sl[r * K + j] - m) / sf - (j == lb ? 1.0f : 0.0f)) / nf : 0.0f;
        __syncthreads();
        for (int v = tid; v < nv; v += LS_BLOCK) reinterpret_cast<float4*>(g_logits + e0)[v] = reinterpret_cast<const float4*>(sl)[v];
        for (int e = 4 * nv + tid; e < ne; e += LS_BLOCK) g_logits[e0 + e] = sl[e];
        for (int e = tid; e < ne; e += LS_BLOCK) {
            const int rr = e / K, k = e - rr * K, l2 = slab[rr];
            float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (l2 > 0 && k == l2) o = sl1_grad4(box[e0 + e], tgt[r0 + rr], nf);
            g_box[e0 + e] = o;
        }
    }
}

#endif  // SNN_LOSS_H
