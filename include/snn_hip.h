/*
 * snn_hip.h — C ABI of libsnnhip.so: the spiking RPN head + spiking RoI (detector) head forward
 * path of aitor-martinez-seras/SNN-Automotive-Object-Detection as hand-written gfx950 (MI355X)
 * HIP kernels.
 *
 * The reference has no FFI of its own (it is pure Python on torch + Norse); the entry points below
 * are what a binding for this path calls instead of the reference's Python loops:
 *
 *   snn_rpn_head_forward   replaces  RPNHeadSNN.forward                    rpn.py:84-121
 *                          (+ the spike-rate variant kept as a string literal, rpn.py:126-200)
 *   snn_det_head_forward   replaces  FastRCNNPredictorSNNFull.forward      faster_rcnn.py:470-516
 *                          (+ the spike-rate variant, faster_rcnn.py:520-618)
 *   snn_pack_*             one-off re-layout of the reference's state_dict tensors
 *                          (shared_conv/conv_cls/conv_bbox, rpn.py:64-75; fc6/fc7/cls_score/bbox_pred,
 *                          faster_rcnn.py:447-467) into the MFMA fragment-major layout the kernels read
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; the caller owns every buffer; the
 *     library allocates nothing persistent and frees nothing of the caller's;
 *   - all work is enqueued on the stream passed in; no default-stream use.  With three exceptions no call synchronises,
 *     allocates, frees or copies between host and device, so every other call is hipGraph-capturable.  The exceptions are
 *     the bf16 packers snn_pack_conv3x3_weight_bf16, snn_pack_linear_weight_bf16 and snn_pack_linear_weight_bf16_perm:
 *     they allocate a status word, copy the verdict (a weight that is not finite or rounds to +-inf) to the host, wait for
 *     the stream and free the word.  Call them before a capture, never inside one;
 *   - capture contract of every other call: ONE stream (no fork / join inside the capture); warm caches on the caller's
 *     side (packed weights and whatever else the binding builds lazily exist before the capture begins: call once eagerly
 *     first); and every buffer the call was handed - operands, outputs, workspace, route_stat, count tensors - lives as
 *     long as the graph, which reads and writes the same addresses on every replay.  The launch attributes and occupancy
 *     queries a call makes on the host are accepted while its stream is capturing.  Nothing a call decides on the host
 *     depends on the contents of a device buffer, and every counter a call uses is cleared by work of that call on the
 *     stream, so a replay on new contents returns what an eager call on them returns, bit for bit
 *     (tests/test_gpu_graph_capture.py; tests/test_graph_capture_cpu.py pins the list of exceptions to csrc/).  One
 *     configuration is NOT established: the *_routed heads in route "auto" at C = 256 / Hd = 1024 inside a capture of
 *     the five-call static-shape sequence ("Graph capture": open);
 *   - return value 0 = success, negative = error (message via snn_last_error(), thread-local);
 *     no exceptions cross the ABI and the library never aborts;
 *   - re-entrant: no global mutable state besides the thread-local error string.  Two kinds of process-wide constants are
 *     cached at first use: the debug / A-B knobs (environment variables SNN_*, read ONCE and frozen; snn_debug_reload_knobs()
 *     re-reads them - test hook, not for concurrent use) and properties of the device (CU count, occupancy of a kernel).
 *   - workspaces: a call that takes one is sized by its snn_*_workspace_bytes query, writes nothing behind that many bytes, and
 *     returns the same bits whatever the bytes held before (opaque scratch; nothing is kept in it from call to call).  A workspace
 *     below the query's size is refused (negative return, nothing enqueued) - also where this call's own layout would need less
 *     (snn_rpn_proposals: the query bounds every level split).  tests/test_gpu_ws_state.py pins all three.
 *
 * Spike tensors never exist as fp32.  A spike train is a set of BIT-PLANES
 *     plane[t][row][w]   (uint32, bit b of word w = spike of channel 32*w+b at time step t)
 * rows are spatial positions (RPN: level-major, then n, y, x) or RoIs (detector).
 */
#ifndef SNN_HIP_H
#define SNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* snn_stream_t;   /* == hipStream_t */

#define SNN_MAX_LEVELS 8
#define SNN_MAX_STEPS 32

/* Neuron constants.  The fp32 products are formed by the caller exactly as Norse forms them
 * (0-dim fp32 tensor arithmetic: dt * tau_mem_inv, -dt * tau_syn_inv) so that the element-wise
 * arithmetic is bit-identical to the reference's (norse lif.py / leaky_integrator.py; reference
 * call sites rpn.py:58,67,101,106,111,115, faster_rcnn.py:444-456,494-510).
 * Semantics of one set (any finite values; the reference's are the comments on the fields):
 *   - the encoder (lif_current_encoder) and the hidden LIF cells share v_leak, v_reset and both products; they differ in their
 *     threshold only (v_th_enc / v_th_lif);
 *   - the encoder's membrane starts at 0 whatever v_leak is (rpn.py:93, faster_rcnn.py:484); an LIF cell's membrane starts at v_leak and
 *     its synaptic current at 0, so v_leak - v_th_lif > 0 fires every LIF neuron at step 0;
 *   - the LI cells of the heads take the same two products with v_leak = 0 and start from zero state;
 *   - the encoder resets arithmetically, v - (v - v_reset), the LIF cells to v_reset; spikes are (v - v_th > 0).
 * No combination is refused.  The values choose the launch plan, never the result: zero rest and reset potentials run period planes, the
 * threshold-table encoder where a table verifies for (dt_tau_mem, v_th_enc) (0 < dt_tau_mem < 1, v_th_enc > 0; else its recurrence) and
 * the structured-sparse launches; any other rest / reset potential the op-for-op encoder and the dense launches; a spike at step 0 keeps
 * step 0 in fc7's window.  Every plan is pinned to the parametrised oracle bit for bit (tests/test_gpu_neuron_constants.py). */
typedef struct snn_params {
    float dt_tau_mem;      /* fl32(dt * tau_mem_inv)   = 0.1f for the reference (dt=0.001, 1/1e-2) */
    float neg_dt_tau_syn;  /* fl32(-dt * tau_syn_inv)  = -0.2f                  (1/5e-3)           */
    float v_leak;          /* 0 */
    float v_reset;         /* 0 */
    float v_th_enc;        /* 0.25  encoder threshold (rpn.py:58, faster_rcnn.py:444) */
    float v_th_lif;        /* 0.1   hidden LIF threshold (rpn.py:67, faster_rcnn.py:449,452) */
    int32_t li_order;      /* 0 = jump-first (upstream li_feed_forward_step), 1 = voltage-first */
    int32_t precision;     /* SNN_PRECISION_*: how the two big contractions run (results are fp32-exact in both) */
} snn_params;

#define SNN_PRECISION_F32 0      /* fp32 matrix cores (v_mfma_f32_32x32x2_f32); 3x3 conv + LIF fused over T */
#define SNN_PRECISION_MXFP6 2    /* fp4 x fp6 block-scaled matrix path, weights as 6 planes of base-32 digits (snn_pack_*_mx):
                                    exact for weights within 2^5 of their block maximum, else rounded at 2^-28 of it;
                                    needs C / D / Hd multiples of 128 (else -4: use SNN_PRECISION_BF16X3) */
#define SNN_PRECISION_BF16X3 1   /* bf16 matrix cores, exact 3-way bf16 split of the fp32 weights; the conv runs
                                    time-batched (currents through HBM) followed by the LIF scan */

#define SNN_PRECISION_F32_STRICT 3 /* SNN_PRECISION_F32 with the LI heads on the fp32 VALU kernel too: no weight is ever split into bf16 planes.
                                    Where layers go whose weights snn_check_bf16x3_split reports as not exactly splittable (packed
                                    weights: the SNN_PRECISION_F32 ones) */

#define SNN_PRECISION_BF16 4     /* the SNN_PRECISION_BF16X3 path on ONE bf16 weight plane: the packers (snn_pack_*_bf16) round every weight of the
                                    3x3 conv, fc6 and fc7 once to the nearest bf16, ties to even, as loading a bf16 checkpoint would; the LI heads'
                                    packed operand is fed the rounded values.  Spikes are {0, 1}, so products stay exact; accumulation and neuron
                                    state stay fp32.  The result is the fp32 computation on the ROUNDED weights - like SNN_PRECISION_MXFP6 this
                                    mode is OUTSIDE the 1e-4-to-the-fp32-reference contract.  A third of the matrix instructions and weight bytes
                                    of the conv + LIF, fc6 and fc7 launches.  Not a default; nothing falls back to it or from it */

typedef struct snn_rpn_level {
    const float* feat;     /* [N][C][H][W] fp32, NCHW contiguous (what the FPN hands over) */
    int32_t N, H, W;
    int32_t reserved;
} snn_rpn_level;

int snn_version(void);
const char* snn_last_error(void);

/* ---- weight packing (call when the weights change; results are plain device buffers) ---------- */
/* number of floats of a packed GEMM operand with K reduction rows and N output columns */
size_t snn_packed_gemm_elems(int K_chunks32, int N);
/* shared_conv.weight [C_out][C_in][3][3] -> packed, reduction index k = tap*Cp + ci (Cp = C_in
 * rounded up to 32) */
size_t snn_packed_conv3x3_elems(int C_out, int C_in);
int snn_pack_conv3x3_weight(const float* w_oihw, int C_out, int C_in, float* packed, snn_stream_t s);
/* nn.Linear weight [N][K] -> packed */
size_t snn_packed_linear_elems(int N, int K);
int snn_pack_linear_weight(const float* w_nk, int N, int K, float* packed, snn_stream_t s);
/* the two leaky-integrator heads (cls then bbox) [NA][K] and [NB][K] -> transposed [Kp][NOp],
 * NOp = (NA+NB) rounded up to 16, Kp = K rounded up to 32 */
size_t snn_packed_heads_elems(int NA, int NB, int K);
int snn_pack_heads_weight(const float* w_a, int NA, const float* w_b, int NB, int K, float* packed,
                          snn_stream_t s);

/* Exactness check of the bf16x3 split (SNN_PRECISION_BF16X3, and the LI heads of every precision but SNN_PRECISION_F32_STRICT, carry
 * each fp32 weight as hi + mid + lo with three bf16 values).  The split is exact for every finite fp32 weight except magnitudes with
 * bits below 2^-133 and values within 2^119 of FLT_MAX; this call classifies n weights (any layout) and writes three counters:
 *   status3[0]  finite weights whose planes do NOT add up to the fp32 value
 *   status3[1]  non-finite weights (the split of a NaN / infinity is meaningless)
 *   status3[2]  weights with a plane that is a non-zero bf16 subnormal (exact; informational)
 * A binding must not run the bf16x3 kernels on a tensor with status3[0] or status3[1] != 0 (the Python modules fall back to
 * SNN_PRECISION_F32_STRICT with a RuntimeWarning).  status3 is a device buffer, written on `s`. */
int snn_check_bf16x3_split(const float* w, size_t n, uint32_t* status3, snn_stream_t s);

/* ---- RPN head ------------------------------------------------------------------------------- */
/* P = sum over levels of N*H*W.  Outputs are position-major ("NHWC"): out_logits[P][A],
 * out_bbox[P][4A]; level l starts at row sum_{j<l} N_j*H_j*W_j and is [N][H][W][A] inside.
 * Optional (nullable) spike-rate outputs of the rpn.py:126-200 variant:
 *   spike_counts[n_levels][max_N] (uint64)  number of shared-LIF spikes per level and image,
 *   sum_logits[P][A], sum_bbox[P][4A]        sum over the T steps of the LI membranes.          */
size_t snn_rpn_head_workspace_bytes(const snn_rpn_level* levels_host, int n_levels, int C, int A, int T,
                                    int precision);
int snn_rpn_head_forward(const snn_rpn_level* levels_host, int n_levels, int C, int A, int T,
                         const snn_params* p_host,
                         const void* w_shared_packed /* snn_pack_conv3x3_weight[_bf16x3], matching p_host->precision */,
                         const float* w_heads_packed,
                         float* out_logits, float* out_bbox,
                         unsigned long long* spike_counts, float* sum_logits, float* sum_bbox,
                         void* workspace, size_t workspace_bytes, snn_stream_t stream);

/* Same call restricted to a subset of its three stages (they communicate through the workspace);
 * lets a profiler bracket the dominant kernel exactly as the full call launches it.
 * CONTRACT: the workspace contents between stages are OPAQUE (which planes exist raw, which only compressed, and where, depends on
 * T, the precision and the library's knobs: since round 5 the encoder stage writes the period planes e_3 .. compressed only).  A
 * stage-by-stage caller must run the stages in order on the SAME workspace with IDENTICAL arguments (levels, C, A, T, params,
 * weights, spike_counts null or not) and an unchanged environment; a later stage after anything else has used the workspace, or
 * with other arguments, computes on stale bytes (no error is raised: the library cannot tell).  Inspect hidden spike planes through
 * snn_rpn_head_planes_view and the spike taps (below), not by guessing at the workspace. */
#define SNN_STAGE_ENCODE 1
#define SNN_STAGE_CONV_LIF 2
#define SNN_STAGE_LI_HEADS 4
#define SNN_STAGE_ALL 7
int snn_rpn_head_forward_stages(const snn_rpn_level* levels_host, int n_levels, int C, int A, int T,
                                const snn_params* p_host,
                                const void* w_shared_packed, const float* w_heads_packed,
                                float* out_logits, float* out_bbox,
                                unsigned long long* spike_counts, float* sum_logits, float* sum_bbox,
                                void* workspace, size_t workspace_bytes, int stage_mask,
                                snn_stream_t stream);

/* ---- detector (RoI) head -------------------------------------------------------------------- */
/* x[R][D] (the flattened [R][C][7][7] RoI features, faster_rcnn.py:473); out_cls[R][K],
 * out_bbox[R][K4].  Optional spike-rate outputs of the faster_rcnn.py:520-618 variant:
 *   spk6_count[R], spk7_count[R] (uint32)  spikes per RoI summed over T and the Hd neurons,
 *   sum_cls[R][K], sum_bbox[R][K4]         sum over T of the LI membranes.                      */
size_t snn_det_head_workspace_bytes(int R, int D, int Hd, int K, int K4, int T, int precision);
int snn_det_head_forward(const float* x, int R, int D, int Hd, int K, int K4, int T,
                         const snn_params* p_host,
                         const void* w6_packed, const void* w7_packed /* snn_pack_linear_weight[_bf16x3] */,
                         const float* w_heads_packed,
                         float* out_cls, float* out_bbox,
                         uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls, float* sum_bbox,
                         void* workspace, size_t workspace_bytes, snn_stream_t stream);

/* The same with fc6's weights packed in a PERMUTED reduction order (snn_pack_linear_weight_bf16x3_perm(w, N, K, inner)): w6_inner =
 * elements per channel of the flattened input (49 for [C][7][7] RoI features), k' = s * C + c instead of k = c * inner + s; the head
 * then transposes the encoder's planes to match.  Four consecutive k' are four channels at one bin (independent values) instead of
 * four neighbouring bins of one channel (correlated: equal firing periods), which is what lets fc6's sparse period planes run on the
 * structured-sparse matrix-core instruction (csrc/snn_sparse.h).  The contraction is the same sum in another order.  w6_inner = 0:
 * snn_det_head_forward.  bf16x3 precision, D % 32 == 0, C % 32 == 0; otherwise -4. */
int snn_pack_linear_weight_bf16x3_perm(const float* w_nk, int N, int K, int inner, uint16_t* packed, snn_stream_t s);
int snn_det_head_forward_k(const float* x, int R, int D, int Hd, int K, int K4, int T,
                           const snn_params* p_host,
                           const void* w6_packed, int w6_inner, const void* w7_packed,
                           const float* w_heads_packed,
                           float* out_cls, float* out_bbox,
                           uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls, float* sum_bbox,
                           void* workspace, size_t workspace_bytes, snn_stream_t stream);

/* ---- RoIAlign fused with the detector encoder (the step in front of the head, roi_heads.py:1217) --------
 * MultiScaleRoIAlign(7x7, sampling_ratio 2, aligned=False) + lif_current_encoder in one kernel: the [R,C,7,7]
 * fp32 RoI features are never materialised.  The caller assigns each RoI its FPN level (torchvision's
 * LevelMapper) and image index; rois are x1,y1,x2,y2 in (padded) image coordinates. */
typedef struct snn_roi_level {
    const float* feat;       /* [N][C][H][W] fp32 */
    int32_t H, W;
    float spatial_scale;     /* 1/4, 1/8, 1/16, 1/32 */
    int32_t reserved;
} snn_roi_level;
int snn_roi_align_encode(const snn_roi_level* levels_host, int n_levels /* <= 4 */, int C, const float* rois /*[R][4]*/,
                         const int* roi_batch /*[R]*/, const int* roi_level /*[R]*/, int R, int T,
                         const snn_params* p_host, uint32_t* planes /*[T][R][ceil(C*49/32)]*/, size_t plane_stride_words,
                         float* pooled_dbg /* nullable [R][C*49]: the pooled features, parity tests only */,
                         snn_stream_t stream);
/* snn_det_head_forward with the encoder fed by snn_roi_align_encode (D = C*49; same workspace size) */
int snn_det_head_forward_roialign(const snn_roi_level* levels_host, int n_levels, int C, const float* rois,
                                  const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                  const snn_params* p_host, const void* w6_packed, const void* w7_packed,
                                  const float* w_heads_packed, float* out_cls, float* out_bbox,
                                  uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls, float* sum_bbox,
                                  void* workspace, size_t workspace_bytes, snn_stream_t stream);

int snn_det_head_forward_roialign_k(const snn_roi_level* levels_host, int n_levels, int C, const float* rois,
                                    const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                    const snn_params* p_host, const void* w6_packed, int w6_inner, const void* w7_packed,
                                    const float* w_heads_packed, float* out_cls, float* out_bbox,
                                    uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls, float* sum_bbox,
                                    void* workspace, size_t workspace_bytes, snn_stream_t stream);

/* ---- any-time readouts: every T' of a time-step sweep from one pass ----
 * steps: host array T'_0 < ... < T'_{n-1}, each in [1, SNN_MAX_STEPS], n_steps in [1, SNN_MAX_STEPS]; the pass runs at
 * T = steps[n_steps - 1] and takes the workspace of the T call (snn_rpn_head_workspace_bytes / snn_det_head_workspace_bytes at T).
 * Every LIF state at step t depends only on steps < t and every forward starts from zero state, so the outputs of a T'-step
 * forward are the first T' steps of the T pass folded with the LI cell's kappa at T'.
 * Outputs are stacked by readout: RPN out_logits [n][P][A], out_bbox [n][P][4A] (sums alike, nullable as a pair), spike_counts
 * [n][n_levels][max_N] (nullable); detector out_cls [n][R][K], out_bbox [n][R][K4] (sums alike), spk6_count / spk7_count [n][R]
 * (nullable as a pair).  Finished rate rows: snn_rpn_rates / snn_det_rates with T = T'_j on readout j's slices.
 * Equality contract:
 *   - readout j is bit-identical to snn_li_heads at T'_j on the first T'_j spike planes of the same pass, and its counts are the
 *     popcounts of those planes; the readout at T' = T is bit-identical to the plain forward at T (outputs, sums, counts);
 *   - against a standalone forward at T' < T: the spike planes of steps < T' are identical wherever both runs take the same conv / fc6
 *     launch (the structured-sparse launches: every accumulator sees the same instructions in the same order, period planes of later
 *     steps add nothing to earlier ones); where the standalone takes another launch (dense conv at T' <= 4, SNN_SPARSE=0, ...) its
 *     currents may round differently and a neuron at its threshold may flip: equal up to those ties.
 * Bad arguments return -1 (snn_last_error) before any device work; no host synchronisation. */
int snn_li_heads_readouts(const uint32_t* spk, size_t spk_stride, const int* steps, int n_steps, int M, int K,
                          const float* w_heads_packed, int NA, int NB, const snn_params* p_host, float* out_a, float* out_b,
                          float* sum_a, float* sum_b, snn_stream_t stream);
int snn_rpn_head_forward_readouts(const snn_rpn_level* levels_host, int n_levels, int C, int A, const int* steps, int n_steps,
                                  const snn_params* p_host, const void* w_shared_packed, const float* w_heads_packed,
                                  float* out_logits, float* out_bbox, unsigned long long* spike_counts, float* sum_logits,
                                  float* sum_bbox, void* workspace, size_t workspace_bytes, snn_stream_t stream);
int snn_det_head_forward_readouts(const float* x, int R, int D, int Hd, int K, int K4, const int* steps, int n_steps,
                                  const snn_params* p_host, const void* w6_packed, int w6_inner, const void* w7_packed,
                                  const float* w_heads_packed, float* out_cls, float* out_bbox,
                                  uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls, float* sum_bbox,
                                  void* workspace, size_t workspace_bytes, snn_stream_t stream);
int snn_det_head_forward_roialign_readouts(const snn_roi_level* levels_host, int n_levels, int C, const float* rois,
                                           const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4,
                                           const int* steps, int n_steps, const snn_params* p_host, const void* w6_packed,
                                           int w6_inner, const void* w7_packed, const float* w_heads_packed, float* out_cls,
                                           float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls,
                                           float* sum_bbox, void* workspace, size_t workspace_bytes, snn_stream_t stream);

/* ---- finished spike-rate tensors of the two spike-rate variants (rpn.py:171-195, faster_rcnn.py:568-618) from the raw side
 * outputs above: rows (rate, "FLOPs") as float32, what the reference hstacks per layer.
 *   snn_rpn_rates: rates[n_levels][3][max_N][2]; [l][0] = shared-LIF spikes / (T*C*H*W) with 9*H*W*C*C, [l][1] / [l][2] = mean
 *   over (A,H,W) / (4A,H,W) of sum_t membrane / T with H*W*C*A*4 / H*W*C*A (the reference's swapped labels, kept).  Two launches.
 *   snn_det_rates: rates[4][R][2] for lif6, lif7, cls_score, bbox_pred (D*Hd, Hd*Hd, Hd*K, Hd*K*4 or Hd*K when only_one_bbox).
 * The spike counts themselves come out of the LIF epilogues of the fused kernels (ballot + popcount + integer atomics). */
size_t snn_rpn_rates_workspace_bytes(int n_levels, int max_N);
int snn_rpn_rates(const snn_rpn_level* levels_host, int n_levels, int C, int A, int T,
                  const unsigned long long* spike_counts, const float* sum_logits, const float* sum_bbox,
                  float* rates, void* workspace, size_t workspace_bytes, snn_stream_t stream);
int snn_det_rates(int R, int D, int Hd, int K, int K4, int T, int only_one_bbox, const uint32_t* spk6_count,
                  const uint32_t* spk7_count, const float* sum_cls, const float* sum_bbox, float* rates, snn_stream_t stream);

/* ---- greedy (batched) NMS for the callers either side of the heads (rpn.py:517, roi_heads.py:1160-1161) ----
 * boxes [n][4] already sorted by decreasing score; category (nullable) restricts suppression to equal values
 * (level for the RPN, class for the detector).  keep_out receives up to max_keep indices into the SORTED order,
 * in that order; *n_keep_out their number (device memory).  n <= 16384.
 * Comparison rule (here and for the nms_thresh of snn_rpn_proposals / snn_det_postprocess / snn_det_postprocess_padded): a box is
 * suppressed when the fp32 IoU is > iou_threshold, compared as floats.  The parity target (torchvision's CPU kernel) compares the
 * float IoU with a DOUBLE threshold t; to get its decisions pass the LARGEST fp32 <= t, not the nearest one - for a float IoU,
 * `iou > t` in double is `iou > that fp32`.  The nearest fp32 lies above 0.3, 0.6, 0.8 (...) and would keep a pair whose IoU
 * equals it.  ops.nms_threshold_f32 does this for every Python caller. */
size_t snn_nms_workspace_bytes(int n);
int snn_nms_sorted(const float* boxes_sorted, const int* category_sorted, int n, float iou_threshold, int max_keep,
                   int* keep_out, int* n_keep_out, void* workspace, size_t workspace_bytes, snn_stream_t stream);

/* ---- RPN proposal selection (rpn.py:420-499: per-level top-k, box decode, sigmoid, clip, size / score filters,
 * per-level NMS, post_nms_top_n) for the whole batch, no host synchronisation ---------------
 * (multi-block radix select + sort per level, decode, NMS mask and NMS walk with one list per (image, level), rank merge of the
 * kept candidates: 12 small launches)
 * Inputs are the head's own position-major outputs.  The K candidates of an image are in the reference's order (level by
 * level, inside a level by decreasing logit as objectness.topk returns them, equal logits by element index); pre_boxes /
 * pre_prob report them in that order (rpn.py:493-499).  Equal sigmoid values keep that order in the NMS walk, like the
 * reference's stable sort.  Outputs are padded to post_nms_top_n rows, out_counts[N] holds the valid rows. */
typedef struct {
    const float* logits;        /* [N*H*W][A]  objectness logits, rows n*H*W + y*W + x                  */
    const float* deltas;        /* [N*H*W][4A] box regression                                           */
    int32_t H, W;
    float stride_h, stride_w;   /* image size // feature size (AnchorGenerator)                         */
    float base_anchors[16][4];  /* the level's cell anchors (rounded, as AnchorGenerator builds them)   */
} snn_rpn_post_level;
int snn_rpn_proposals_candidates(const snn_rpn_post_level* levels, int n_levels, int A, int pre_nms_top_n);
size_t snn_rpn_proposals_workspace_bytes(int N, int K_candidates);
int snn_rpn_proposals(const snn_rpn_post_level* levels, int n_levels, int N, int A, const float* image_hw_host,
                      int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float score_thresh, float min_size,
                      float* out_boxes, float* out_scores, int* out_counts,
                      float* pre_boxes /* nullable [N][K][4]: decoded un-clipped candidates */,
                      float* pre_prob /* nullable [N][K] */, void* workspace, size_t workspace_bytes,
                      snn_stream_t stream);

/* ---- detection post-processing (roi_heads.py:1075-1176, incl. the reference's background-box report): softmax,
 * per-class box decode, clip, score / size filters, per-class NMS (one list per (image, class)), detections_per_img - five
 * launches for the batch, no host synchronisation.  Rows of image i in out_* [N][out_cap]: out_counts[2i] foreground
 * detections by decreasing score, then out_counts[2i+1] background boxes (RoIs without any class above the score
 * threshold).  all_scores [R][K] / all_boxes [R][K][4] receive the softmax scores and clipped boxes of every class.
 * out_cap >= detections_per_img + max RoIs per image; max RoIs per image <= 10240, K <= 96 and
 * (K-1) * detections_per_img <= 8192, else -4. */
size_t snn_det_postprocess_workspace_bytes(int N, int max_rois_per_image, int K);
int snn_det_postprocess(const float* class_logits, const float* box_regression, const float* proposals,
                        const int* rois_per_image_host, int N, int K, const float* image_hw_host,
                        const float* box_weights_host /* [4]: BoxCoder weights, (10, 10, 5, 5) in the reference */,
                        float score_thresh, float nms_thresh, int detections_per_img, float min_size,
                        float* all_scores, float* all_boxes, float* out_boxes, float* out_scores, int* out_labels,
                        int* out_counts, int out_cap, void* workspace, size_t workspace_bytes, snn_stream_t stream);

/* ---- static-shape path: FPN features -> padded detections with no host synchronisation -------------
 * snn_rpn_proposals already leaves [N][post_nms_top_n][4] padded rows and out_counts[N] in device memory.  The two calls below take
 * that layout on: every per-image row count is READ ON THE DEVICE and clamped to 0 .. cap there (a garbage count never indexes out
 * of bounds), shapes depend on (N, cap) alone, nothing waits for the host: the sequence snn_rpn_head_forward, snn_rpn_proposals,
 * snn_roi_assign, snn_det_head_forward_roialign, snn_det_postprocess_padded runs from the FPN features to the detections on one stream,
 * and snn_pack_padded_detections (below, behind snn_det_exchange_payload) turns them into fixed-size exchange rows as a sixth call.
 * Bad arguments return -1 (limits: -4) before any device work.
 *
 * snn_roi_assign: the RoI table of snn_det_head_forward_roialign from padded proposals, one launch.  Row r = i * cap + j:
 * roi_batch[r] = i; for j < clamp(counts[i], 0, cap) rois[r] = boxes[r] and roi_level[r] = torchvision's LevelMapper,
 *   clamp(floor(canonical_level + log2(sqrt((x2 - x1) * (y2 - y1)) / canonical_scale) + 1e-6), k_min, k_max) - k_min
 * in fp32 in that operation order (a zero-area box gives -inf and therefore k_min); the other rows are NOT read and become the box
 * (0, 0, 0, 0) on level 0.  N <= 64, cap <= 10240, k_min <= k_max < k_min + 8, canonical_scale > 0 (the reference: 224, level 4). */
int snn_roi_assign(const float* boxes /* [N][cap][4] */, const int* counts_dev /* [N] */, int N, int cap, int k_min, int k_max,
                   float canonical_scale, float canonical_level, float* rois /* [N*cap][4] */, int32_t* roi_batch /* [N*cap] */,
                   int32_t* roi_level /* [N*cap] */, snn_stream_t stream);

/* snn_det_postprocess_padded: snn_det_postprocess for rows laid out [N][cap] (class_logits [N*cap][K], box_regression [N*cap][4K],
 * proposals [N*cap][4]) with the rows per image in device memory; workspace snn_det_postprocess_workspace_bytes(N, cap, K).
 * With c_i = clamp(roi_counts_dev[i], 0, cap): out_boxes / out_scores / out_labels / out_counts are bit-identical to snn_det_postprocess
 * on the concatenation of the first c_i rows of every image (rois_per_image_host = c); all_scores [N*cap][K] / all_boxes [N*cap][K][4]
 * are bit-identical on those rows and zero on the others; output rows behind the out_counts[2i] + out_counts[2i+1] rows of an image are
 * zero.  Padding rows are never read.  cap <= 10240, (K-1) * min(detections_per_img, cap) <= 8192 (else -4), out_cap >=
 * detections_per_img + cap.  Six launches. */
int snn_det_postprocess_padded(const float* class_logits, const float* box_regression, const float* proposals,
                               const int* roi_counts_dev /* [N] */, int N, int cap, int K, const float* image_hw_host,
                               const float* box_weights_host, float score_thresh, float nms_thresh, int detections_per_img,
                               float min_size, float* all_scores, float* all_boxes, float* out_boxes, float* out_scores,
                               int* out_labels, int* out_counts, int out_cap, void* workspace, size_t workspace_bytes,
                               snn_stream_t stream);

/* ---- exchange payload of the data-parallel path: what each rank hands to the ONE all-gather of a batch (the reference's
 * counterpart is the pickled all_gather_object of coco_eval.py:158-177, disabled under NCCL at train.py:874-880).  Per
 * image the max_det RoIs with the highest foreground score (softmax over K, best class >= 1; the selection of
 * roi_heads.py:1103-1110 without NMS) as rows (the 4 regression values of that class, score, label) by decreasing
 * score, ties by RoI index; counts[i] = min(max_det, rois_per_image).  One launch; rois_per_image <= 4096. */
int snn_det_exchange_payload(const float* class_logits /* [N*rois_per_image][K] */,
                             const float* box_regression /* [N*rois_per_image][4K] */, int N, int rois_per_image, int K,
                             int max_det, float* payload /* [N][max_det][6] */, int* counts /* [N] */, snn_stream_t stream);

/* ---- padded detections -> exchange rows: the sixth call of the static-shape path --------------------------------
 * out_* of snn_det_postprocess_padded -> the rows of dp.pack_detections, payload [N][max_det][6] fp32 (x1, y1, x2, y2, score, label) and counts [N]:
 * the one fixed-size record a deployment copies to pinned memory or hands to the all-gather, formed without the host reading a count.
 *   k_i = min(clamp(out_counts[i][0] + out_counts[i][1], 0, out_cap), max_det)        (on the device; the sum in 64 bits)
 *   payload[i][r] = (out_boxes[i][r], out_scores[i][r], (float)out_labels[i][r]) for r < k_i, six zeros for r >= k_i;  counts[i] = k_i.
 * Input rows at or past k_i are never read; every element of payload and counts is written on every call, so the outputs depend on the
 * inputs alone.  One launch, no workspace, stream-only, capturable.  out_boxes 16-byte aligned, payload 8-byte aligned (16-byte stores
 * when max_det is even and payload is 16-byte aligned).  Bad arguments (N < 1 or > 64, out_cap < 1, max_det < 1, a null or misaligned
 * pointer) return -1 before any device work; max_det > 2^24 (counts travel as fp32) returns -4. */
int snn_pack_padded_detections(const float* out_boxes /* [N][out_cap][4] */, const float* out_scores /* [N][out_cap] */,
                               const int32_t* out_labels /* [N][out_cap] */, const int32_t* out_counts /* [N][2], device */, int N,
                               int out_cap, int max_det, float* payload /* [N][max_det][6] */, int32_t* counts /* [N] */,
                               snn_stream_t stream);

/* ---- helper outside the spiking path: FrozenBatchNorm2d (+ residual) (+ ReLU) of the stock backbone in one pass -----
 * y[n][c][i] = relu?( (x[n][c][i] * scale[c] + bias[c]) (+ residual[n][c][i]) ), the operations of torchvision's
 * FrozenBatchNorm2d.forward / Bottleneck.forward (called at faster_rcnn.py:693-694 through resnet_fpn_backbone) in the same
 * order with separate roundings: bit-identical to the four torch launches it replaces.  residual nullable; y may be x. */
int snn_affine_act_nchw(const float* x, const float* scale, const float* bias, const float* residual, int N, int C,
                        int HW, int relu, float* y, snn_stream_t stream);

/* ---- stage-level entry points (parity tests drive the layers one by one, teacher-forced) ----- */
/* constant-current LIF encoder -> bit-planes.  NCHW feature map -> planes[T][N*H*W][Cw]          */
int snn_encode_nchw(const float* feat, int N, int C, int H, int W, int T, const snn_params* p_host,
                    uint32_t* planes, size_t plane_stride_words, snn_stream_t stream);
/* row-major x[R][D] -> planes[T][R][Dw]                                                          */
int snn_encode_rows(const float* x, int R, int D, int T, const snn_params* p_host,
                    uint32_t* planes, size_t plane_stride_words, snn_stream_t stream);
/* fused 3x3 spike convolution + LIF over T for ONE level: enc planes [T][N*H*W][Cw] ->
 * spk planes [T][N*H*W][Nw]; counts[N] nullable; dbg_cur (nullable, parity tests only) receives the
 * shared-LIF input currents [T][N*H*W][Nw*32] fp32                                               */
int snn_conv3x3_lif(const uint32_t* enc, size_t enc_stride_words, int N, int C_in, int C_out, int H, int W,
                    int T, const snn_params* p_host, const float* w_packed,
                    uint32_t* spk, size_t spk_stride_words, unsigned long long* counts, float* dbg_cur,
                    snn_stream_t stream);
/* time-batched spike GEMM: A planes as [M][Kw] rows -> cur[M][ldo] fp32 (ldo >= Np)              */
int snn_spike_gemm(const uint32_t* a_rows, int M, int K, int N, const float* w_packed, float* cur,
                   int ldo, snn_stream_t stream);
/* LIF scan over T of currents cur[T][R][ldc] -> spk planes [T][R][Nw]; row_counts[R] nullable     */
int snn_lif_scan(const float* cur, int T, int R, int N, int ldc, const snn_params* p_host,
                 uint32_t* spk, size_t spk_stride_words, uint32_t* row_counts, snn_stream_t stream);
/* leaky-integrator heads on spike planes [T][M][Kw]: out_a[M][NA], out_b[M][NB] = LI membranes at
 * the last step; sum_a / sum_b (nullable) = their sums over the T steps                           */
int snn_li_heads(const uint32_t* spk, size_t spk_stride_words, int T, int M, int K,
                 const float* w_heads_packed, int NA, int NB, const snn_params* p_host,
                 float* out_a, float* out_b, float* sum_a, float* sum_b, snn_stream_t stream);

/* ---- exact bf16x3 contractions (bf16 matrix cores, fp32-exact result) -------------------------------
 * Spikes are exactly {0,1} and every fp32 weight is exactly the sum of three bf16 values, so
 * A x W = A x W_hi + A x W_mid + A x W_lo with every product exact and fp32 accumulation; measured as
 * accurate as the fp32 MFMA chain (tools/bf16x3_numerics.hip).  Packed operand: uint16 [3][K/32][Np][32]. */
size_t snn_packed_bf16x3_elems(int K_chunks32, int N);
size_t snn_packed_conv3x3_bf16x3_elems(int C_out, int C_in);
int snn_pack_conv3x3_weight_bf16x3(const float* w_oihw, int C_out, int C_in, uint16_t* packed, snn_stream_t s);
size_t snn_packed_linear_bf16x3_elems(int N, int K);
int snn_pack_linear_weight_bf16x3(const float* w_nk, int N, int K, uint16_t* packed, snn_stream_t s);
/* Single bf16 plane (SNN_PRECISION_BF16): uint16 [K/32][Np][32], each element the bf16 nearest to the fp32 weight (ties to even, subnormal results
 * kept: bit for bit torch's w.to(torch.bfloat16)) - the *_elems counts are a third of the bf16x3 ones.  The _perm form packs fc6 in bin-major order
 * as snn_pack_linear_weight_bf16x3_perm does.  A tensor with a non-finite weight or one that rounds to +-inf is REFUSED: the call returns -4
 * (snn_last_error) - there is no other precision that computes the same thing to fall back to.  To deliver that verdict these three calls wait
 * for the stream (pack time only) and are NOT hipGraph-capturable (Conventions).  Bad arguments return -1 before any device work.
 * The LI heads have NO packer of their own at this precision: they keep snn_pack_heads_weight and its layout, and the CALLER rounds the two
 * head weight matrices to bf16 (ties to even) and back to fp32 before that call, and refuses non-finite results itself - as the Python
 * binding's ops.pack_heads_bf16 does.  Head weights passed unrounded run unrounded: the result is then not this mode's. */
size_t snn_packed_bf16_elems(int K_chunks32, int N);
size_t snn_packed_conv3x3_bf16_elems(int C_out, int C_in);
int snn_pack_conv3x3_weight_bf16(const float* w_oihw, int C_out, int C_in, uint16_t* packed, snn_stream_t s);
size_t snn_packed_linear_bf16_elems(int N, int K);
int snn_pack_linear_weight_bf16(const float* w_nk, int N, int K, uint16_t* packed, snn_stream_t s);
int snn_pack_linear_weight_bf16_perm(const float* w_nk, int N, int K, int inner, uint16_t* packed, snn_stream_t s);
/* Block-scaled fp6 digit planes (precision "mxfp6", csrc/snn_mx.h): the fp32 weights as 6 planes of signed base-32
 * digits in fp6 e2m3 with one E8M0 scale per (32 consecutive k, column).  Exact for every weight within 2^5 of the
 * largest magnitude of its block, else rounded at 2^-28 of that magnitude.  Packed operand: uint32 words. */
size_t snn_packed_linear_mx_words(int N, int K);
size_t snn_packed_conv3x3_mx_words(int C_out, int C_in);
int snn_pack_linear_weight_mx(const float* w_nk, int N, int K, uint32_t* packed, snn_stream_t s);
int snn_pack_conv3x3_weight_mx(const float* w_oihw, int C_out, int C_in, uint32_t* packed, snn_stream_t s);
/* the spike GEMMs on the fp4 x fp6 block-scaled matrix path (k_gemm_mx); K / C_in must be a multiple of 128 (-4 else),
 * same operands and results as the _bf16x3 entry points - except that the two conv entry points read encoder planes
 * with a one-position ZERO HALO around every image (row (n, y, x) of an H x W level at (n (H+2) + y+1) (W+2) + x+1,
 * levels back to back, enc_stride >= sum N (H+2) (W+2) C_in/32 words): 3x3 taps then need no border logic */
int snn_spike_gemm_mx(const uint32_t* a_rows, int M, int K, int N, const uint32_t* w_packed, float* cur, int ldo,
                      snn_stream_t stream);
int snn_spike_gemm_lif_mx(const uint32_t* a_planes, int T, int R, int K, int N, const snn_params* p,
                          const uint32_t* w_packed, uint32_t* spk, size_t spk_stride, snn_stream_t stream);
int snn_conv3x3_lif_mx(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in, int C_out,
                       int T, const snn_params* p, const uint32_t* w_packed, uint32_t* spk, size_t spk_stride,
                       snn_stream_t stream);
int snn_spike_conv3x3_mx(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in,
                         int C_out, int T, const uint32_t* w_packed, float* cur, int ldo, snn_stream_t stream);
/* cur[M][ldo] = A_bits[M][K] x W[K][N] */
int snn_spike_gemm_bf16x3(const uint32_t* a_rows, int M, int K, int N, const uint16_t* w_packed, float* cur,
                          int ldo, snn_stream_t stream);
/* Linear layer + LIF over all T steps in one launch (faster_rcnn.py:498-499 / 500-501): a_planes [T][R][K/32] spike
 * bit-planes in, spk [T][R][N/32 words] out (spk_stride = words per time plane).  A row tile of the GEMM holds all T
 * steps of its RoIs, so the input currents and the LIF state never leave the chip.  Returns -4 when T does not fit a
 * row tile (T > 64 or a poor divisor of 256/192/128): use snn_spike_gemm_bf16x3 + snn_lif_scan then. */
int snn_spike_gemm_lif_bf16x3(const uint32_t* a_planes, int T, int R, int K, int N, const snn_params* p,
                              const uint16_t* w_packed, uint32_t* spk, size_t spk_stride, snn_stream_t stream);
/* 3x3 spike convolution + LIF fused over T on the bf16 matrix cores, all levels in one launch:
 * enc planes [T][P][Cw] -> spk planes [T][P][Nw]; the membrane state never leaves the registers */
int snn_conv3x3_lif_bf16x3(const uint32_t* enc, size_t enc_stride_words, const snn_rpn_level* levels_host,
                           int n_levels, int C_in, int C_out, int T, const snn_params* p_host,
                           const uint16_t* w_packed, uint32_t* spk, size_t spk_stride_words, snn_stream_t stream);
/* un-fused time-batched 3x3 spike convolution over all levels: enc planes [T][P][Cw] -> cur[T*P][ldo]
 * (row = t*P + position; position order as in snn_rpn_head_forward); follow with snn_lif_scan */
int snn_spike_conv3x3_bf16x3(const uint32_t* enc, size_t enc_stride_words, const snn_rpn_level* levels_host,
                             int n_levels, int C_in, int C_out, int T, const uint16_t* w_packed, float* cur,
                             int ldo, snn_stream_t stream);

/* ---- half-precision feature maps: fp16 / bf16 features straight into both heads --------------------------------------------------------
 * The *_typed twins of the entry points that READ features take them as `const void*` plus a feat_dtype.  A feature element of dtype
 * SNN_FEAT_F16 / SNN_FEAT_BF16 means its exact fp32 value (both widenings are exact: subnormals, +-0, +-inf and NaN included): the encoder
 * kernels load the 16-bit element and widen it in registers; neuron arithmetic, RoIAlign interpolation, thresholds and every output stay
 * fp32, and the call returns bit for bit what the fp32 entry returns for the widened tensor.  (This is NOT fp16 arithmetic: nothing is
 * computed in half precision.)  With SNN_FEAT_F32 a typed entry IS the fp32 entry - the same launches - and the entries without the
 * suffix are one-line calls of it.
 *   - struct layouts are unchanged: the `feat` members of snn_rpn_level / snn_roi_level then point at 16-bit elements;
 *   - alignment: a half-precision feature base pointer (x, every level's feat) must be 16-byte aligned, else -1 (fp32 pointers: as
 *     before); inside the kernels no load is wider than the element address guarantees (RoIAlign's x-adjacent tap pairs are two
 *     2-byte loads: an element address is only 2-byte aligned where W or y W + x is odd);
 *   - workspace sizes do not depend on the feature dtype;
 *   - typed kernels exist for the encoders the default plans launch (all levels of the RPN head; the fused RoIAlign encoders on
 *     word-major planes; the row encoders on word-major planes).  Where the launch plan of the call picks another encoder kernel
 *     (knob-selected legacy kernels such as SNN_ROI_TAB=0, row-major planes: SNN_PRECISION_F32 / SNN_PLANES=rm detector heads,
 *     D % 32 != 0) a typed entry with half features returns SNN_STATUS_NO_TYPED_KERNEL (> 0: not an error, snn_last_error is not set) and
 *     enqueues NOTHING; the caller widens the features to fp32 and calls again with SNN_FEAT_F32. */
enum { SNN_FEAT_F32 = 0, SNN_FEAT_F16 = 1, SNN_FEAT_BF16 = 2 };
#define SNN_STATUS_NO_TYPED_KERNEL 1
/* ---- channels-last (NHWC) feature maps ---------------------------------------------------------------------------------------------------
 * SNN_FEAT_NHWC is a LAYOUT bit, OR-ed into the feat_dtype of the typed entries that read feature MAPS (both snn_rpn_head_forward_*_typed,
 * both snn_det_head_forward_roialign_*_typed, snn_encode_nchw_typed).  With the bit every `feat` pointer of the call addresses [N][H][W][C]
 * elements of the dtype in the low bits - what data_ptr() of a dense channels-last [N, C, H, W] tensor addresses.  The layout is per call, not
 * per level; struct layouts and workspace sizes are unchanged, and the call returns bit for bit what it returns for the same values in NCHW.
 *   - alignment: an NHWC base pointer must be 16-byte aligned for EVERY dtype, else -1;
 *   - the row-fed entries (snn_det_head_forward_k_typed, snn_det_head_forward_readouts_typed) return -1 with the bit: pooled rows have no layout;
 *   - snn_roi_align_encode_typed returns SNN_STATUS_NO_TYPED_KERNEL with the bit (flatten-order planes are not built for NHWC);
 *   - NHWC kernels exist for C % 32 == 0 (the level / stage encoders) and, for the RoIAlign-fed detector head, for the plans in which fc6 reads
 *     bin-major period planes (w6_inner == 49, word-major planes, threshold-form encoder, C % 64 == 0, SNN_ROI_TAB != 0).  Any other plan returns
 *     SNN_STATUS_NO_TYPED_KERNEL with nothing enqueued; the caller converts the maps to NCHW and calls again without the bit.
 * Without the bit SNN_FEAT_* behave exactly as before. */
#define SNN_FEAT_NHWC 16
int snn_rpn_head_forward_stages_typed(const snn_rpn_level* levels_host, int feat_dtype, int n_levels, int C, int A, int T,
                                      const snn_params* p_host, const void* w_shared_packed, const float* w_heads_packed,
                                      float* out_logits, float* out_bbox, unsigned long long* spike_counts, float* sum_logits,
                                      float* sum_bbox, void* workspace, size_t workspace_bytes, int stage_mask, snn_stream_t stream);
int snn_rpn_head_forward_readouts_typed(const snn_rpn_level* levels_host, int feat_dtype, int n_levels, int C, int A, const int* steps,
                                        int n_steps, const snn_params* p_host, const void* w_shared_packed, const float* w_heads_packed,
                                        float* out_logits, float* out_bbox, unsigned long long* spike_counts, float* sum_logits,
                                        float* sum_bbox, void* workspace, size_t workspace_bytes, snn_stream_t stream);
int snn_det_head_forward_k_typed(const void* x, int feat_dtype, int R, int D, int Hd, int K, int K4, int T, const snn_params* p_host,
                                 const void* w6_packed, int w6_inner, const void* w7_packed, const float* w_heads_packed,
                                 float* out_cls, float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls,
                                 float* sum_bbox, void* workspace, size_t workspace_bytes, snn_stream_t stream);
int snn_det_head_forward_readouts_typed(const void* x, int feat_dtype, int R, int D, int Hd, int K, int K4, const int* steps, int n_steps,
                                        const snn_params* p_host, const void* w6_packed, int w6_inner, const void* w7_packed,
                                        const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                        uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* workspace, size_t workspace_bytes,
                                        snn_stream_t stream);
int snn_det_head_forward_roialign_k_typed(const snn_roi_level* levels_host, int feat_dtype, int n_levels, int C, const float* rois,
                                          const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                          const snn_params* p_host, const void* w6_packed, int w6_inner, const void* w7_packed,
                                          const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                          uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* workspace,
                                          size_t workspace_bytes, snn_stream_t stream);
int snn_det_head_forward_roialign_readouts_typed(const snn_roi_level* levels_host, int feat_dtype, int n_levels, int C, const float* rois,
                                                 const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4,
                                                 const int* steps, int n_steps, const snn_params* p_host, const void* w6_packed,
                                                 int w6_inner, const void* w7_packed, const float* w_heads_packed, float* out_cls,
                                                 float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls,
                                                 float* sum_bbox, void* workspace, size_t workspace_bytes, snn_stream_t stream);
/* ---- conv route of the RPN head (opt-in, per call) -------------------------------
 * The shared 3x3 conv + LIF has two launch plans for the bf16x3 family: the structured-sparse one (period planes e_3 .. compressed; its cost
 * grows with the share of 16-row tiles that hold a third or fourth spike of one period in a nibble) and the all-dense one (cost independent of
 * the input).  snn_rpn_head_forward_routed is snn_rpn_head_forward_stages_typed at SNN_STAGE_ALL with the choice made per call:
 *   SNN_ROUTE_SPARSE  today's plan: the launches of snn_rpn_head_forward, bit for bit
 *   SNN_ROUTE_DENSE   the all-dense plan for this call (what SNN_SPARSE=0 selects for a process), bit for bit
 *   SNN_ROUTE_AUTO    decided ON THE DEVICE from the input, no host read: the encoder leaves every period plane raw; one launch compresses
 *                     the planes e_3 .. and counts, with integer atomics, the HITS among the BLOCKS - block = 16 consecutive rows of the
 *                     padded row space (aligned to 16 within the Pe = sum N (H + 2)(W + 2) rows of a word plane; blocks run across image
 *                     and level boundaries and include halo rows) x one 64-channel word pair x one compressed plane; hit = a block in which
 *                     some row's secondary-occupancy dword is non-zero; one thread sets route = (float)hits > crossover * (float)blocks ? 1 : 0;
 *                     then BOTH conv launches are enqueued and the one whose route was not taken leaves at entry.  The route is a function
 *                     of the input alone; the two sides write the same spike-plane layout and may differ only where the sparse and the dense
 *                     plan may (threshold ties of the fp32 sums taken in another order).  crossover <= -1 always takes the dense side,
 *                     crossover >= 1 never does.
 * route_stat (device, int32[4], written on `stream`; nullable unless AUTO) = {hits, blocks, route taken (0 sparse / 1 dense), 0}.
 * Where the call's plan is not the sparse one anyway (SNN_PRECISION_F32 / F32_STRICT / MXFP6, T outside 5 .. 16, a channel count whose padded
 * words are odd in number or whose 64-column blocks are not 1, 2 or 4 - 3, 192, 320 -, non-zero rest or reset potentials, knobs), all three
 * routes run that plan and route_stat = {0, 0, 1, 0}.  In spike-rate mode (spike_counts != NULL) all three routes run the plan of
 * snn_rpn_head_forward and route_stat = {0, 0, 0, 0}.  SPARSE and DENSE count nothing either: route_stat = {0, 0, 0 / 1, 0}.
 * The workspace is the plain forward's (its plane sets hold the raw planes of every period and the compressed planes; the gate word is
 * route_stat[2]); the _routed size query exists so that this can change.  An unknown route, a null route_stat with AUTO and a workspace
 * below the query's size return -1 with nothing enqueued.  SNN_ROUTE_DEFAULT_CROSSOVER: see profiles/route_crossover.txt. */
#define SNN_ROUTE_SPARSE 0
#define SNN_ROUTE_DENSE 1
#define SNN_ROUTE_AUTO 2
#define SNN_ROUTE_DEFAULT_CROSSOVER 0.357f
size_t snn_rpn_head_workspace_bytes_routed(const snn_rpn_level* levels_host, int n_levels, int C, int A, int T, int precision, int route);
int snn_rpn_head_forward_routed(const snn_rpn_level* levels_host, int feat_dtype, int n_levels, int C, int A, int T,
                                const snn_params* p_host, const void* w_shared_packed, const float* w_heads_packed,
                                float* out_logits, float* out_bbox, unsigned long long* spike_counts, float* sum_logits,
                                float* sum_bbox, void* workspace, size_t workspace_bytes, int route, float crossover,
                                int32_t* route_stat, snn_stream_t stream);

/* ---- fc6 route of the detector head (opt-in, per call) --------------------------------
 * fc6 + LIF has the same two launch plans for the bf16x3 family on bin-major period planes (reduction order k' = bin * C + c, w6_inner = 49):
 * the structured-sparse one, whose cost grows with the share of 16-RoI tiles that hold a third or fourth spike of one period in a nibble,
 * and the all-dense one.  snn_det_head_forward_routed is snn_det_head_forward_k_typed, snn_det_head_forward_roialign_routed is
 * snn_det_head_forward_roialign_k_typed, each with the choice made per call (SNN_ROUTE_* above):
 *   SNN_ROUTE_SPARSE  the plain entry's launches, bit for bit
 *   SNN_ROUTE_DENSE   what a process started with SNN_SPARSE=0 runs for this call, bit for bit
 *   SNN_ROUTE_AUTO    decided ON THE DEVICE, no host read: the encoder leaves every period plane raw (no fold; channels-last RoIAlign input:
 *                     the raw bin-major form), k_permute_planes brings the planes into bin-major order where they are not, one launch
 *                     compresses the planes e_3 .. and counts the HITS among the BLOCKS - block = 16 consecutive RoIs (cut every 16 rows
 *                     from row 0; the last block is short; rows of a plane stride beyond R belong to no block) x one 64-k word pair of the
 *                     bin-major order (D / 64 of them) x one compressed plane e_n, n = 3 .. fc6's window; hit = a block in which some row's
 *                     secondary-occupancy dword is non-zero (some nibble of that plane holds at least three ones) -, one thread sets
 *                     route = (float)hits > crossover * (float)blocks ? 1 : 0, then BOTH fc6 launches are enqueued on the same raw planes
 *                     and permuted weights and the one whose route was not taken leaves at entry; fc7 and the LI heads follow as always.
 *                     crossover <= -1 always takes the dense side, crossover >= 1 never does.
 * route_stat (device, int32[4], written on `stream`; nullable unless AUTO) = {hits, blocks, route taken (0 sparse / 1 dense), 0}.
 * SPARSE and DENSE count nothing: route_stat = {0, 0, 0 / 1 = the fc6 launch that ran, 0}.  Where the call's fc6 plan is dense anyway
 * (SNN_PRECISION_F32 / F32_STRICT / MXFP6, C % 64 != 0, a non-zero rest or reset potential, a lif6 that fires at step 0, knobs), all three
 * routes run that plan and route_stat = {0, 0, 1, 0}.  With w6_inner != 49 AUTO decides nothing and runs the plain plan (route_stat[2] says
 * which launch that was).  In spike-rate mode (spk6_count != NULL) all three routes run the plain plan and route_stat = {0, 0, 0, 0}.
 * The workspace is the plain forward's; the _routed size query exists so that this can change.  An unknown route, a null route_stat with
 * AUTO and a workspace below the query's size return -1 with nothing enqueued.  The readout entries have no route.
 * SNN_FC6_ROUTE_DEFAULT_CROSSOVER: see profiles/fc6_route_crossover.txt. */
#define SNN_FC6_ROUTE_DEFAULT_CROSSOVER 0.061f
size_t snn_det_head_workspace_bytes_routed(int R, int D, int Hd, int K, int K4, int T, int precision, int route);
int snn_det_head_forward_routed(const void* x, int feat_dtype, int R, int D, int Hd, int K, int K4, int T, const snn_params* p_host,
                                const void* w6_packed, int w6_inner, const void* w7_packed, const float* w_heads_packed,
                                float* out_cls, float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count, float* sum_cls,
                                float* sum_bbox, void* workspace, size_t workspace_bytes, int route, float crossover,
                                int32_t* route_stat, snn_stream_t stream);
int snn_det_head_forward_roialign_routed(const snn_roi_level* levels_host, int feat_dtype, int n_levels, int C, const float* rois,
                                         const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                         const snn_params* p_host, const void* w6_packed, int w6_inner, const void* w7_packed,
                                         const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                         uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* workspace, size_t workspace_bytes,
                                         int route, float crossover, int32_t* route_stat, snn_stream_t stream);

/* the two stage-level calls the tests compare planes through */
int snn_encode_nchw_typed(const void* feat, int feat_dtype, int N, int C, int H, int W, int T, const snn_params* p_host,
                          uint32_t* planes, size_t plane_stride_words, snn_stream_t stream);
int snn_roi_align_encode_typed(const snn_roi_level* levels_host, int feat_dtype, int n_levels, int C, const float* rois,
                               const int* roi_batch, const int* roi_level, int R, int T, const snn_params* p_host, uint32_t* planes,
                               size_t plane_stride_words, float* pooled_dbg, snn_stream_t stream);

/* ---- spike taps: rasters and activity statistics of the hidden LIF layers -------------------------------------------
 * A head pass leaves the spike planes of its hidden LIF layers - the RPN's shared LIF, the detector's lif6 and lif7 - in the CALLER's
 * workspace.  The two *_planes_view calls say where and in which layout; the three tap calls read planes through such a view.
 *
 * snn_planes_view: `steps_formed` steps of `rows` x `words` 32-bit words (bit b of word w = spike of column 32 w + b; rows = P positions in
 * the order of the head's outputs, or R RoIs), step t at word offset t * step_stride_words behind workspace + offset_bytes, inside a step:
 *   SNN_PLANES_ROWS        word w of row r at  r * words + w
 *   SNN_PLANES_SPLIT4      ... at  ((w / 4) * rows + r) * 4 + w % 4     (blocks of four words; words % 4 == 0)
 *   SNN_PLANES_WORD_MAJOR  ... at  w * rows + r
 * These three are all the layouts a head pass writes today, for every precision and every SNN_PLANES setting; a further layout would
 * be a further enumerator.  The view queries are HOST-ONLY (no stream, no device work, no workspace pointer): they are answered from the
 * arguments of the pass by the plan code the forward itself runs, so a pass with these arguments and an unchanged environment (the SNN_*
 * knobs) leaves its planes exactly there.  The arguments are those of the forward; `route` is the SNN_ROUTE_* of a *_routed entry
 * (SNN_ROUTE_SPARSE for every other entry); spike_rates != 0: the pass is handed the spike-rate side outputs (spike_counts /
 * spk6_count non-null).  The row-fed detector entries take word-major planes only for a 16-byte aligned x; the view assumes one.
 * offset_bytes + T * step_stride_words * 4 never exceeds the matching snn_*_workspace_bytes[_routed] size.
 *
 * steps_formed = the number of leading steps whose planes the pass FORMS.  A pass computes no more than its outputs need (dead time
 * steps: an input current first moves a spike one step later).  Without the side outputs lif6's spikes of the last step reach nothing -
 * fc7's current of step T - 1 cannot move a lif7 spike any more - so fc6 forms the currents of steps 0 .. T - 3 only, and lif6's plane
 * of step T - 1 is integrated without its input: steps_formed = T - 1 for T >= 3 (snn_debug_tile_shape reports the same window).  With
 * the side outputs every spike is counted, fc6's window is one step longer and all T planes are formed.  The shared LIF and lif7 feed
 * LI cells that read every step, in both update orders (the passes do not shorten the last step under li_order = 1), so their
 * steps_formed is T.  A tap on steps at or past steps_formed returns -1 with nothing enqueued.
 *
 * There is no separate "tapped" forward: the pass to tap for statistics is the existing spike-rate-mode pass (side outputs non-null),
 * which returns outputs, counts and time sums together.  The planes stay valid until the next call that is handed the same workspace.
 *
 * The taps (all three: every output nullable, enqueued on `stream`, no host synchronisation, hipGraph-capturable under the capture
 * contract above; bad arguments - a null workspace or view, an unknown layout, T' outside 1 .. steps_formed, shapes outside the view -
 * return -1 before any device work):
 *   snn_planes_counts       spike counts of the steps t < T' over `n_groups` groups of rows; group g = rows group_row_start_host[g] ..
 *                           group_row_start_host[g + 1] - 1 (host array of n_groups + 1 non-decreasing values within 0 .. rows: an image
 *                           of a level for the RPN, an image's RoIs for the detector; n_groups <= 512, rows < 2^31).
 *                             per_step uint64 [T'][n_groups]       spikes of step t in group g
 *                             per_col  uint32 [n_groups][n_cols]   spikes of column c in group g, summed over its rows and the T' steps
 *                             per_row  uint32 [rows]               spikes of row r, summed over the columns and the T' steps (rows outside
 *                                                                  every group: 0)
 *                           n_cols <= 32 * words (<= 8192); bits at or above n_cols - the padding of a row's last word - are never
 *                           counted.  The counters are cleared by work of this call on the stream.
 *   snn_planes_raster_nchw  one RPN level as bytes {0, 1}: out [T'][N][C][H][W], channel c of position (n, y, x) = bit c of row
 *                           row0 + (n H + y) W + x (row0 = the level's first row: sum of N H W of the levels before it).
 *   snn_planes_raster_rows  out [T'][rows][n_cols], byte (t, r, c) = bit c of row r.
 * Encoder planes are not part of this: most plans keep them as period planes or compressed.  snn_encode_nchw / snn_encode_rows return
 * them on request as [T][rows][words], and the raster calls read that output with a hand-filled view {0, rows * words, rows, words,
 * SNN_PLANES_ROWS, T, 0} and the plane tensor as `workspace`. */
enum { SNN_PLANES_ROWS = 0,        /* [T][rows][words]                       */
       SNN_PLANES_SPLIT4 = 1,      /* [T][words/4][rows][4]                  */
       SNN_PLANES_WORD_MAJOR = 2   /* [T][words][rows]                       */ };
typedef struct snn_planes_view {
    uint64_t offset_bytes;         /* into the caller's workspace            */
    uint64_t step_stride_words;
    int64_t  rows;                 /* P or R                                 */
    int32_t  words, layout, steps_formed, reserved;
} snn_planes_view;
int snn_rpn_head_planes_view(const snn_rpn_level* levels_host, int n_levels, int C, int A, int T, const snn_params* p_host, int route,
                             int spike_rates, snn_planes_view* shared_lif);
int snn_det_head_planes_view(int R, int D, int Hd, int K, int K4, int T, const snn_params* p_host, int w6_inner, int route,
                             int spike_rates, snn_planes_view* lif6, snn_planes_view* lif7 /* either may be null */);
int snn_planes_counts(const void* workspace, const snn_planes_view* view, const int64_t* group_row_start_host, int n_groups, int n_cols,
                      int T_prime, unsigned long long* per_step, uint32_t* per_col, uint32_t* per_row, snn_stream_t stream);
int snn_planes_raster_nchw(const void* workspace, const snn_planes_view* view, int64_t row0, int N, int C, int H, int W, int T_prime,
                           uint8_t* out, snn_stream_t stream);
int snn_planes_raster_rows(const void* workspace, const snn_planes_view* view, int n_cols, int T_prime, uint8_t* out,
                           snn_stream_t stream);

/* ---- readout weight gradients: exact gradients of the two LI heads' weights from a pass's spike planes ----------------
 * The LI cell is linear and so is the bias-free 1x1 conv / linear in front of it, and the hidden spike train does not depend on the readout
 * weights.  With out = W S, S[r][k] = sum_{t < T'} kappa_t bit_t(r, k) and kappa = the impulse responses the forward folds the LI cell into
 * (li_kappa at T', in either li_order), the gradient of any loss with respect to the readout weights is
 *     gw_x[j][k] (+)= sum_r grad_x[r][j] * S[r][k]              x = a (cls_logits / cls_score), b (bbox_pred)
 * exactly: no surrogate gradient, no threshold, nothing that can flip.  Nothing else of training is here (hidden-layer gradients, losses).
 *   - `planes` / `view`: read exactly as the spike taps read them (the workspace of the pass, or a copy of its plane region with offset_bytes
 *     = 0); all three layouts are addressed inside the kernel; bits at or above n_cols are never read as spikes.  n_cols <= 32 * words
 *     (<= 8192), rows < 2^31;
 *   - T_prime in 1 .. view->steps_formed: T' = T is the gradient of the plain forward, T' < T that of the any-time readout at T';
 *   - grad_a [rows][NA], grad_b [rows][NB] fp32, rows in the order of the head's outputs; either (grad, gw) pair may be null with its count
 *     0; 1 <= NA + NB <= 480;
 *   - accumulate = 0 writes every element of gw_a [NA][n_cols] / gw_b [NB][n_cols] by work of this call (nothing is cleared in front: no
 *     memset node), accumulate = 1 adds to what they hold;
 *   - DETERMINISTIC: no floating-point atomics.  Slabs of rows write partial sums to `scratch` (snn_li_heads_wgrad_workspace_bytes: at
 *     most 512 x (NA + NB) x n_cols floats; monotone in every argument; 0 for a shape outside the limits), a second launch adds them in a
 *     fixed order: two calls on the same data are bit-equal, whatever the scratch held before.  The scratch must not overlap the planes;
 *   - rounding: S is summed in fp32 for t ascending, the products are fused multiply-adds over the rows; against exact arithmetic every
 *     element is within (rows + 2 T' + 4) 2^-24 sum_r |grad| S;
 *   - stream-only, no host synchronisation, hipGraph-capturable under the capture contract above; bad arguments (a null view / planes /
 *     parameters, an unknown layout, T' outside 1 .. steps_formed, n_cols > 32 * words, NA + NB = 0 or > 480, a null pointer of a head with
 *     outputs, a short or null scratch) return -1 with snn_last_error before any device work.  Two launches. */
size_t snn_li_heads_wgrad_workspace_bytes(int64_t rows, int n_cols, int NA, int NB);
int snn_li_heads_wgrad(const void* planes, const snn_planes_view* view, int n_cols, int T_prime, const snn_params* p_host,
                       const float* grad_a /* [rows][NA] */, const float* grad_b /* [rows][NB] */, int NA, int NB,
                       float* gw_a /* [NA][n_cols] */, float* gw_b /* [NB][n_cols] */, int accumulate, void* scratch,
                       size_t scratch_bytes, snn_stream_t stream);

/* ---- readout fine-tuning: target matching and the two head losses with their gradients -----------------------------
 * What lies between the head outputs and a scalar in the reference's training forward, for the readouts only: the gradients written here
 * are the `grad_a` / `grad_b` of snn_li_heads_wgrad.  All three calls are stream-only, synchronise nothing, are hipGraph-capturable under
 * the capture contract above (host tables are read at enqueue time and travel as kernel arguments), use no floating-point atomic and clear
 * nothing with a memset: every output element, and every scratch element a launch reads, is written by a launch of the same call, so two
 * calls on the same data are bit-equal whatever scratch and outputs held before.  Bad arguments return -1, a shape beyond a limit -4, both
 * before any device work and with snn_last_error set; each size query is monotone in every argument and 0 outside the limits.
 *
 * snn_match_targets: IoU matching (torchvision's Matcher), labels and BoxCoder.encode for N <= 64 images in one call.
 *   - boxes [sum B_n][4] (anchors or proposals, x1 y1 x2 y2) with the HOST table box_start[N + 1]; gt_boxes [sum G_n][4] and gt_labels
 *     [sum G_n] int64 (null: RPN mode) with the HOST table gt_start[N + 1]; both tables start at 0; G_n <= 256 (else -4), fewer than 2^31
 *     boxes; weights: HOST float[4], the coder's (wx, wy, ww, wh); boxes, gt_boxes and reg_target 16-byte aligned;
 *   - per box: matched_idx int32 = the index of the image's ground-truth box with the largest IoU (the lowest index on a tie), -1 where
 *     that IoU < low, -2 where low <= IoU < high (both compared in fp32); with allow_low_quality every box whose IoU with some ground-truth
 *     box equals that box's maximum over the image's boxes gets its own arg-max back (a ground-truth box that overlaps nothing has maximum 0
 *     and restores every box with IoU 0 to it: the published behaviour); label int32 = 1 / 0 / -1 in RPN mode, gt_labels[idx] / 0 / -1
 *     otherwise; reg_target [4] = encode(gt[max(idx, 0)], box).  An image with G_n = 0: matched_idx 0, label 0, the encoding of the zero box
 *     (-inf in the two log terms);
 *   - the IoU is formed in fp32 in the operation order of torchvision's box_iou with IEEE division: every decision equals the one torch takes
 *     on the same fp32 boxes.  Precondition: finite coordinates, x2 >= x1 and y2 >= y1, ground-truth boxes with positive area (an IoU of 0 / 0
 *     is NaN in torch and never a maximum here);
 *   - scratch (snn_match_targets_workspace_bytes(sum B_n, N)) is used with allow_low_quality only: three launches, else one.
 *
 * snn_rpn_loss_grad: the RPN's compute_loss and its gradient with respect to the head outputs.
 *   - logits [P][A], deltas [P][4A]: the head's own outputs (rows level-major, then image, y, x; `levels`: N, H, W of each level, feat
 *     unused); label int32, sampled uint8 and reg_target [4] per anchor in the reference's order (image, level, y, x, a) - what
 *     snn_match_targets writes for boxes = the images' anchors; the kernel maps between the two orders;
 *   - n = the number of sampled anchors, counted on the device; loss[0] = mean over the sampled anchors of max(x, 0) - x y + log1p(exp(-|x|)),
 *     y = label; loss[1] = the smooth-L1 sum (beta 1/9) over the four coordinates of the sampled anchors with label 1, divided by n;
 *     g_logits [P][A] = (sigmoid(x) - y) / n, g_deltas [P][4A] = (d / beta inside |d| < beta, sign(d) outside) / n, zero where the loss does
 *     not read; n = 0: NaN losses (torch's) and zero gradients;
 *   - at most 8 levels, A <= 64, fewer than 2^31 anchors (-4); deltas, reg_target, g_deltas 16-byte aligned; three launches.
 *
 * snn_det_loss_grad: fastrcnn_loss and its gradient.
 *   - logits [R][K], box [R][K4], label [R] int32, reg_target [R][4]; K4 must be 4 K (-1: the loss indexes one box per class); 2 <= K <= 256
 *     (-4 above); rows with label -1 (or a label that is no class) are left out of both terms and get zero gradients: n = the rows with
 *     label >= 0; with no such row left out the result is the reference's;
 *   - loss[0] = mean softmax cross-entropy (maximum subtracted), loss[1] = smooth L1 (beta 1/9, sum) on the four outputs of the row's own
 *     class for labels > 0, divided by n; g_logits = (softmax - onehot) / n, g_box zero but for those four outputs; three launches.
 *
 * Rounding: per-term arithmetic is fp32 (expf, logf, log1pf of the device library), the sums of the losses and the softmax denominators
 * are carried in fp64 and rounded once: against the same formulas in exact arithmetic on the same fp32 inputs a loss is within 10 x 2^-24
 * of its value, a gradient element within 8 x 2^-24 / n, a regression target within 8 x 2^-24 of its magnitude plus the conditioning of
 * the centre difference. */
size_t snn_match_targets_workspace_bytes(int64_t total_boxes, int N);
int snn_match_targets(const float* boxes, const int64_t* box_start_host, const float* gt_boxes, const int64_t* gt_labels,
                      const int64_t* gt_start_host, int N, float high, float low, int allow_low_quality, const float* weights_host,
                      int32_t* matched_idx, int32_t* label, float* reg_target, void* scratch, size_t scratch_bytes, snn_stream_t stream);
size_t snn_rpn_loss_grad_workspace_bytes(int64_t anchors /* P x A */);
int snn_rpn_loss_grad(const snn_rpn_level* levels, int n_levels, int A, int N, const float* logits, const float* deltas,
                      const int32_t* label, const uint8_t* sampled, const float* reg_target, float* loss /* [2] */, float* g_logits,
                      float* g_deltas, void* scratch, size_t scratch_bytes, snn_stream_t stream);
size_t snn_det_loss_grad_workspace_bytes(int R, int K);
int snn_det_loss_grad(const float* logits, const float* box, const int32_t* label, const float* reg_target, int R, int K, int K4,
                      float* loss /* [2] */, float* g_logits, float* g_box, void* scratch, size_t scratch_bytes, snn_stream_t stream);

/* ---- hidden-layer gradients: SuperSpike through lif7 into fc7 ---------------------------------------------------------
 * The reference's hidden cells are Norse LIFCells with the default method "super": Heaviside forward, grad / (alpha |x| + 1)^2 backward,
 * x = vd - v_th.  With a = dt_tau_mem, b = neg_dt_tau_syn, th = v_th_lif, one neuron of lif_feed_forward_step is
 *     vd_t = v_{t-1} + a ((v_leak - v_{t-1}) + i_{t-1})     z_t = H(vd_t - th)     v_t = (1 - z_t) vd_t + z_t v_reset     i_t = (i_{t-1} + b i_{t-1}) + cur_t
 * from v_{-1} = v_leak, i_{-1} = 0.  cur_t first moves a spike at step t + 1, so a pass of T steps has Tc = T - 1 currents that matter.  The
 * adjoint, with gz_t = dL/dz_t and (G_v, G_i) the gradient of the state after step t (zero after step T - 1; the reset is differentiated
 * through z, as Norse's autograd does):
 *     for t = T - 1 .. 0:   d_cur_t = G_i (t <= T - 2);   s = 1 / (alpha |vd_t - th| + 1)^2;   dz = gz_t + G_v (v_reset - vd_t);
 *                           dvd = G_v (1 - z_t) + dz s;   G_i = dvd a + G_i (1 + b);   G_v = dvd (1 - a)
 * and dL/dW[n][k] = sum_{t < Tc} sum_r d_cur_t[r][n] spk_in_t[r][k] for the bias-free linear layer in front.  TEACHER FORCING: z_t is the bit
 * the forward pass saved, never a fresh comparison - a recomputed current may differ from the fused kernel's in its last bit, which moves
 * vd_t by an ulp under a surrogate that is continuous in |x|, and flips nothing.
 * All four entries: stream-only, no host synchronisation, no allocation, hipGraph-capturable under the capture contract above, no
 * floating-point atomics, nothing cleared by a memset - every output and scratch element that is read is written by a launch of the same
 * call, so two calls on the same data are bit-equal whatever outputs and scratch held before.  Bad arguments return -1 with snn_last_error
 * before any device work; the size query is monotone in every argument and 0 outside the limits.
 *
 * snn_planes_to_rows: the first T' (1 .. view->steps_formed) steps of a plane set in any of the three layouts -> out [T'][rows][words] in
 *   SNN_PLANES_ROWS order, bit for bit (padding bits included).  The "save" of a pass's planes (the next pass overwrites the workspace) and
 *   the [M][Kw] operand of snn_spike_gemm / snn_spike_gemm_bf16x3.  `out` must not overlap the planes.  One launch.
 *
 * snn_lif_surrogate_bwd: the adjoint above, one thread per (row, column); d_cur [Tc][R][N] = dL/dcur.
 *   - cur [Tc][R][ldc] (ldc >= N: the un-fused GEMMs' output), z_rows [Tc + 1][R][ceil(N / 32)]: the layer's OWN spikes of all T = Tc + 1
 *     steps, rows layout; bits at or above N are never read;
 *   - the upstream gradient is gz_t + kappa_t gu: gz [Tc + 1][R][N] and gu [R][N] are each nullable (both null: -1); kappa = the impulse
 *     responses of snn_li_heads_wgrad at T = Tc + 1 in p_host->li_order, formed on the host - gu = g_cls W_cls + g_box W_box is then the
 *     whole readout's pull on lif7's spikes;
 *   - alpha finite and >= 0 (0: the straight-through estimator); 1 <= Tc <= SNN_MAX_STEPS - 1, N <= 8192; d_cur must not overlap cur;
 *   - arithmetic: fp32, in the operation order written above (the build does not contract), IEEE division; no scratch memory, no register
 *     array: the forward sweep parks vd_{t+1} in d_cur[t], the reverse sweep writes d_cur[t] after step t + 1 has consumed that slot.
 *     Memory-bound, about 4 Tc R N 4 bytes.  One launch.
 *
 * snn_spike_linear_wgrad: gw[n][k] (+)= sum_{t < T'} sum_r d_cur[t][r][n] * bit_t(r, k), the weight gradient of a linear layer fed by spikes.
 *   - a_rows [T'][rows][ceil(K / 32)] (rows layout: snn_planes_to_rows), d_cur [T'][rows][ldd], N <= ldd < 2^28; K <= 8192, N <= 8192, rows < 2^31,
 *     T' <= SNN_MAX_STEPS; rows past `rows`, columns past N and bits past K contribute nothing and no word past a row's last word is loaded;
 *   - runs on v_mfma_f32_32x32x2_f32 with both operands taken straight from global memory (no LDS): the spike operand is 0.0 / 1.0, every
 *     product is exact, a result is an fp32 fused-multiply-add chain over the rows of a slab;
 *   - DETERMINISTIC: the T' x rows reduction rows are split into at most 16 slabs (a function of T' x rows alone), partial tiles go to
 *     `scratch` (snn_spike_linear_wgrad_workspace_bytes = slabs x N x K floats), a second launch adds them in ascending order and writes every
 *     element of gw [N][K] (accumulate = 0) or adds to it (accumulate = 1);
 *   - rounding: against exact arithmetic every element is within (T' rows + slabs + 2) 2^-24 sum_{t, r} |d_cur[t][r][n]| bit_t(r, k).
 *   Two launches. */
int snn_planes_to_rows(const void* workspace, const snn_planes_view* view, int T_prime, uint32_t* out /* [T'][rows][words] */,
                       snn_stream_t stream);
int snn_lif_surrogate_bwd(const float* cur /* [Tc][R][ldc] */, int ldc, const uint32_t* z_rows /* [Tc+1][R][ceil(N/32)] */, int Tc, int R,
                          int N, const snn_params* p_host, float alpha, const float* gz /* [Tc+1][R][N], nullable */,
                          const float* gu /* [R][N], nullable */, float* d_cur /* [Tc][R][N] */, snn_stream_t stream);
size_t snn_spike_linear_wgrad_workspace_bytes(int64_t rows, int K, int N, int T_prime);
int snn_spike_linear_wgrad(const uint32_t* a_rows /* [T'][rows][ceil(K/32)] */, const float* d_cur /* [T'][rows][ldd] */, int ldd,
                           int T_prime, int64_t rows, int K, int N, float* gw /* [N][K] */, int accumulate, void* scratch,
                           size_t scratch_bytes, snn_stream_t stream);

/* ---- fc6's gradient: the spike-fed weight gradient on the bf16 matrix cores --------------------------------------------
 * One layer below the section above: lif6's upstream gradient is gz6_t = d_cur7_t W7 (t <= T - 2, no gu term), lif6 receives cur6_t =
 * W6 enc_t of which only steps 0 .. T - 3 matter (Tc = T - 2: the window the forward forms, see the spike taps), and
 *     dL/dW6[n][k] = sum_{t <= T - 3} sum_r d_cur6_t[r][n] enc_t(r, k)        k = channel * 49 + bin, fc6.weight's own layout.
 * snn_lif_surrogate_bwd (gz given, gu null), snn_planes_to_rows, the un-fused spike GEMMs and the stand-alone encoders serve it as they are;
 * what fc6's shape (K = 49 C = 12544, N = 1024, M = (T - 2) R = 10240) needs is a weight gradient that takes K > 8192, a scratch that does
 * not grow with slabs the grid does not need, and the bf16 matrix cores:
 *
 * snn_spike_wgrad_bf16x3: gw[n][k] (+)= sum_{t < T'} sum_r d_cur[t][r][n] * bit_t(r, k), the argument list of snn_spike_linear_wgrad.
 *   - 1 <= K <= 16384 (49 C up to C = 320), 1 <= N <= 8192, rows < 2^31, T' <= SNN_MAX_STEPS, N <= ldd < 2^28; K need not be a multiple of
 *     32; rows past `rows`, columns past N and bits past K contribute nothing, no word past a row's last word is loaded and no byte outside
 *     gw [N][K] is written;
 *   - every d_cur element is split on the fly, once per work-group, into three bf16 values hi = rn(x), mid = rn(x - hi), lo = rn(x - hi - mid)
 *     - exact for every fp32 of magnitude below 2^128 - 2^119 (above it hi rounds up to bf16 infinity) whose lowest set bit is >= 2^-133
 *     (k_bf16x3_split_check describes the same split) - the spike operand is
 *     0.0 / 1.0 in bf16, every product is exact, a result is an fp32 accumulation of exact products inside v_mfma_f32_32x32x16_bf16; the planes
 *     reach an accumulator in the order lo, mid, hi, so a column with a single spike returns d_cur bit for bit (-0 may return +0);
 *   - PRECONDITION: d_cur is finite and of magnitude below 2^128 - 2^119 = 0x7F7F8000 (bf16's largest value plus half its last place).  An
 *     element at or above it, infinite or NaN makes its whole output row non-finite (as 0 x inf does in the fp32 kernel);
 *   - DETERMINISTIC: the T' x rows reduction rows are split into slabs, a pure function of (M = T' rows, K, N): with tiles = ceil(N / 128)
 *     ceil(K / 256), want = 1 if tiles >= 256, else min(ceil(256 / tiles), ceil(M / 256), 32); a slab holds ceil(ceil(M / want) / 32) 32 rows.
 *     One slab (the output tiles alone fill the 256 CUs): the kernel writes (accumulate = 0) or adds to (1) every element of gw itself.
 *     Several: partial tiles go to `scratch`, a second launch adds them in ascending order and writes or adds to every element of gw;
 *   - snn_spike_wgrad_bf16x3_workspace_bytes = 4 min(min(ceil(M / 256), 32) N K, 256 x 128 x 256 + N K): never below slabs N K floats,
 *     monotone in every argument (the slab count itself falls as the tiles grow), 0 outside the limits, non-zero inside; at fc6's shape
 *     (rows 1024, T' 10, K 12544, N 1024) it is 85 MB, below 2 N K floats.  The entry asks for the queried size whatever the plan: with ONE
 *     slab (fc6's shape) no byte of scratch is read or written - what monotonicity costs;
 *   - snn_spike_wgrad_bf16x3_slabs: that plan's slab count and, through `slab_rows`, the rows of every slab but the last; host only, 0 outside
 *     the limits;
 *   - rounding: against exact arithmetic every element is within (3 T' rows + slabs + 4) 2^-24 sum_{t, r} |d_cur[t][r][n]| bit_t(r, k)
 *     + T' rows 2^-133: the three planes' terms, each |part| <= |d|, under the standard model, and what lies below the finest bf16 subnormal.
 *   One or two launches; the contract of the section above (stream-only, capturable, no floating-point atomics, no memset, bit-equal
 *   repeats, -1 with snn_last_error before any device work). */
size_t snn_spike_wgrad_bf16x3_workspace_bytes(int64_t rows, int K, int N, int T_prime);
int snn_spike_wgrad_bf16x3_slabs(int64_t rows, int K, int N, int T_prime, int64_t* slab_rows /* nullable */);
int snn_spike_wgrad_bf16x3(const uint32_t* a_rows /* [T'][rows][ceil(K/32)] */, const float* d_cur /* [T'][rows][ldd] */, int ldd,
                           int T_prime, int64_t rows, int K, int N, float* gw /* [N][K] */, int accumulate, void* scratch,
                           size_t scratch_bytes, snn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SNN_HIP_H */
