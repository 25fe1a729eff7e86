// gfx950 (MI355X, CDNA4) kernels of the spiking RPN / detector heads + their C ABI (include/snn_hip.h).
//
// Data flow (bit-planes everywhere a spike tensor would be; see include/snn_hip.h):
//   RPN  : k_encode_nchw -> k_conv3x3_lif (fp32-MFMA implicit GEMM, T-loop inside, LIF state in
//          registers, ballot -> spike planes) -> k_li_heads (both 1x1 LI heads, time-collapsed)
//   DET  : k_encode_rows -> k_spike_gemm (time-batched fc6) -> k_lif_scan -> k_spike_gemm (fc7)
//          -> k_lif_scan -> k_li_heads
// Reference loops replaced: rpn.py:84-121 (+126-200), faster_rcnn.py:470-516 (+520-618).
#include "snn_common.h"
#include "snn_hip.h"
#include "snn_hip_debug.h"

// Timing-only switches of the A/B harness (tools/ab_build.sh, tools/ab_mx.sh: what does a staging step / barrier cost) give
// WRONG results by construction.  A build that defines one must say so with -DSNN_EXPERIMENTS; the product build
// (snn_automotive_object_detection_amd/build.py) never does, and tests/test_code_object.py checks that this guard fires.
#if !defined(SNN_EXPERIMENTS) && (defined(SNN_EXP_NO_FETCH) || defined(SNN_EXP_NO_GLDS) || defined(SNN_EXP_NO_BARRIER) || \
    defined(SNN_EXP_CLOCK) || defined(SNN_EXP_TIMELINE) || defined(SNN_EXP_SP_NO_A) || defined(SNN_EXP_SP_NO_B) || defined(SNN_EXP_SP_NO_AREAD) || defined(SNN_EXP_SP_NO_BREAD) || defined(SNN_EXP_SP_NO_MFMA) || defined(SNN_EXP_SP_NO_BAR) || defined(SNN_EXP_ONE_WG_PER_CU) || defined(SNN_EXP_MX_NOSTAGE) || defined(SNN_EXP_MX_NOREADB) || defined(SNN_EXP_MX_NOBAR) || \
    defined(SNN_EXP_MX_NOA) || defined(SNN_EXP_MX_BAR2) || defined(SNN_EXP_MX_RDW_G) || defined(SNN_EXP_ENCP_NOLOAD) || defined(SNN_EXP_ENCP_NOENC) || defined(SNN_EXP_ENCP_NOSTORE) || \
    defined(SNN_EXP_PP_NOWAIT) || defined(SNN_EXP_PP_NOCOPY) || defined(SNN_EXP_PP_NOBAR) || defined(SNN_EXP_PP_NOMFMA) || defined(SNN_EXP_PP_NOEPI) || defined(SNN_EXP_PP_NOY) || defined(SNN_EXP_PP_ALLDENSE) || defined(SNN_EXP_PP_ALLSPARSE) || defined(SNN_EXP_PP_NOBREAD) || defined(SNN_EXP_SP_NO_SEC))
#error "SNN_EXP_* switches are timing experiments with wrong results: add -DSNN_EXPERIMENTS (never in a product build)"
#endif

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// ------------------------------------------------------------------------------------------------
// error plumbing (thread-local; no exceptions, no abort)
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static thread_local int g_last_fc_sparse = 0;      // ... the detector's fc6 + LIF
static thread_local unsigned long long g_last_rpn_planes[3] = {0, 0, 0};      // workspace offset of the shared LIF's spike planes, blocks of four words?, positions
static thread_local unsigned long long g_last_det_planes[3] = {0, 0, 0};      // workspace offsets of lif6's / lif7's spike planes, lif6 word-major?
static thread_local int g_last_enc_mode = -1;      // ENC_* form of this thread's last encoder launch (snn_debug_last_enc_mode); -1: none yet
static thread_local int g_last_conv_sparse = 0;    // did this thread's last RPN conv + LIF enqueue the sparse launch pair (snn_debug_last_conv_path)

static int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int check_launch(const char* name) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-3, "launch of %s failed: %s", name, hipGetErrorString(e));
    return 0;
}
#define SNN_CHECK_LAUNCH(name)                 \
    do {                                       \
        const int rc_ = check_launch(name);    \
        if (rc_) return rc_;                   \
    } while (0)

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// SNN_PRECISION_F32_STRICT = the fp32 family with the LI heads on the fp32 VALU kernel as well: no weight is ever split into bf16 planes
// SNN_PRECISION_BF16 = the bf16x3 family - same encoders, planes, launch plans, LI heads - on ONE weight plane (the packers rounded every weight to
// the nearest bf16): its contractions run the single-plane kernels k_gemm_lif_sparse1 / k_gemm_bf16
static inline int prec_family(int precision) {
    return precision == SNN_PRECISION_F32_STRICT ? SNN_PRECISION_F32 : precision == SNN_PRECISION_BF16 ? SNN_PRECISION_BF16X3 : precision;
}
static inline int prec_family(const snn_params* p) { return prec_family(p->precision); }
// weight planes of a bf16 matrix-core launch: 3, or 1 inside a head pass at SNN_PRECISION_BF16 (the stage-level entry points always run three)
static inline int weight_planes(const snn_params* p) { return p->precision == SNN_PRECISION_BF16 ? 1 : 3; }

// route of a head pass's sparse-capable layer - the RPN's conv (snn_rpn_head_forward_routed) or the detector's fc6
// (snn_det_head_forward_routed / _roialign_routed, 4.10); every other entry and the stage-level ones: SPARSE_ROUTE = the plain plan.
// dense: the sparse plan is not taken (as SNN_SPARSE=0, for this call); gated (decided by the pass's plan for an AUTO call whose plan is the
// sparse one): the layer enqueues compress + count, the decision, and BOTH launches behind the gate word stat[2]
struct SparseRoute { int route; float crossover; int32_t* stat; bool gated; };
static const SparseRoute SPARSE_ROUTE = {SNN_ROUTE_SPARSE, 0.0f, nullptr, false};
static bool route_known(int route) { return route == SNN_ROUTE_SPARSE || route == SNN_ROUTE_DENSE || route == SNN_ROUTE_AUTO; }
// what a routed entry hands its pass: the caller's route - in spike-rate mode the plain plan on every route (route_stat is still written)
static SparseRoute routed(int route, float crossover, int32_t* route_stat, bool spike_rates) {
    return SparseRoute{spike_rates ? (int)SNN_ROUTE_SPARSE : route, crossover, route_stat, false};
}
// the checks the three routed entries share, before anything is asked of the plan or enqueued.  need: the routed size query's answer for
// the call's shape; 0 where the shape is none it knows - the pass's own message follows
static int route_check(const char* who, int route, float crossover, const int32_t* route_stat, size_t ws_bytes, size_t need) {
    if (!route_known(route)) return fail(-1, "%s: unknown route %d", who, route);
    if (route == SNN_ROUTE_AUTO && !route_stat) return fail(-1, "%s: SNN_ROUTE_AUTO needs route_stat", who);
    if (route == SNN_ROUTE_AUTO && crossover != crossover) return fail(-1, "%s: crossover is not a number", who);
    if (ws_bytes < need) return fail(-1, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return 0;
}

static NeuronP make_p(const snn_params* p, float v_th) {
    NeuronP q;
    q.ca = p->dt_tau_mem; q.cb = p->neg_dt_tau_syn; q.v_leak = p->v_leak; q.v_reset = p->v_reset;
    q.v_th = v_th;
    q.v_fire = 0.0f;
    return q;
}

// ------------------------------------------------------------------------------------------------
// weight packing: GEMM operand B[k][n] -> fragment-major
//   packed[((kc*Nw + nt)*4 + qq)*64 + lane][r] = B[k = kc*32 + 4*qq + r + 16*(lane>>5)][n = nt*32 + (lane&31)]
// so that one ds_read_b128 per lane yields the B operands of 4 consecutive MFMAs and both the
// global->LDS copy and the LDS read are perfectly linear (no bank conflicts, no swizzle needed).
// ------------------------------------------------------------------------------------------------
enum { PACK_CONV3X3 = 0, PACK_LINEAR = 1, PACK_LINEAR_PERM = 2 };

__global__ void k_pack_gemm_b(const float* __restrict__ src, float* __restrict__ dst, int mode,
                              int K, int N, int Kc, int Nw, int Cin, int Cp) {
    const size_t total = (size_t)Kc * Nw * 1024;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        const int r = idx & 3;
        const int lane = (idx >> 2) & 63;
        const int qq = (idx >> 8) & 3;
        const size_t blk = idx >> 10;
        const int nt = (int)(blk % Nw);
        const int kc = (int)(blk / Nw);
        const int k = kc * 32 + 4 * qq + r + 16 * (lane >> 5);
        const int n = nt * 32 + (lane & 31);
        float v = 0.0f;
        if (n < N) {
            if (mode == PACK_CONV3X3) {            // k = tap*Cp + ci ; src OIHW [N][Cin][3][3]
                const int tap = k / Cp, ci = k % Cp;
                if (ci < Cin) v = src[((size_t)n * Cin + ci) * 9 + tap];
            } else {                               // src [N][K] (nn.Linear weight)
                if (k < K) v = src[(size_t)n * K + k];
            }
        }
        dst[idx] = v;
    }
}

// both LI heads -> transposed [Kp][NOp] (NOp = NA+NB rounded up to 16)
__global__ void k_pack_heads(const float* __restrict__ wa, int NA, const float* __restrict__ wb, int NB,
                             int K, int Kp, int NOp, float* __restrict__ dst) {
    const int total = Kp * NOp;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int k = idx / NOp, j = idx % NOp;
        float v = 0.0f;
        if (k < K) {
            if (j < NA) v = wa[(size_t)j * K + k];
            else if (j < NA + NB) v = wb[(size_t)(j - NA) * K + k];
        }
        dst[idx] = v;
    }
}

#include "snn_encode.h"
#include "snn_f32.h"
#include "snn_bf16x3.h"
#include "snn_sparse.h"
#ifdef SNN_PINGPONG                                 // (round 6: measured 14 % SLOWER than the FAT conv - profiles/r6_pingpong.txt; A/B builds only, tools/ab_build.sh)
#include "snn_sparse_pp.h"
#endif
#include "snn_heads.h"
#include "snn_post.h"

#include "snn_mx.h"

#include "snn_affine.h"
#include "snn_taps.h"
#include "snn_wgrad.h"
#include "snn_loss.h"
#include "snn_hidden.h"
#include "snn_spike_wgrad_x3.h"

// ================================================================================================
// C ABI
// ================================================================================================
// Debug / A-B knobs.  They are read from the environment ONCE (first call into the library, thread-safe static
// initialisation) and frozen: later setenv() calls change nothing, calls from several threads see one consistent set.
// snn_debug_reload_knobs() re-reads them (the parity tests compare kernel variants in one process; not for concurrent use).
#define SNN_SPARSE_FAT_CONV_DEFAULT 3
#ifndef SNN_CONV_PP_DEFAULT
#define SNN_CONV_PP_DEFAULT 0
#endif
struct Knobs {
    bool enc_generic;        // SNN_ENC_GENERIC=1     op-for-op encoder kernels even for zero rest / reset potentials
    bool enc_rows_ballot;    // SNN_ENC_ROWS=ballot   element-per-lane row encoder
    int bf16x3_mt;           // SNN_BF16X3_MT=2|3|4   M-tiles per wave (0: cost model)
    int bf16x3_short;        // SNN_BF16X3_SHORT=0|1  T-in-tile launches: no / half of the row-waves one M-tile short (-1 = by cost)
    int bf16x3_wn;           // SNN_BF16X3_WN=1|2     waves along N of the tile (0 = default = 1: the 512 x 64 tile; 2 = 256 x 128, the conv's shape until round 3)
    bool bf16x3_lif_reg;     // SNN_BF16X3_LIF=reg    register-resident conv + LIF fusion instead of T-in-tile
    int mx_mw;               // SNN_MX_MW=4|8         rows per wave of k_gemm_mx
    int li_heads;            // SNN_LI_HEADS=valu|mfma|ksplit -> 1 | 2 | 3 (0: by shape)
    bool debug_occ;          // SNN_DEBUG_OCC         print occupancy of the big kernels
    bool spk_rows;           // SNN_SPK_SPLIT=0       the RPN conv writes plain row-major spike planes (A/B; default: blocks of four words
                             //                       where the LI heads kernel reads them that way)
    bool bf16x3_xcd;         // SNN_BF16X3_XCD=0      plain block order instead of the XCD-aware one (A/B)
    bool stage_wm;           // SNN_STAGE_PLANES=wm   A/B harness only: snn_conv3x3_lif_bf16x3 / snn_spike_gemm_lif_bf16x3 take their
                             //                       INPUT planes word-major ([T][word][row]; tools/ab_conv.py)
    bool enc_quant;          // SNN_ENC_QUANT=0       period planes by the encoder's recurrence instead of its threshold table (A/B, tests)
    bool periods;            // SNN_PERIOD_PLANES=0   the whole heads multiply the encoder's spike planes z_t instead of its period planes e_n
                             //                       (snn_common.h; default: period planes on the bf16x3 tile path with zero rest / reset potentials)
    bool stage_periods;      // SNN_STAGE_PERIODS=1   tests / tools: the STAGE-level encoders emit period planes and the stage-level fused launches
                             //                       (snn_conv3x3_lif_bf16x3, snn_spike_gemm_lif_bf16x3) take their input planes as such
    int roi_e, roi_rw;       // SNN_ROI_E / SNN_ROI_RW  table-driven RoIAlign kernel: element groups per work-group / RoIs per wave (0 = default 2 / 4)
    bool epi_general;        // SNN_EPI_GENERAL=1     T-in-tile LIF epilogue: the general (guarded) form instead of the straight-line instance of this T (tests)
    bool roi_tab;            // SNN_ROI_TAB=0         fused RoIAlign + encoder: the per-element kernel instead of the table-driven one (A/B, tests)
    bool dead_keep;          // SNN_DEAD_STEPS=keep   form the input currents of ALL time steps (A/B + test switch: the default
                             //                       skips the steps whose currents cannot reach an output, lif_windows)
    bool sparse;             // SNN_SPARSE=0          RPN conv: every period plane on the dense matrix-core instruction (default: planes e_3.. on the
                             //                       structured-sparse one, snn_sparse.h)
    int encp_nw;             // SNN_ENCP_NW=4|8       waves per block of k_encode_rows_perm (A/B; default: 8 where two blocks fit a CU, else 4)
    int encp_rb;             // SNN_ENCP_RB=8|16      RoIs per block of k_encode_rows_perm (A/B; default: 16 where the window fits one pass through LDS)
    int sparse_fat_conv;     // SNN_SPARSE_FAT_CONV=0..3 the FAT conv (four waves, LIF in registers; bit-identical to the 8-wave shape): bit 0 = T = 7 .. 9 (4 x 1 waves, tiles of
                             //                       64 positions), bit 1 = T = 12 .. 16 (2 x 2 waves, tiles of 32); default: both
    bool lif_regs;           // SNN_LIF_REGS=0        FAT shapes: the LIF through the LDS tile image instead of in registers (linear layers; the FAT conv has no other form)
    bool conv_pp;            // SNN_CONV_PP=0|1       -DSNN_PINGPONG builds only (tools/ab_build.sh): RPN conv at T = 7, 8 in the ping-pong form of the FAT conv (snn_sparse_pp.h:
                             //                       one persistent work-group of 8 waves per CU, the two waves of a SIMD alternate matrix / memory phases; bit-identical spike
                             //                       planes, measured 14 % slower: profiles/r6_pingpong.txt)
    bool enc_fold;           // SNN_ENC_FOLD=0        RPN head: k_compress_planes as its own launch again instead of inside the encoder launch (bit-identical planes)
    bool sparse_fat;         // SNN_SPARSE_FAT=0      linear layers (fc6) on the 8-wave shape of k_gemm_lif_sparse instead of the FAT one (four waves of up to 256
                             //                       registers, twice the M-tile slots per wave: the default where its loop instances exist; bit-identical)
    int planes;              // SNN_PLANES=rm|wm      internal spike planes of the bf16x3 heads: all row-major [T][row][word] / all
                             //                       word-major [T][word][row] (1 / 2; 0 = default = word-major since round 3;
                             //                       bit-identical results either way, A/B + test switch)
};
static Knobs load_knobs() {
    Knobs k;
    const char* e;
    k.enc_generic = (e = getenv("SNN_ENC_GENERIC")) && e[0] == '1';
    k.enc_rows_ballot = (e = getenv("SNN_ENC_ROWS")) && !strcmp(e, "ballot");
    k.bf16x3_mt = (e = getenv("SNN_BF16X3_MT")) ? atoi(e) : 0;
    e = getenv("SNN_BF16X3_SHORT");
    k.bf16x3_short = (e && e[0] == '1') ? 1 : (e && e[0] == '0') ? 0 : -1;
    e = getenv("SNN_BF16X3_WN");
    k.bf16x3_wn = (e && e[0] == '2') ? 2 : (e && e[0] == '1') ? 1 : 0;
    k.bf16x3_lif_reg = (e = getenv("SNN_BF16X3_LIF")) && !strcmp(e, "reg");
    e = getenv("SNN_MX_MW");
    k.mx_mw = (e && e[0] == '8') ? 8 : ((e && e[0] == '4') ? 4 : 0);
    e = getenv("SNN_LI_HEADS");
    k.li_heads = !e ? 0 : !strcmp(e, "valu") ? 1 : !strcmp(e, "mfma") ? 2 : !strcmp(e, "ksplit") ? 3 : 4;
    k.debug_occ = getenv("SNN_DEBUG_OCC") != nullptr;
    k.sparse_fat = !((e = getenv("SNN_SPARSE_FAT")) && e[0] == '0');
    k.enc_fold = !((e = getenv("SNN_ENC_FOLD")) && e[0] == '0');
    k.conv_pp = (e = getenv("SNN_CONV_PP")) ? e[0] == '1' : SNN_CONV_PP_DEFAULT != 0;
    k.lif_regs = !((e = getenv("SNN_LIF_REGS")) && e[0] == '0');
    k.sparse_fat_conv = (e = getenv("SNN_SPARSE_FAT_CONV")) ? atoi(e) : SNN_SPARSE_FAT_CONV_DEFAULT;
    k.encp_rb = (e = getenv("SNN_ENCP_RB")) ? atoi(e) : 0;
    k.encp_nw = (e = getenv("SNN_ENCP_NW")) ? atoi(e) : 0;
    e = getenv("SNN_PLANES");
    k.planes = !e ? 0 : !strcmp(e, "rm") ? 1 : !strcmp(e, "wm") ? 2 : 0;
    k.bf16x3_xcd = !((e = getenv("SNN_BF16X3_XCD")) && e[0] == '0');
    k.spk_rows = (e = getenv("SNN_SPK_SPLIT")) && e[0] == '0';
    k.stage_wm = (e = getenv("SNN_STAGE_PLANES")) && !strcmp(e, "wm");
    k.dead_keep = (e = getenv("SNN_DEAD_STEPS")) && !strcmp(e, "keep");
    k.periods = !((e = getenv("SNN_PERIOD_PLANES")) && e[0] == '0');
    k.enc_quant = !((e = getenv("SNN_ENC_QUANT")) && e[0] == '0');
    k.stage_periods = (e = getenv("SNN_STAGE_PERIODS")) && e[0] == '1';
    k.epi_general = (e = getenv("SNN_EPI_GENERAL")) && e[0] == '1';
    k.roi_tab = !((e = getenv("SNN_ROI_TAB")) && e[0] == '0');
    k.sparse = !((e = getenv("SNN_SPARSE")) && e[0] == '0');
    k.roi_e = (e = getenv("SNN_ROI_E")) ? atoi(e) : 0;
    k.roi_rw = (e = getenv("SNN_ROI_RW")) ? atoi(e) : 0;
    if (k.roi_e < 0 || k.roi_e > 16) k.roi_e = 0;
    if (k.roi_rw < 0 || k.roi_rw > 8) k.roi_rw = 0;
    return k;
}
static Knobs& knobs() {
    static Knobs k = load_knobs();
    return k;
}

// encoder fast path: Norse's default rest / reset potentials
static bool enc_zero_rest(const NeuronP& p) { return p.v_leak == 0.0f && p.v_reset == 0.0f && !knobs().enc_generic; }

// ---- the period-plane encoder as a quantiser (snn_common.h: THRESHOLD FORM) ----------------------------------------------
// first spike of the zero-rest encoder at or before step k (0-based), with the device's exact fp32 operation sequence
// (enc_step_word<true> / enc_step with v_leak = 0; this translation unit is compiled with -ffp-contract=off)
static bool enc_fires_by(float x, int k, float ca, float v_th) {
    float v = 0.0f;
    for (int j = 0; j <= k; ++j) {
        const float d = x - v;
        const float m = ca * d;
        v = v + m;
        if (v > v_th) return true;
    }
    return false;
}
struct EncThTable { EncTh t; bool ok; float ca, v_th; };
// th[k] = the smallest float x with enc_fires_by(x, k): bisection over the bit patterns of the non-negative floats (the predicate is
// monotone up to rounding), then every float within ENC_TH_WINDOW ulps of the threshold is classified by the recurrence and must
// agree with the comparison x >= th[k] - beyond that distance the membrane is more than 1e-4 away from the threshold in relative
// terms, an order of magnitude above the rounding the recurrence can accumulate in 32 steps.  ok = false (any disagreement, a
// non-positive threshold, ca outside (0, 1)): the launchers keep the recurrence.  Per thread, recomputed when the parameters change.
#define ENC_TH_WINDOW 1024
static const EncThTable& enc_thresholds(float ca, float v_th) {
    // a model has two encoders (RPN head, detector head) whose parameters may differ: a few tables per thread, replaced round-robin
    constexpr int N_TAB = 4;
    static thread_local EncThTable tabs[N_TAB];
    static thread_local int n_tabs = 0, next_tab = 0;
    for (int j = 0; j < n_tabs; ++j)
        if (tabs[j].ca == ca && tabs[j].v_th == v_th) return tabs[j];
    EncThTable& tab = tabs[next_tab];
    next_tab = (next_tab + 1) % N_TAB;
    if (n_tabs < N_TAB) ++n_tabs;
    tab.ca = ca; tab.v_th = v_th; tab.ok = ca > 0.0f && ca < 1.0f && v_th > 0.0f;
    auto as_float = [](uint32_t b) { float f; memcpy(&f, &b, 4); return f; };
    for (int k = 0; k < SNN_MAX_STEPS && tab.ok; ++k) {
        uint32_t lo = 0u, hi = 0x7f800000u;                      // +0 never fires (v stays 0 < v_th), +inf fires at once
        if (!enc_fires_by(as_float(hi), k, ca, v_th) || enc_fires_by(0.0f, k, ca, v_th)) { tab.ok = false; break; }
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (enc_fires_by(as_float(mid), k, ca, v_th)) hi = mid; else lo = mid;
        }
        tab.t.th[k] = as_float(hi);
        const uint32_t b0 = hi > ENC_TH_WINDOW ? hi - ENC_TH_WINDOW : 1u, b1 = hi + ENC_TH_WINDOW < 0x7f800000u ? hi + ENC_TH_WINDOW : 0x7f800000u;
        for (uint32_t b = b0; b <= b1 && tab.ok; ++b)
            if (enc_fires_by(as_float(b), k, ca, v_th) != (b >= hi)) tab.ok = false;
        if (k > 0 && !(tab.t.th[k] <= tab.t.th[k - 1])) tab.ok = false;
    }
    return tab;
}
// encoder mode of a launch: ENC_QUANT for period planes whose threshold table verified, else the recurrence
static int enc_mode(const NeuronP& np, const EncTh** eth) {
    static const EncTh none = {{0}};
    *eth = &none;
    if (!enc_zero_rest(np)) return ENC_GENERIC;
    if (np.v_fire != 0.0f && knobs().enc_quant) {
        const EncThTable& t = enc_thresholds(np.ca, np.v_th);
        if (t.ok) { *eth = &t.t; return ENC_QUANT; }
    }
    return ENC_ZR;
}

// period planes (snn_common.h): the encoder's spike trains are exactly periodic when it starts from and resets to +0
static bool periods_possible(const snn_params* p) {
    return prec_family(p) == SNN_PRECISION_BF16X3 && p->v_leak == 0.0f && p->v_reset == 0.0f && !knobs().enc_generic && !knobs().bf16x3_lif_reg;
}

static int g3_slots() {                       // CUs: two co-resident work-groups share a CU's matrix pipe, so the tail is
                                              // quantised per CU, not per work-group slot (fc6: MT=4 1.03 ms, MT=3 1.07 ms)
    static int slots = 0;
    if (!slots) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        slots = cus;
    }
    return slots;
}

// ------------------------------------------------------------------------------------------------
// Dead time steps.  Norse's lif_feed_forward_step (rpn.py:106, faster_rcnn.py:499,501) updates the membrane from the OLD
// synaptic current and only then adds the step's input:  v_dec = v + ca*((v_leak - v) + i);  z = v_dec > v_th;  i = i_dec + x_t.
// So x_t first moves a spike at step t+1, and x_{T-1} moves nothing that leaves the layer: a LIF layer whose spikes
// z_0 .. z_last are consumed needs the currents of steps 0 .. last-1 only.  And a layer FED by a LIF layer sees z_0 = 0 at
// step 0 (v = v_leak, i = 0: v_dec = v_leak, no spike unless v_leak - v_th > 0), i.e. its current of step 0 is exactly +0.
// The kernels form currents for a window of steps and integrate +0 elsewhere - bit-identical spikes, counts and outputs
// (tests/test_gpu_dead_steps.py against SNN_DEAD_STEPS=keep, which forms all T).
//   RPN (rpn.py:98-119): shared LIF spikes of all T steps feed the LI heads -> conv currents of steps 0 .. T-2.
//   detector (faster_rcnn.py:492-516): lif7 spikes of all T steps feed the LI heads -> fc7 currents of steps 1 .. T-2
//   (z6_0 = 0); those read lif6 spikes 1 .. T-2 -> fc6 currents of steps 0 .. T-3 (0 .. T-2 in spike-rate mode, which
//   counts the lif6 spikes of every step, faster_rcnn.py:556).
// ------------------------------------------------------------------------------------------------
struct StepWindow { int t0, n; };                 // currents of steps t0 .. t0+n-1
static StepWindow lif_window_all(int T) { return StepWindow{0, T}; }
// the layer's spikes of every step are consumed (stage-level calls, the RPN conv, fc7 with z_in(0) != 0)
static StepWindow lif_window_full_out(int T) { return knobs().dead_keep ? lif_window_all(T) : StepWindow{0, T > 1 ? T - 1 : 1}; }
static bool lif_first_spike_is_zero(const snn_params* p) { return !((float)(p->v_leak - p->v_th_lif) > 0.0f); }
struct DetWindows { StepWindow fc6, fc7; int enc_steps; };
static DetWindows det_windows(const snn_params* p, int T, bool spike_rates) {
    DetWindows w;
    if (knobs().dead_keep) { w.fc6 = w.fc7 = lif_window_all(T); w.enc_steps = T; return w; }
    w.fc7.t0 = (lif_first_spike_is_zero(p) && T >= 2) ? 1 : 0;
    w.fc7.n = (T - 1) - w.fc7.t0 > 0 ? (T - 1) - w.fc7.t0 : 1;
    const int last6 = spike_rates ? T - 1 : w.fc7.t0 + w.fc7.n - 1;          // last lif6 spike plane that is read
    w.fc6.t0 = 0;
    w.fc6.n = last6 > 0 ? last6 : 1;
    w.enc_steps = w.fc6.n;
    return w;
}

// M-tiles per wave (work-group rows = 64*MT): fewest rounds of work-groups x (tile work + per-chunk staging overhead)
template <typename F>
static int g3_pick_mt(F tiles_of) {
    int best = 0;
    double best_cost = 0;
    const int force = knobs().bf16x3_mt;                      // debug / A-B knob: 2, 3, 4 or 8 (8: fat waves, 4 x 2 grid only)
    if (force == 8 && knobs().bf16x3_wn == 2 && tiles_of(8) > 0) return 8;
    for (int mt = 4; mt >= 2; --mt) {
        const long long wgs = tiles_of(mt);
        if (wgs <= 0) continue;
        if (force == mt) return mt;
        const double cost = (double)((wgs + g3_slots() - 1) / g3_slots()) * (mt + 0.5);
        if (best_cost == 0 || cost < best_cost * 0.97) { best = mt; best_cost = cost; }
    }
    return best;
}

// T-in-tile launches: tile height = 16 * (mt - short / 2) rows per row-wave pair ... i.e. rows = row-waves * 16 * mt - 16 * n_short
// with n_short = 0 or half the row-waves (every SIMD then hosts one full and one short wave).  `wgs_of(rows)` = work-groups
// of the launch at that tile height (0: T does not fit).  Cost = rounds of work-groups per CU x (M-tiles per wave + per-chunk
// staging overhead); ties go to the larger tile.  SNN_BF16X3_MT / SNN_BF16X3_SHORT=0|1 force a shape (A/B, tests).
struct G3Tile { int mt, n_short, rows; };
template <typename F>
static G3Tile g3_pick_tile(int wn, F wgs_of) {
    G3Tile best = {0, 0, 0};
    double best_cost = 0;
    const int force_mt = knobs().bf16x3_mt, force_short = knobs().bf16x3_short;     // -1: by cost
    const int nwm = 8 / wn;
    if (force_mt == 8 && knobs().bf16x3_wn == 2 && wgs_of(256) > 0) return G3Tile{8, 0, 256};
    for (int mt = 4; mt >= 2; --mt)
        for (int sh = 0; sh < 2; ++sh) {
            if (force_mt >= 2 && force_mt <= 4 && force_mt != mt) continue;
            if (force_short >= 0 && force_short != sh) continue;
            const int n_short = sh ? nwm / 2 : 0, rows = nwm * 16 * mt - 16 * n_short;
            const long long wgs = wgs_of(rows);
            if (wgs <= 0) continue;
            const double cost = (double)((wgs + g3_slots() - 1) / g3_slots()) * (mt - 0.5 * sh + 0.5);
            if (best_cost == 0 || cost < best_cost * 0.97) { best = G3Tile{mt, n_short, rows}; best_cost = cost; }
        }
    return best;
}

#ifndef G3_NB1
#define G3_NB1 4                                    // ring slots of the 8 x 1 wave grid (14 KB each)
#endif
// waves along N of the bf16x3 tile: 1 (512 x 64 tile, 4-slot ring) or 2 (256 x 128 tile).  The 512 x 64 tile pulls half the
// weight-plane bytes per MFMA through the L2 -> LDS path, which is what the clock under these kernels pays for (DESIGN.md 4.1:
// +3.6 % clock); with row-major spike planes its doubled spike-word gather ate the gain, with word-major planes it is conv
// -1.7 %, detector head -1.5 %.  Defaults: the linear layers take it; the 3x3 convolution stays on 256 x 128, because with four
// column blocks every spike row and every output row passes through twice as many XCDs (FETCH 84 -> 190-206 MB, WRITE 98 ->
// 98-198 MB per launch) for those 1.7 %.  SNN_BF16X3_WN=1|2 forces one shape everywhere (A-B / test knob).
// (the conv ran the 256 x 128 tile until the end of round 3; with the straight-line LIF epilogue the 512 x 64 tile - half the weight bytes
// per MFMA, 4-slot ring - is 1-2 % faster there too: tools/ab_knobs.py, profiles/r3_k_ab_knobs.txt.  SNN_BF16X3_WN=2 selects the old shape)
static int g3_wn(bool conv = false) { (void)conv; return knobs().bf16x3_wn ? knobs().bf16x3_wn : 1; }

// rows of the work-group tile (MT = 8 is the 256 x 128 tile of MT = 4 / WN = 2 run by four fat waves)
static int g3_bm(int wn, int mt) { return mt == 8 ? 256 : G3_BM(wn, mt); }

template <int MODE>
static const void* g3_kernel(int mt, int wn, int planes) {
    if (planes == 1) {
        if (wn == 2)
            return mt == 8 ? (const void*)k_gemm_bf16<MODE, 3, 8, 2>
                 : mt == 4 ? (const void*)k_gemm_bf16<MODE, 3, 4, 2> : mt == 3 ? (const void*)k_gemm_bf16<MODE, 3, 3, 2>
                                                                                : (const void*)k_gemm_bf16<MODE, 3, 2, 2>;
        return mt == 4 ? (const void*)k_gemm_bf16<MODE, G3_NB1, 4, 1> : mt == 3 ? (const void*)k_gemm_bf16<MODE, G3_NB1, 3, 1>
                                                                                  : (const void*)k_gemm_bf16<MODE, G3_NB1, 2, 1>;
    }
    if (wn == 2)
        return mt == 8 ? (const void*)k_gemm_bf16x3<MODE, 3, 8, 2>
             : mt == 4 ? (const void*)k_gemm_bf16x3<MODE, 3, 4, 2> : mt == 3 ? (const void*)k_gemm_bf16x3<MODE, 3, 3, 2>
                                                                              : (const void*)k_gemm_bf16x3<MODE, 3, 2, 2>;
    return mt == 4 ? (const void*)k_gemm_bf16x3<MODE, G3_NB1, 4, 1> : mt == 3 ? (const void*)k_gemm_bf16x3<MODE, G3_NB1, 3, 1>
                                                                                : (const void*)k_gemm_bf16x3<MODE, G3_NB1, 2, 1>;
}

// ------------------------------------------------------------------------------------------------
// Exchange payload of the data-parallel path: per image the max_det RoIs with the highest foreground score
// (softmax over K, best class >= 1) as rows (the 4 regression values of that class, score, label), by decreasing score,
// ties by RoI index.  One work-group per image: scores -> 64-bit keys (score bits | 0xFFFF - RoI | label) -> bitonic
// sort in LDS -> gather.  Replaces ~12 small torch launches per batch in front of the all-gather.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long det_payload_key(const float* __restrict__ l, int K, int r) {
    float m = l[0];
    for (int c = 1; c < K; ++c) m = fmaxf(m, l[c]);
    float sum = 0.0f, best = -1.0f;
    int lab = 1;
    for (int c = 0; c < K; ++c) {
        const float e = expf(l[c] - m);
        sum += e;
        if (c >= 1 && e > best) { best = e; lab = c; }
    }
    const float score = best / sum;                             // > 0
    return ((unsigned long long)__float_as_uint(score) << 32) | ((unsigned long long)(0xFFFFu - (unsigned)r) << 16) | (unsigned)lab;
}

// E = keys per thread (npad = E * blockDim.x).  E == 1: the key lives in a register, partners closer than a wave are
// exchanged by lane shuffles (45 of the 55 stages at 1024 keys need no barrier).
template <int E>
__global__ __launch_bounds__(1024) void k_det_payload(const float* __restrict__ cls, const float* __restrict__ reg, int Rn,
                                                      int K, int max_det, int npad, float* __restrict__ payload,
                                                      int* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* const keys = reinterpret_cast<unsigned long long*>(smem);
    const int img = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const size_t base = (size_t)img * Rn;
    if (E == 1) {
        unsigned long long key = tid < Rn ? det_payload_key(cls + (base + tid) * K, K, tid) : 0ull;   // padding sorts last
        for (int k = 2; k <= npad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                unsigned long long other;
                if (j < 64) {
                    other = __shfl_xor(key, j);
                } else {
                    __syncthreads();
                    keys[tid] = key;
                    __syncthreads();
                    other = keys[tid ^ j];
                }
                const bool desc = (tid & k) == 0, lower = (tid & j) == 0;
                const bool take_max = desc == lower;            // descending overall
                key = take_max ? (key > other ? key : other) : (key < other ? key : other);
            }
        __syncthreads();
        keys[tid] = key;
        __syncthreads();
    } else {
        for (int r = tid; r < npad; r += nthr) keys[r] = r < Rn ? det_payload_key(cls + (base + r) * K, K, r) : 0ull;
        __syncthreads();
        for (int k = 2; k <= npad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < npad; i += nthr) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const unsigned long long a = keys[i], b = keys[ixj];
                        if ((i & k) == 0 ? a < b : a > b) { keys[i] = b; keys[ixj] = a; }
                    }
                }
                __syncthreads();
            }
    }
    const int n = min(max_det, Rn);
    for (int t = tid; t < max_det; t += nthr) {
        float* out = payload + ((size_t)img * max_det + t) * 6;
        if (t < n) {
            const unsigned long long key = keys[t];
            const int r = 0xFFFF - (int)((key >> 16) & 0xFFFFu), lab = (int)(key & 0xFFFFu);
            const float* d = reg + (base + r) * 4 * K + 4 * lab;
            out[0] = d[0]; out[1] = d[1]; out[2] = d[2]; out[3] = d[3];
            out[4] = __uint_as_float((uint32_t)(key >> 32));
            out[5] = (float)lab;
        } else {
            for (int q = 0; q < 6; ++q) out[q] = 0.0f;
        }
    }
    if (tid == 0) counts[img] = n;
}

// ---- the encoder kernel of a launch: K<..> for fp32 features, K_h<.., feat_f16 | feat_bf16> for half-precision ones (fdt has passed check_feat);
// with the layout bit SNN_FEAT_NHWC the channels-last kernel KN<.., float | feat_f16 | feat_bf16> (nullptr: the launch has none)
#define ENC_PICKER(fn, K, KN)                                                                                                                              \
    template <int EM>                                                                                                                                      \
    static const void* fn##_of(int fdt) {                                                                                                                  \
        if (fdt & SNN_FEAT_NHWC) return KN<EM>(fdt & ~SNN_FEAT_NHWC);                                                                                      \
        return fdt == SNN_FEAT_F16 ? (const void*)K##_h<EM, feat_f16> : fdt == SNN_FEAT_BF16 ? (const void*)K##_h<EM, feat_bf16> : (const void*)K<EM>;      \
    }                                                                                                                                                      \
    static const void* fn(int em, int fdt) { return em == ENC_QUANT ? fn##_of<ENC_QUANT>(fdt) : em == ENC_ZR ? fn##_of<ENC_ZR>(fdt) : fn##_of<ENC_GENERIC>(fdt); }
template <int EM> static const void* enc_nhwc_stage(int dt) {
    return dt == SNN_FEAT_F16 ? (const void*)k_encode_nhwc<EM, feat_f16> : dt == SNN_FEAT_BF16 ? (const void*)k_encode_nhwc<EM, feat_bf16> : (const void*)k_encode_nhwc<EM, float>;
}
template <int EM> static const void* enc_nhwc_levels(int dt) {
    return dt == SNN_FEAT_F16 ? (const void*)k_encode_levels_nhwc<EM, feat_f16> : dt == SNN_FEAT_BF16 ? (const void*)k_encode_levels_nhwc<EM, feat_bf16>
                                                                                                       : (const void*)k_encode_levels_nhwc<EM, float>;
}
template <int EM> static const void* enc_nhwc_none(int) { return nullptr; }      // (the row-fed entries refuse the bit)
ENC_PICKER(encode_nchw_kernel, k_encode_nchw, enc_nhwc_stage)
ENC_PICKER(encode_levels_kernel, k_encode_levels, enc_nhwc_levels)
ENC_PICKER(encode_rows_wm_kernel, k_encode_rows_wm, enc_nhwc_none)
#undef ENC_PICKER
static size_t feat_elem_bytes(int fdt) { return (fdt & ~SNN_FEAT_NHWC) == SNN_FEAT_F32 ? 4 : 2; }
template <int RB, int NW>
static const void* encode_rows_perm_of(int fdt) {
    return fdt == SNN_FEAT_F16 ? (const void*)k_encode_rows_perm_h<49, RB, NW, feat_f16> : fdt == SNN_FEAT_BF16 ? (const void*)k_encode_rows_perm_h<49, RB, NW, feat_bf16>
                                                                                                                 : (const void*)k_encode_rows_perm<49, RB, NW>;
}
static const void* encode_rows_perm_kernel(int rb, int nw, int fdt) {
    return rb == 16 ? (nw == 8 ? encode_rows_perm_of<16, 8>(fdt) : encode_rows_perm_of<16, 4>(fdt)) : (nw == 8 ? encode_rows_perm_of<8, 8>(fdt) : encode_rows_perm_of<8, 4>(fdt));
}
static const void* roi_align_encode_tab_kernel(int fdt) {
    return fdt == SNN_FEAT_F16 ? (const void*)k_roi_align_encode_tab_h<feat_f16> : fdt == SNN_FEAT_BF16 ? (const void*)k_roi_align_encode_tab_h<feat_bf16>
                                                                                                         : (const void*)k_roi_align_encode_tab;
}
template <int RW>
static const void* roi_align_encode_perm_kernel(int fdt) {
    if (fdt & SNN_FEAT_NHWC) {                                     // (channels-last maps: lanes = channels, snn_encode.h K1f)
        const int dt = fdt & ~SNN_FEAT_NHWC;
        return dt == SNN_FEAT_F16 ? (const void*)k_roi_align_encode_nhwc<RW, feat_f16> : dt == SNN_FEAT_BF16 ? (const void*)k_roi_align_encode_nhwc<RW, feat_bf16>
                                                                                                              : (const void*)k_roi_align_encode_nhwc<RW, float>;
    }
    return fdt == SNN_FEAT_F16 ? (const void*)k_roi_align_encode_perm_h<RW, feat_f16> : fdt == SNN_FEAT_BF16 ? (const void*)k_roi_align_encode_perm_h<RW, feat_bf16>
                                                                                                              : (const void*)k_roi_align_encode_perm<RW>;
}
// launch of a picked kernel: every argument has exactly its parameter's type (a refused launch is the thread's last error: SNN_CHECK_LAUNCH)
template <typename... A>
static void launch_picked(const void* kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... a) {
    void* kargs[] = {(void*)&a...};
    (void)hipLaunchKernel(kern, grid, block, kargs, lds, s);
}

extern "C" {

int snn_version(void) { return 2; }
void snn_debug_reload_knobs(void) { knobs() = load_knobs(); }
const char* snn_last_error(void) { return g_err; }

size_t snn_packed_gemm_elems(int K_chunks32, int N) { return (size_t)K_chunks32 * cdiv(N, 32) * 1024; }
size_t snn_packed_conv3x3_elems(int C_out, int C_in) { return snn_packed_gemm_elems(9 * cdiv(C_in, 32), C_out); }
size_t snn_packed_linear_elems(int N, int K) { return snn_packed_gemm_elems(cdiv(K, 32), N); }
size_t snn_packed_heads_elems(int NA, int NB, int K) {
    return (size_t)cdiv(K, 32) * 32 * (size_t)(cdiv(NA + NB, 16) * 16);
}

int snn_pack_conv3x3_weight(const float* w, int C_out, int C_in, float* packed, snn_stream_t s) {
    if (!w || !packed || C_out <= 0 || C_in <= 0) return fail(-1, "snn_pack_conv3x3_weight: bad argument");
    const int Cp = cdiv(C_in, 32) * 32, Kc = 9 * (Cp / 32), Nw = cdiv(C_out, 32);
    const size_t total = (size_t)Kc * Nw * 1024;
    hipLaunchKernelGGL(k_pack_gemm_b, dim3((unsigned)min((size_t)4096, (total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)s, w, packed, (int)PACK_CONV3X3, 9 * Cp, C_out, Kc, Nw, C_in, Cp);
    SNN_CHECK_LAUNCH("k_pack_gemm_b");
    return 0;
}

int snn_pack_linear_weight(const float* w, int N, int K, float* packed, snn_stream_t s) {
    if (!w || !packed || N <= 0 || K <= 0) return fail(-1, "snn_pack_linear_weight: bad argument");
    const int Kc = cdiv(K, 32), Nw = cdiv(N, 32);
    const size_t total = (size_t)Kc * Nw * 1024;
    hipLaunchKernelGGL(k_pack_gemm_b, dim3((unsigned)min((size_t)4096, (total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)s, w, packed, (int)PACK_LINEAR, K, N, Kc, Nw, 0, 32);
    SNN_CHECK_LAUNCH("k_pack_gemm_b");
    return 0;
}

int snn_pack_heads_weight(const float* wa, int NA, const float* wb, int NB, int K, float* packed,
                          snn_stream_t s) {
    if (!wa || !wb || !packed || NA <= 0 || NB <= 0 || K <= 0)
        return fail(-1, "snn_pack_heads_weight: bad argument");
    const int Kp = cdiv(K, 32) * 32, NOp = cdiv(NA + NB, 16) * 16;
    hipLaunchKernelGGL(k_pack_heads, dim3(cdiv((long long)Kp * NOp, 256)), dim3(256), 0, (hipStream_t)s, wa, NA,
                       wb, NB, K, Kp, NOp, packed);
    SNN_CHECK_LAUNCH("k_pack_heads");
    return 0;
}

static int check_T(int T, const char* who);

// ---- bf16x3 (exact 3-way bf16 weight split on the bf16 matrix cores) ----------------------------------
size_t snn_packed_bf16x3_elems(int K_chunks32, int N) { return (size_t)3 * K_chunks32 * (cdiv(N, 32) * 32) * 32; }
size_t snn_packed_conv3x3_bf16x3_elems(int C_out, int C_in) { return snn_packed_bf16x3_elems(9 * cdiv(C_in, 32), C_out); }
size_t snn_packed_linear_bf16x3_elems(int N, int K) { return snn_packed_bf16x3_elems(cdiv(K, 32), N); }

int snn_pack_conv3x3_weight_bf16x3(const float* w, int C_out, int C_in, uint16_t* packed, snn_stream_t s) {
    if (!w || !packed || C_out <= 0 || C_in <= 0) return fail(-1, "snn_pack_conv3x3_weight_bf16x3: bad argument");
    const int Cp = cdiv(C_in, 32) * 32, Kc = 9 * (Cp / 32), Np = cdiv(C_out, 32) * 32;
    const size_t total = (size_t)Kc * Np * 32;
    hipLaunchKernelGGL(k_pack_bf16x3, dim3((unsigned)min((size_t)4096, (total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)s, w, packed, (int)PACK_CONV3X3, 9 * Cp, C_out, Kc, Np, C_in, Cp);
    SNN_CHECK_LAUNCH("k_pack_bf16x3");
    return 0;
}

int snn_pack_linear_weight_bf16x3(const float* w, int N, int K, uint16_t* packed, snn_stream_t s) {
    if (!w || !packed || N <= 0 || K <= 0) return fail(-1, "snn_pack_linear_weight_bf16x3: bad argument");
    const int Kc = cdiv(K, 32), Np = cdiv(N, 32) * 32;
    const size_t total = (size_t)Kc * Np * 32;
    hipLaunchKernelGGL(k_pack_bf16x3, dim3((unsigned)min((size_t)4096, (total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)s, w, packed, (int)PACK_LINEAR, K, N, Kc, Np, 0, 32);
    SNN_CHECK_LAUNCH("k_pack_bf16x3");
    return 0;
}

int snn_check_bf16x3_split(const float* w, size_t n, uint32_t* status3, snn_stream_t s) {
    if (!w || !status3 || n == 0) return fail(-1, "snn_check_bf16x3_split: bad argument");
    if (hipMemsetAsync(status3, 0, 3 * sizeof(uint32_t), (hipStream_t)s) != hipSuccess) return fail(-3, "hipMemsetAsync failed");
    hipLaunchKernelGGL(k_bf16x3_split_check, dim3((unsigned)min((size_t)2048, (n + 255) / 256)), dim3(256), 0, (hipStream_t)s, w, n, status3);
    SNN_CHECK_LAUNCH("k_bf16x3_split_check");
    return 0;
}

int snn_pack_linear_weight_bf16x3_perm(const float* w, int N, int K, int inner, uint16_t* packed, snn_stream_t s) {
    if (!w || !packed || N <= 0 || K <= 0 || inner <= 0 || K % inner) return fail(-1, "snn_pack_linear_weight_bf16x3_perm: bad argument");
    const int Kc = cdiv(K, 32), Np = cdiv(N, 32) * 32;
    const size_t total = (size_t)Kc * Np * 32;
    hipLaunchKernelGGL(k_pack_bf16x3, dim3((unsigned)min((size_t)4096, (total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)s, w, packed, (int)PACK_LINEAR_PERM, K, N, Kc, Np, inner, K / inner);
    SNN_CHECK_LAUNCH("k_pack_bf16x3");
    return 0;
}

// ---- bf16 (precision "bf16"): ONE plane, every weight rounded once to the nearest bf16 -----------------------------------------------
size_t snn_packed_bf16_elems(int K_chunks32, int N) { return (size_t)K_chunks32 * (cdiv(N, 32) * 32) * 32; }
size_t snn_packed_conv3x3_bf16_elems(int C_out, int C_in) { return snn_packed_bf16_elems(9 * cdiv(C_in, 32), C_out); }
size_t snn_packed_linear_bf16_elems(int N, int K) { return snn_packed_bf16_elems(cdiv(K, 32), N); }

// the pack launch + its verdict: the call waits for the stream and fails if a weight was not finite or rounded to +-inf
static int pack_bf16_launch(const char* who, const float* w, uint16_t* packed, int mode, int K, int N, int Kc, int Np, int Cin, int Cp, snn_stream_t s) {
    const size_t total = (size_t)Kc * Np * 32;
    uint32_t* status = nullptr;
    if (hipMalloc((void**)&status, sizeof(uint32_t)) != hipSuccess) return fail(-3, "%s: hipMalloc failed", who);
    uint32_t bad = 0;
    hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), (hipStream_t)s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_pack_bf16, dim3((unsigned)min((size_t)4096, (total + 255) / 256)), dim3(256), 0, (hipStream_t)s, w, packed, mode, K, N, Kc, Np,
                           Cin, Cp, status);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, status, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)s);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)s);
    (void)hipFree(status);
    if (e != hipSuccess) return fail(-3, "%s: %s", who, hipGetErrorString(e));
    if (bad) return fail(-4, "%s: %u weight(s) are not finite or round to +-inf in bf16 (precision \"bf16\" has no other precision to fall back to)", who, bad);
    return 0;
}

int snn_pack_conv3x3_weight_bf16(const float* w, int C_out, int C_in, uint16_t* packed, snn_stream_t s) {
    if (!w || !packed || C_out <= 0 || C_in <= 0) return fail(-1, "snn_pack_conv3x3_weight_bf16: bad argument");
    const int Cp = cdiv(C_in, 32) * 32, Kc = 9 * (Cp / 32), Np = cdiv(C_out, 32) * 32;
    return pack_bf16_launch("snn_pack_conv3x3_weight_bf16", w, packed, (int)PACK_CONV3X3, 9 * Cp, C_out, Kc, Np, C_in, Cp, s);
}

int snn_pack_linear_weight_bf16(const float* w, int N, int K, uint16_t* packed, snn_stream_t s) {
    if (!w || !packed || N <= 0 || K <= 0) return fail(-1, "snn_pack_linear_weight_bf16: bad argument");
    return pack_bf16_launch("snn_pack_linear_weight_bf16", w, packed, (int)PACK_LINEAR, K, N, cdiv(K, 32), cdiv(N, 32) * 32, 0, 32, s);
}

int snn_pack_linear_weight_bf16_perm(const float* w, int N, int K, int inner, uint16_t* packed, snn_stream_t s) {
    if (!w || !packed || N <= 0 || K <= 0 || inner <= 0 || K % inner) return fail(-1, "snn_pack_linear_weight_bf16_perm: bad argument");
    return pack_bf16_launch("snn_pack_linear_weight_bf16_perm", w, packed, (int)PACK_LINEAR_PERM, K, N, cdiv(K, 32), cdiv(N, 32) * 32, inner, K / inner, s);
}

// ---- block-scaled fp6 digit planes (snn_mx.h) ---------------------------------------------------
size_t snn_packed_linear_mx_words(int N, int K) { return mx_words(cdiv(K, 128), cdiv(N, 32) * 32); }
size_t snn_packed_conv3x3_mx_words(int C_out, int C_in) { return mx_words(9 * cdiv(C_in, 128), cdiv(C_out, 32) * 32); }

int snn_pack_linear_weight_mx(const float* w, int N, int K, uint32_t* packed, snn_stream_t s) {
    if (!w || !packed || N <= 0 || K <= 0) return fail(-1, "snn_pack_linear_weight_mx: bad argument");
    const int Kc = cdiv(K, 128), Np = cdiv(N, 32) * 32;
    const size_t blocks = (size_t)Kc * Np * 4;
    hipLaunchKernelGGL(k_pack_mx, dim3((unsigned)min((size_t)8192, (blocks + 127) / 128)), dim3(128), 0, (hipStream_t)s, w, packed,
                       (int)PACK_LINEAR, K, N, Kc, Np, 0, 128);
    SNN_CHECK_LAUNCH("k_pack_mx");
    return 0;
}

int snn_pack_conv3x3_weight_mx(const float* w, int C_out, int C_in, uint32_t* packed, snn_stream_t s) {
    if (!w || !packed || C_out <= 0 || C_in <= 0) return fail(-1, "snn_pack_conv3x3_weight_mx: bad argument");
    const int Cp = cdiv(C_in, 128) * 128, Kc = 9 * Cp / 128, Np = cdiv(C_out, 32) * 32;
    const size_t blocks = (size_t)Kc * Np * 4;
    hipLaunchKernelGGL(k_pack_mx, dim3((unsigned)min((size_t)8192, (blocks + 127) / 128)), dim3(128), 0, (hipStream_t)s, w, packed,
                       (int)PACK_CONV3X3, 9 * Cp, C_out, Kc, Np, C_in, Cp);
    SNN_CHECK_LAUNCH("k_pack_mx");
    return 0;
}

// T-in-tile LIF fusion needs T <= 64 (one lane per time step keeps the spike words) and wastes rows % T rows per tile
static bool g3_tile_ok(int T, int rows) { return T >= 1 && T <= 64 && T <= rows && T * (rows / T) * 10 >= rows * 9; }
// some tile height of the bf16x3 family holds Tc time steps
static bool g3_some_tile_ok(int Tc, bool conv = false) {
    return g3_pick_tile(g3_wn(conv), [&](int rows) { return g3_tile_ok(Tc, rows) ? 1ll : 0ll; }).mt != 0;
}

struct G3Launch { Gemm3Args ax; int grid, lds, threads; const void* kern; };

// everything of a k_gemm_bf16x3 launch but the launch itself: kernel instance, LDS size, block order, grid
static int prepare_gemm3(int mode, int mt, int wn, const Gemm3Args& a, int planes, G3Launch* L) {
    // LIF_REG owns its CU (256 registers per wave); the others run two work-groups per CU
    const void* kern;
    int lds = G3_LDS(wn == 1 ? G3_NB1 : 3, wn), tiles = cdiv(a.M, g3_bm(wn, mt));
    const int threads = mt == 8 ? 256 : 512;
    const int tile_lds = (wn == 2 ? G3_TILE_BYTES(2) : G3_TILE_BYTES(1)) + G3_CNT_BYTES;   // the LIF_TILE epilogue reuses the ring (+ per-position spike counts)
    switch (mode) {
    case G3_FC: kern = g3_kernel<G3_FC>(mt, wn, planes); break;
    case G3_CONV: kern = g3_kernel<G3_CONV>(mt, wn, planes); break;
    case G3_CONV_LIF_REG: kern = planes == 1 ? (const void*)k_gemm_bf16<G3_CONV_LIF_REG, 3, 4, 2> : (const void*)k_gemm_bf16x3<G3_CONV_LIF_REG, 3, 4, 2>; lds = G3_LDS(3, 2) + G3_STATE_BYTES; break;
    case G3_CONV_LIF_TILE: kern = g3_kernel<G3_CONV_LIF_TILE>(mt, wn, planes); tiles = cdiv(a.M, a.pb); lds = max(lds, tile_lds); break;
    default: kern = g3_kernel<G3_FC_LIF_TILE>(mt, wn, planes); tiles = cdiv(a.M, a.pb); lds = max(lds, tile_lds); break;
    }
    static_assert(2 * (G3_TILE_BYTES(1) + G3_CNT_BYTES) <= 160 * 1024 && 2 * G3_LDS(3, 2) <= 160 * 1024, "two work-groups per CU");
    // XCD-aware order for launches with 4, 8 or 16 column blocks whose weight panels are small enough to stay in an XCD's L2
    // in pairs (the RPN conv: 2 x 0.9 MB): see k_gemm_bf16x3.  SNN_BF16X3_XCD=0 switches it off (A/B).
    Gemm3Args& ax = L->ax;
    ax = a;
    ax.n_tiles = tiles; ax.xcd_classes = 0;
    ax.epi_general = knobs().epi_general;
    int grid = tiles * a.n_blocks;
    const size_t pair_bytes = (size_t)2 * G3_BN(wn) * a.Kc * 32 * 2 * planes;
    const bool conv_mode = mode == G3_CONV || mode == G3_CONV_LIF_TILE;
    if (knobs().bf16x3_xcd && mt != 8 && conv_mode && (a.n_blocks == 2 || (a.n_blocks == 4 && pair_bytes <= (size_t)2 << 20)) && tiles >= 64) {
        // 3x3 convolution with two / four column blocks: half of them and a contiguous quarter of the row tiles per XCD (halo rows stay
        // in one L2, every spike row is fetched by two XCDs)
        ax.xcd_cpx = a.n_blocks / 2;
        ax.xcd_contig = cdiv(tiles, 4);
        grid = ax.xcd_contig * ax.xcd_cpx * 8;
    } else if (knobs().bf16x3_xcd && mt != 8 && (a.n_blocks == 4 || a.n_blocks == 8 || a.n_blocks == 16) && pair_bytes <= (size_t)2 << 20) {
        ax.xcd_classes = 8 / (a.n_blocks / 2);
        grid = cdiv(tiles, ax.xcd_classes) * ax.xcd_classes * a.n_blocks;
    }
#ifdef SNN_EXP_ONE_WG_PER_CU                                       // timing experiment: ask for so much LDS that only one work-group fits a CU
    lds = max(lds, 100 * 1024);
#endif
    L->grid = grid; L->lds = lds; L->threads = threads; L->kern = kern;
    return 0;
}

static int launch_gemm3(int mode, int mt, int wn, const Gemm3Args& a, int planes, hipStream_t s) {
    G3Launch L;
    prepare_gemm3(mode, mt, wn, a, planes, &L);
    hipError_t e = hipFuncSetAttribute(L.kern, hipFuncAttributeMaxDynamicSharedMemorySize, L.lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    if (knobs().debug_occ) {                                   // debug: co-resident work-groups per CU
        int v = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, L.kern, L.threads, L.lds);
        fprintf(stderr, "k_gemm_bf16x3 mode %d mt %d wn %d short %d: pb %d x Tc %d rows, lds %d B, %d work-groups per CU, grid %d\n", mode, mt, wn,
                a.n_short, a.pb, a.Tc, L.lds, v, L.grid);
    }
    void* kargs[] = {(void*)&L.ax};
    e = hipLaunchKernel(L.kern, dim3(L.grid), dim3(L.threads), kargs, L.lds, s);
    if (e != hipSuccess) return fail(-3, "k_gemm_bf16x3 launch failed: %s", hipGetErrorString(e));
    SNN_CHECK_LAUNCH("k_gemm_bf16x3");
    return 0;
}

int snn_debug_encoder_thresholds(const snn_params* p, float* th32) {
    static_assert(SNN_MAX_STEPS == 32, "EncTh holds 32 thresholds");
    if (!p || !th32) return fail(-1, "snn_debug_encoder_thresholds: null argument");
    const EncThTable& t = enc_thresholds(p->dt_tau_mem, p->v_th_enc);
    memcpy(th32, t.t.th, sizeof(t.t.th));
    return (t.ok && p->v_leak == 0.0f && p->v_reset == 0.0f) ? 1 : 0;
}

// The shader clock the chip HOLDS while other work runs (bench.py: `held_clock`): ONE wave that sleeps and polls the constant 100-MHz counter
// (s_memrealtime) until `ticks` of it have passed, then reports how many shader-clock cycles (s_memtime) went by.  Launched on a side stream beside
// the step it costs one wave slot of one CU and a few scalar instructions per microsecond.  out2[0] = cycles, out2[1] = ticks: GHz = 0.1 * cycles / ticks.
__global__ __launch_bounds__(64) void k_clock_probe(unsigned long long* out2, const unsigned int ticks) {
    unsigned long long t0, c0, t1, c1;
    asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0), "=s"(c0) :: "memory");
    do {
        __builtin_amdgcn_s_sleep(32);
        asm volatile("s_memrealtime %0\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1), "=s"(c1) :: "memory");
    } while (t1 - t0 < (unsigned long long)ticks);
    if (threadIdx.x == 0) { out2[0] = c1 - c0; out2[1] = t1 - t0; }
}

int snn_debug_clock_probe(unsigned long long* out2_dev, unsigned int ticks_100mhz, snn_stream_t stream) {
    if (!out2_dev || ticks_100mhz == 0 || ticks_100mhz > 100u * 1000u * 1000u) return fail(-1, "snn_debug_clock_probe: bad argument (at most one second)");
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, out2_dev, ticks_100mhz);
    SNN_CHECK_LAUNCH("k_clock_probe");
    return 0;
}

int snn_debug_last_enc_mode(void) { return g_last_enc_mode; }
int snn_debug_last_conv_path(void) { return g_last_conv_sparse; }
int snn_debug_last_fc6_path(void) { return g_last_fc_sparse; }
void snn_debug_last_rpn_planes(unsigned long long* out3) { if (out3) for (int i = 0; i < 3; ++i) out3[i] = g_last_rpn_planes[i]; }
void snn_debug_last_det_planes(unsigned long long* out3) { if (out3) for (int i = 0; i < 3; ++i) out3[i] = g_last_det_planes[i]; }

static int spike_gemm_bf16x3_impl(const uint32_t* a_rows, int M, int K, int N, const uint16_t* w_packed, float* cur, int ldo, int planes,
                                  snn_stream_t s) {
    if (!a_rows || !w_packed || !cur || M <= 0 || K <= 0 || N <= 0 || ldo < N)
        return fail(-1, "snn_spike_gemm_bf16x3: bad argument");
    Gemm3Args a;
    memset(&a, 0, sizeof(a));
    if ((long long)M * cdiv(K, 32) * 4 > 0xffffffffLL) return fail(-1, "snn_spike_gemm_bf16x3: spike rows over 4 GB");
    a.A = a_rows; a.wpk = w_packed; a.out = cur; a.M = M; a.Kc = cdiv(K, 32); a.Np = cdiv(N, 32) * 32; a.ldo = ldo;
    a.plane_elems = (unsigned long long)a.Kc * a.Np * 32;
    const int wn = g3_wn();
    a.n_blocks = cdiv(a.Np, G3_BN(wn));
    const int mt = g3_pick_mt([&](int m) { return (long long)cdiv(M, g3_bm(wn, m)) * a.n_blocks; });
    return launch_gemm3(G3_FC, mt, wn, a, planes, (hipStream_t)s);
}

int snn_spike_gemm_bf16x3(const uint32_t* a_rows, int M, int K, int N, const uint16_t* w_packed, float* cur, int ldo,
                          snn_stream_t s) {
    return spike_gemm_bf16x3_impl(a_rows, M, K, N, w_packed, cur, ldo, 3, s);
}

// period planes: row group n - 1 of a tile holds u_n = W e_n; the current of step t < Tc is the sum over the divisors n <= Tc of t + 1
static int set_periods(Gemm3Args& a, const char* who) {
    if (a.t0 != 0) return fail(-1, "%s: period planes need a window that starts at step 0", who);
    a.periods = 1;
    for (int t = 0; t < SNN_MAX_STEPS; ++t) {
        a.div[t] = 0;
        if (t < a.Tc)
            for (int n = 1; n <= a.Tc; ++n)
                if ((t + 1) % n == 0) a.div[t] |= 1u << (n - 1);
    }
    return 0;
}

// row_counts (nullable, zeroed by the caller): spikes per row over all T steps and N columns, added by the LIF epilogue
static int spike_gemm_lif_bf16x3_args(const uint32_t* a_planes, int T, int R, int K, int N, const snn_params* p,
                                      const uint16_t* w_packed, uint32_t* spk, size_t spk_stride, uint32_t* row_counts,
                                      bool wm_in, bool wm_out, const StepWindow* win, bool periods, Gemm3Args* out, G3Tile* tile) {
    if (!a_planes || !w_packed || !spk || !p || R <= 0 || K <= 0 || N <= 0)
        return fail(-1, "snn_spike_gemm_lif_bf16x3: bad argument");
    if (check_T(T, "snn_spike_gemm_lif_bf16x3")) return -1;
    if ((long long)T * R * cdiv(K, 32) * 4 > 0xffffffffLL) return fail(-1, "snn_spike_gemm_lif_bf16x3: input planes over 4 GB");
    Gemm3Args& a = *out;
    memset(&a, 0, sizeof(a));
    a.A = a_planes; a.wpk = w_packed; a.M = R; a.Kc = cdiv(K, 32); a.Np = cdiv(N, 32) * 32;
    a.plane_elems = (unsigned long long)a.Kc * a.Np * 32;
    const int wn = g3_wn();
    a.n_blocks = cdiv(a.Np, G3_BN(wn));
    a.T = T; a.spk = spk; a.spk_stride = spk_stride; a.p = make_p(p, p->v_th_lif); a.cnt_row = row_counts;
    a.wm = wm_in; a.out_wm = wm_out; a.a_step = (unsigned long long)R;       // word-major planes [T][K/32][R]
    const StepWindow w = win ? *win : lif_window_full_out(T);                // time steps whose currents are formed
    a.t0 = w.t0; a.Tc = w.n;
    const int Tc = w.n;
    const G3Tile tl = g3_pick_tile(wn, [&](int rows) { return g3_tile_ok(Tc, rows) ? (long long)cdiv(R, rows / Tc) * a.n_blocks : 0ll; });
    if (!tl.mt) return fail(-4, "snn_spike_gemm_lif_bf16x3: T=%d does not fit a row tile (use snn_spike_gemm_bf16x3 + snn_lif_scan)", T);
    a.pb = tl.rows / Tc; a.n_short = tl.n_short;
    if (periods && set_periods(a, "snn_spike_gemm_lif_bf16x3")) return -1;
    *tile = tl;
    return 0;
}

static int spike_gemm_lif_bf16x3_impl(const uint32_t* a_planes, int T, int R, int K, int N, const snn_params* p,
                                      const uint16_t* w_packed, uint32_t* spk, size_t spk_stride, uint32_t* row_counts, snn_stream_t s,
                                      bool wm_in = false, bool wm_out = false, const StepWindow* win = nullptr, bool periods = false) {
    Gemm3Args a;
    G3Tile tl;
    const int rc = spike_gemm_lif_bf16x3_args(a_planes, T, R, K, N, p, w_packed, spk, spk_stride, row_counts, wm_in, wm_out, win, periods, &a, &tl);
    if (rc) return rc;
    return launch_gemm3(G3_FC_LIF_TILE, tl.mt, g3_wn(), a, 3, (hipStream_t)s);
}

int snn_spike_gemm_lif_bf16x3(const uint32_t* a_planes, int T, int R, int K, int N, const snn_params* p,
                              const uint16_t* w_packed, uint32_t* spk, size_t spk_stride, snn_stream_t s) {
    return spike_gemm_lif_bf16x3_impl(a_planes, T, R, K, N, p, w_packed, spk, spk_stride, nullptr, s, knobs().stage_wm, false, nullptr,
                                      knobs().stage_periods);
}

// ---- spike GEMMs on the block-scaled fp4 x fp6 path (snn_mx.h) ------------------------------------
static bool mx_tile_ok(int T) { return g3_tile_ok(T, MX_BM); }

// rows per wave: 4 M-tiles (8 waves, 128 registers; default) or 8 (4 waves, 256 registers: half the LDS fragment reads
// per MFMA - measured equal in the loop, slower in the LIF epilogue); SNN_MX_MW=4|8 overrides (debug / A-B switch)
static int mx_mw() { return knobs().mx_mw ? knobs().mx_mw : MX_MW_DEFAULT; }

#define MX_KERNEL_OF(MW, mode)                                                                        \
    ((mode) == G3_FC ? (const void*)k_gemm_mx<G3_FC, MW>                                              \
     : (mode) == G3_CONV ? (const void*)k_gemm_mx<G3_CONV, MW>                                        \
     : (mode) == G3_CONV_LIF_TILE ? (const void*)k_gemm_mx<G3_CONV_LIF_TILE, MW>                      \
                                  : (const void*)k_gemm_mx<G3_FC_LIF_TILE, MW>)

static int launch_gemm_mx(int mode, MxArgs& a, hipStream_t s) {
    const int mw = mx_mw();
    const void* kern = mw == 8 ? MX_KERNEL_OF(8, mode) : MX_KERNEL_OF(4, mode);
    const bool tile = mode == G3_CONV_LIF_TILE || mode == G3_FC_LIF_TILE;
    const int lds = tile ? max((int)MX_LDS, (int)(G3_TILE_BYTES(1) + G3_CNT_BYTES)) : MX_LDS;
    const int tiles = tile ? cdiv(a.g.M, a.g.pb) : cdiv(a.g.M, MX_BM);
    a.g.n_blocks = cdiv(a.g.Np, MX_BN);
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    if (knobs().debug_occ) {
        int v = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kern, 2048 / mw, lds);
        fprintf(stderr, "k_gemm_mx mode %d mw %d: lds %d B, %d work-groups per CU, grid %d\n", mode, mw, lds, v, tiles * a.g.n_blocks);
    }
    void* kargs[] = {(void*)&a};
    e = hipLaunchKernel(kern, dim3(tiles * a.g.n_blocks), dim3(2048 / mw), kargs, lds, s);
    if (e != hipSuccess) return fail(-3, "k_gemm_mx launch failed: %s", hipGetErrorString(e));
    SNN_CHECK_LAUNCH("k_gemm_mx");
    return 0;
}

int snn_spike_gemm_mx(const uint32_t* a_rows, int M, int K, int N, const uint32_t* w_packed, float* cur, int ldo,
                      snn_stream_t s) {
    if (!a_rows || !w_packed || !cur || M <= 0 || K <= 0 || N <= 0 || ldo < N) return fail(-1, "snn_spike_gemm_mx: bad argument");
    if (K % 128) return fail(-4, "snn_spike_gemm_mx: K=%d is not a multiple of 128 (use the bf16x3 kernels)", K);
    if ((long long)M * (K / 32) * 4 > 0xffffffffLL) return fail(-1, "snn_spike_gemm_mx: spike rows over 4 GB");
    MxArgs a;
    memset(&a, 0, sizeof(a));
    a.g.A = a_rows; a.g.out = cur; a.g.M = M; a.g.Np = cdiv(N, 32) * 32; a.g.ldo = ldo;
    a.wq = w_packed; a.Kc = K / 128;
    return launch_gemm_mx(G3_FC, a, (hipStream_t)s);
}

static int spike_gemm_lif_mx_impl(const uint32_t* a_planes, int T, int R, int K, int N, const snn_params* p,
                                  const uint32_t* w_packed, uint32_t* spk, size_t spk_stride, uint32_t* row_counts, snn_stream_t s,
                                  const StepWindow* win = nullptr) {
    if (!a_planes || !w_packed || !spk || !p || R <= 0 || K <= 0 || N <= 0) return fail(-1, "snn_spike_gemm_lif_mx: bad argument");
    if (check_T(T, "snn_spike_gemm_lif_mx")) return -1;
    if (K % 128) return fail(-4, "snn_spike_gemm_lif_mx: K=%d is not a multiple of 128", K);
    const StepWindow w = win ? *win : lif_window_full_out(T);
    if (!mx_tile_ok(w.n)) return fail(-4, "snn_spike_gemm_lif_mx: T=%d does not fit a row tile", T);
    if ((long long)T * R * (K / 32) * 4 > 0xffffffffLL) return fail(-1, "snn_spike_gemm_lif_mx: input planes over 4 GB");
    MxArgs a;
    memset(&a, 0, sizeof(a));
    a.g.A = a_planes; a.g.M = R; a.g.Np = cdiv(N, 32) * 32;
    a.g.T = T; a.g.spk = spk; a.g.spk_stride = spk_stride; a.g.p = make_p(p, p->v_th_lif); a.g.pb = MX_BM / w.n;
    a.g.t0 = w.t0; a.g.Tc = w.n;
    a.g.cnt_row = row_counts;
    a.wq = w_packed; a.Kc = K / 128;
    return launch_gemm_mx(G3_FC_LIF_TILE, a, (hipStream_t)s);
}

int snn_spike_gemm_lif_mx(const uint32_t* a_planes, int T, int R, int K, int N, const snn_params* p,
                          const uint32_t* w_packed, uint32_t* spk, size_t spk_stride, snn_stream_t s) {
    return spike_gemm_lif_mx_impl(a_planes, T, R, K, N, p, w_packed, spk, spk_stride, nullptr, s);
}

static int conv_mx_common(const char* who, const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels,
                          int C_in, int C_out, int T, const uint32_t* w_packed, MxArgs& a, long long* P_out) {
    if (!enc || !lv || !w_packed || n_levels <= 0 || n_levels > SNN_MAX_LEVELS || C_in <= 0 || C_out <= 0)
        return fail(-1, "%s: bad argument", who);
    if (C_in % 128) return fail(-4, "%s: C_in=%d is not a multiple of 128 (use the bf16x3 kernels)", who, C_in);
    if (check_T(T, who)) return -1;
    memset(&a, 0, sizeof(a));
    long long P = 0, Pp = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (lv[l].N <= 0 || lv[l].H <= 0 || lv[l].W <= 0) return fail(-1, "%s: bad level %d", who, l);
        a.g.lv[l].pos_base = (int)P; a.g.lv[l].N = lv[l].N; a.g.lv[l].H = lv[l].H; a.g.lv[l].W = lv[l].W;
        a.g.lv[l].tile_begin = (int)Pp;                // first row of the level in the padded (zero-halo) encoder planes
        P += (long long)lv[l].N * lv[l].H * lv[l].W;
        Pp += (long long)lv[l].N * (lv[l].H + 2) * (lv[l].W + 2);
    }
    if ((long long)T * P > 0x7fffffffLL) return fail(-1, "%s: T*P too large", who);
    if (enc_stride < (size_t)Pp * (C_in / 32)) return fail(-1, "%s: enc_stride %zu < %lld words (planes with a one-position zero halo)", who, enc_stride, Pp * (C_in / 32));
    if (((long long)(T - 1) * (long long)enc_stride + Pp * (C_in / 32)) * 4 > 0xffffffffLL) return fail(-1, "%s: encoder planes over 4 GB", who);
    a.g.A = enc; a.g.enc_stride = enc_stride; a.g.Cw = C_in / 32; a.g.Np = cdiv(C_out, 32) * 32;
    a.g.P_total = (int)P; a.g.n_levels = n_levels;
    a.wq = w_packed; a.Kc = 9 * C_in / 128;
    *P_out = P;
    return 0;
}

// counts (nullable, zeroed by the caller): shared-LIF spikes per (level, image) slot l * max_n + n, added by the LIF epilogue
static int conv3x3_lif_mx_impl(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in, int C_out,
                               int T, const snn_params* p, const uint32_t* w_packed, uint32_t* spk, size_t spk_stride,
                               unsigned long long* counts, int max_n, snn_stream_t s) {
    if (!spk || !p) return fail(-1, "snn_conv3x3_lif_mx: bad argument");
    MxArgs a;
    long long P;
    int rc = conv_mx_common("snn_conv3x3_lif_mx", enc, enc_stride, lv, n_levels, C_in, C_out, T, w_packed, a, &P);
    if (rc) return rc;
    const StepWindow w = lif_window_full_out(T);
    if (!mx_tile_ok(w.n)) return fail(-4, "snn_conv3x3_lif_mx: T=%d does not fit a row tile", T);
    a.g.M = (int)P; a.g.T = T; a.g.spk = spk; a.g.spk_stride = spk_stride; a.g.p = make_p(p, p->v_th_lif); a.g.pb = MX_BM / w.n;
    a.g.t0 = w.t0; a.g.Tc = w.n;
    a.g.cnt_img = counts; a.g.max_n = max_n;
    return launch_gemm_mx(G3_CONV_LIF_TILE, a, (hipStream_t)s);
}

int snn_conv3x3_lif_mx(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in, int C_out,
                       int T, const snn_params* p, const uint32_t* w_packed, uint32_t* spk, size_t spk_stride,
                       snn_stream_t s) {
    return conv3x3_lif_mx_impl(enc, enc_stride, lv, n_levels, C_in, C_out, T, p, w_packed, spk, spk_stride, nullptr, 0, s);
}

int snn_spike_conv3x3_mx(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in, int C_out,
                         int T, const uint32_t* w_packed, float* cur, int ldo, snn_stream_t s) {
    if (!cur || ldo < C_out) return fail(-1, "snn_spike_conv3x3_mx: bad argument");
    MxArgs a;
    long long P;
    int rc = conv_mx_common("snn_spike_conv3x3_mx", enc, enc_stride, lv, n_levels, C_in, C_out, T, w_packed, a, &P);
    if (rc) return rc;
    a.g.M = (int)(T * P); a.g.out = cur; a.g.ldo = ldo;
    return launch_gemm_mx(G3_CONV, a, (hipStream_t)s);
}

static int conv3_common(const char* who, const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels,
                        int C_in, int C_out, int T, const uint16_t* w_packed, Gemm3Args& a, long long* P_out) {
    if (!enc || !lv || !w_packed || n_levels <= 0 || n_levels > SNN_MAX_LEVELS || C_in <= 0 || C_out <= 0)
        return fail(-1, "%s: bad argument", who);
    if (check_T(T, who)) return -1;
    memset(&a, 0, sizeof(a));
    long long P = 0, Pp = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (lv[l].N <= 0 || lv[l].H <= 0 || lv[l].W <= 0) return fail(-1, "%s: bad level %d", who, l);
        a.lv[l].pos_base = (int)P; a.lv[l].N = lv[l].N; a.lv[l].H = lv[l].H; a.lv[l].W = lv[l].W;
        a.lv[l].tile_begin = (int)Pp;                  // first row of the level in the padded (zero-halo) encoder planes
        P += (long long)lv[l].N * lv[l].H * lv[l].W;
        Pp += (long long)lv[l].N * (lv[l].H + 2) * (lv[l].W + 2);
    }
    if ((long long)T * P > 0x7fffffffLL) return fail(-1, "%s: T*P too large", who);
    if (enc_stride < (size_t)Pp * cdiv(C_in, 32))
        return fail(-1, "%s: enc_stride %zu < %lld words (planes with a one-position zero halo)", who, enc_stride, Pp * cdiv(C_in, 32));
    // the kernels address a spike word as 64-bit scalar base + 32-bit lane byte offset
    if (((long long)(T - 1) * (long long)enc_stride + Pp * cdiv(C_in, 32)) * 4 > 0xffffffffLL)
        return fail(-1, "%s: encoder planes over 4 GB", who);
    a.A = enc; a.wpk = w_packed; a.enc_stride = enc_stride;
    a.Cw = cdiv(C_in, 32); a.Kc = 9 * a.Cw; a.Np = cdiv(C_out, 32) * 32;
    a.plane_elems = (unsigned long long)a.Kc * a.Np * 32;
    a.P_total = (int)P; a.n_levels = n_levels;
    *P_out = P;
    return 0;
}

static int count_spikes_per_image(const snn_rpn_level* lv, int n_levels, int Cw, int T, const uint32_t* spk, size_t stride,
                                  unsigned long long* counts, int max_n, hipStream_t s);

static size_t sparse_side_bytes(long long P, long long Pe, int Kw, int T);
// ---- structured-sparse conv (snn_sparse.h): tile geometry + wave assignment ----
struct SparsePlan { int q, pb, nd, wn, fat; signed char plane[8][SP_MTMAX]; unsigned char j[8][SP_MTMAX], w_nd[8], w_ns[8]; };
// q = M-tiles (16 positions / RoIs each) per plane.  The conv has thousands of tiles and takes the largest one; a linear layer with a few
// hundred work-groups takes the q with the fewest rounds of work-groups x work per tile (fc6 at 2000 RoIs, 10 planes: q = 3 is 672
// work-groups = 1.31 rounds of the 512 slots, q = 2 is 1008 = 1.97 rounds of tiles two thirds the size: 687 -> ~520 us)
// FAT conv (round 5): four waves; T = 7 .. 9: 4 x 1, wave w holds ALL planes of position block w (slot s = plane s, tiles of 64 positions); T = 12 .. 16
// (loop instances exist from T = 10; 10 / 11 are not planned, see below): 2 x 2, row-wave wm holds all planes of block wm for its column-wave's 32
// columns (tiles of 32 positions) - what the register LIF needs
static bool sparse_plan_fat_conv(int Tc, SparsePlan* sp) {
    static const int inst_a[][2] = {SP_FAT1_INSTANCES}, inst_b[][2] = {SP_FAT1B_INSTANCES};
    bool ok_a = false, ok_b = false;
    for (size_t i = 0; i < sizeof(inst_a) / sizeof(inst_a[0]); ++i) ok_a |= inst_a[i][0] == 2 && inst_a[i][1] == Tc - 2;
    for (size_t i = 0; i < sizeof(inst_b) / sizeof(inst_b[0]); ++i) ok_b |= inst_b[i][0] == 2 && inst_b[i][1] == Tc - 2;
    // (T = 10 / 11 stay on the 8-wave shape, whose tiles hold 48 positions there: the 2 x 2 shape measured +2 % / +4 %; -5.6 % / -7.3 % / -1.1 % at T = 12 / 14 / 16)
    ok_a &= Tc <= SP_MT_FAT; ok_b &= Tc >= 11 && Tc <= SP_MT2_FAT_CONV && !ok_a;
    if (!ok_a && !ok_b) return false;
    if (ok_b && !(knobs().sparse_fat_conv & 2)) return false;
    if (ok_a && !(knobs().sparse_fat_conv & 1)) return false;
    const int nwm = ok_a ? 4 : 2;
    memset(sp, 0, sizeof(*sp));
    sp->q = nwm; sp->pb = 16 * nwm; sp->nd = 2; sp->wn = ok_a ? 1 : 2; sp->fat = 1;
    for (int w = 0; w < 8; ++w)
        for (int m = 0; m < SP_MTMAX; ++m) { sp->plane[w][m] = (w < nwm && m < Tc) ? (signed char)m : (signed char)-1; sp->j[w][m] = (unsigned char)(w % nwm); }
    for (int w = 0; w < nwm; ++w) { sp->w_nd[w] = 2; sp->w_ns[w] = (unsigned char)(Tc - 2); }
    return true;
}

// may the LIF of this FAT plan run in registers (snn_sparse.h: sp_lif_regs)?  Every (row-)wave must hold ALL planes of its own block
// (slot s = plane s, block = the row-wave), the (T, window) must have an instance, and the launch must not count spikes.
static bool sparse_plan_lif_regs(const SparsePlan& sp, bool conv, int T, int Tc, bool counting, int epi_general) {
    if (!sp.fat || (counting && !conv) || epi_general || !knobs().lif_regs) return false;
    if (conv ? (sp.wn == 1 ? (T < 7 || T > 9) : (T < 10 || T > 16)) : (T < 6 || T > 14)) return false;
    const int nwm = 4 / sp.wn;
    if (sp.q != nwm) return false;
    for (int w = 0; w < nwm; ++w)
        for (int m = 0; m < Tc; ++m)
            if (sp.plane[w][m] != m || sp.j[w][m] != w) return false;
    return true;
}

static bool sparse_plan_wn(int Tc, int wn, int q, SparsePlan* sp, bool fat = false) {
    const int nd = 2, nwm = (fat ? 4 : 8) / wn, mts = fat ? SP_MT2_FAT : wn == 1 ? SP_MT : SP_MT2;
    if (q < 1 || Tc * q > nwm * mts || (fat && wn != 2)) return false;
    memset(sp, 0, sizeof(*sp));
    sp->q = q; sp->pb = 16 * q; sp->nd = nd; sp->wn = wn; sp->fat = fat ? 1 : 0;
    int used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double cost[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w < 8; ++w)
        for (int m = 0; m < SP_MTMAX; ++m) sp->plane[w][m] = -1;
    int w_rr = 0;
    for (int t = 0; t < nd; ++t)                           // dense M-tiles: round-robin over the row-waves
        for (int jj = 0; jj < q; ++jj) {
            const int w = w_rr++ % nwm;
            if (used[w] >= mts) return false;
            sp->plane[w][used[w]] = (signed char)t; sp->j[w][used[w]] = (unsigned char)jj;
            ++used[w]; ++sp->w_nd[w]; cost[w] += 2.0;
        }
    for (int t = nd; t < Tc; ++t)                          // sparse M-tiles: to the cheapest row-wave with a free slot
        for (int jj = 0; jj < q; ++jj) {
            int best = -1;
            for (int w = 0; w < nwm; ++w)
                if (used[w] < mts && (best < 0 || cost[w] < cost[best] - 1e-9)) best = w;
            if (best < 0) return false;
            sp->plane[best][used[best]] = (signed char)t; sp->j[best][used[best]] = (unsigned char)jj;
            ++used[best]; ++sp->w_ns[best]; cost[best] += 1.1;
        }
    // loop instances that exist (snn_sparse.h: SP_CASE)
    static const int inst1[][2] = {{1, 3}, {1, 2}, {2, 2}, {0, 4}, {0, 3}, {1, 1}, {2, 1}, {0, 2}, {0, 1}, {2, 0}, {1, 0}, {0, 0}, {0, 0}, {0, 0}};
    static const int inst2[][2] = {{1, 4}, {1, 5}, {2, 4}, {2, 3}, {1, 3}, {0, 6}, {0, 5}, {2, 2}, {0, 4}, {1, 2}, {0, 3}, {0, 0}, {0, 0}, {0, 0}};
    static const int inst_fat2[][2] = {SP_FAT2_INSTANCES, {0, 0}};
    for (int w = 0; w < nwm; ++w) {
        bool ok = false;
        if (fat) {
            for (size_t i = 0; i < sizeof(inst_fat2) / sizeof(inst_fat2[0]); ++i) ok |= inst_fat2[i][0] == sp->w_nd[w] && inst_fat2[i][1] == sp->w_ns[w];
        } else {
            for (int i = 0; i < 14; ++i) {
                const int* c = wn == 1 ? inst1[i] : inst2[i];
                ok |= c[0] == sp->w_nd[w] && c[1] == sp->w_ns[w];
            }
        }
        if (!ok) return false;
    }
    return true;
}

// q = M-tiles (16 positions / RoIs each) per plane.  The conv has thousands of tiles and takes the largest one on the 8 x 1 wave grid
// (its K loop is matrix-pipe-bound there).  A linear layer with a few hundred work-groups takes the (wave grid, q) with the fewest
// rounds of work-groups x work per tile; on the 8 x 1 grid small tiles are LDS-bound (every wave reads the whole weight slot), so the
// 4 x 2 grid is preferred where its plan exists (fc6 at 2000 RoIs, 10 planes: q = 2 on 4 x 2 = 1008 work-groups = 1.97 rounds).
static bool sparse_plan(int Tc, SparsePlan* sp, long long units = 0, int n_blocks = 0) {
    if (Tc < 4 || Tc > 32) return false;
    const bool conv = !(units > 0 && n_blocks > 0);
    const bool fat = !conv && knobs().sparse_fat;           // linear layers: the same tiles on four fat waves, where the plan's row-waves have loop instances
    if (conv) {
        if (knobs().sparse_fat_conv && knobs().lif_regs && sparse_plan_fat_conv(Tc, sp)) return true;      // (register LIF only: T = Tc + 1 = 7 .. 16)
        int q = 32 / Tc;
        if (q > 8) q = 8;
        return sparse_plan_wn(Tc, 1, q, sp);
    }
    const int slots = 2 * g3_slots();
    bool have = false;
    double best_cost = 0;
    SparsePlan cand;
    for (int wn = 2; wn >= 1; --wn)
        for (int c = (wn == 1 ? 32 : 24) / Tc; c >= 1; --c) {
            if (!sparse_plan_wn(Tc, wn, c, &cand)) continue;
            const long long wgs = (long long)cdiv(units, 16 * c) * n_blocks;
            // per-tile cost: matrix work + a fixed part; on the 8 x 1 grid a step cannot be shorter than its LDS reads (~ the matrix time of 17 units)
            double work = c * (2.0 * 2 + 1.1 * (Tc - 2));
            if (wn == 1 && work < 34.0) work = 34.0;
            const double cost = (double)((wgs + slots - 1) / slots) * (work + 2.0);
            if (!have || cost < best_cost * 0.97) { *sp = cand; best_cost = cost; have = true; }
        }
    if (have && fat && sp->wn == 2 && sparse_plan_wn(Tc, 2, sp->q, &cand, true)) *sp = cand;
    return have;
}

// Shape-only part of the sparse launch's eligibility (shared with snn_debug_tile_shape, so that what bench.py reports is the plan that
// runs): the knob, channel counts, the (T, window) pairs the LIF epilogue has a form for, a tile plan with existing loop instances, the
// conv's XCD grouping and the LDS budget.  Kw = plane words per reduction row (conv: C_in / 32; linear: K / 32), Kc = 32-deep chunks.
// conv: T = 5 .. 16 with the window T - 1 (straight-line LIF instances; T = 4: built and measured 2.3 % slower than the dense launch).
// linear: any T whose window (T - 2, or T - 1 in spike-rate mode) fits the slot grid - 4 .. 24 planes on the 4 x 2 wave grid - with the
// general LIF epilogue outside the straight-line grid (round 5: T_det = 17 .. 26 and spike-rate mode used to take the all-dense launch).
struct SparseShape { SparsePlan sp; int n_tiles, n_blocks, grid, lds, xcd_cpx, xcd_contig, epi_general; };
static bool sparse_shape(bool conv, long long M, int Kw, int Kc, int Np, int T, int Tc, const SparseRoute& rt, SparseShape* out) {
    if (!knobs().sparse || rt.route == SNN_ROUTE_DENSE || Kw % 2 || Np % 64 || Kc * 32 > 65536 || M <= 0) return false;
    if (conv ? (T < 5 || T > 16 || Tc != T - 1) : (T < 5 || T > SNN_MAX_STEPS || (Tc != T - 2 && Tc != T - 1))) return false;
    if (!sparse_plan(Tc, &out->sp, conv ? 0 : M, Np / 64)) return false;
    const SparsePlan& sp = out->sp;
    out->n_tiles = cdiv(M, sp.pb);
    out->n_blocks = Np / 64;
    out->grid = out->n_tiles * out->n_blocks;                  // linear layers: plain order
    out->xcd_cpx = out->xcd_contig = 0;
    if (conv) {
        out->xcd_cpx = (out->n_blocks >= 4 && out->n_blocks % 2 == 0) ? out->n_blocks / 2 : 1;     // column blocks per XCD
        const int groups = out->n_blocks / out->xcd_cpx;                                             // XCD groups along N (2)
        if (8 % groups) return false;
        out->xcd_contig = cdiv(out->n_tiles, 8 / groups);
        out->grid = out->xcd_contig * out->xcd_cpx * 8;
    }
    out->lds = max((int)SP_LDS, Tc * sp.pb * SP_PITCH * 4);    // the ring, then the epilogue's tile image in the same bytes
    if (out->lds > 80 * 1024) return false;
    out->epi_general = !(T >= 5 && T <= 16 && Tc == T - (conv ? 1 : 2));
    return true;
}

// the sparse launch pair: compress the planes e_3 .., then the mixed dense / sparse contraction + LIF (conv: the RPN's shared 3x3
// convolution; !conv: a linear layer on word-major period planes - the detector's fc6).  `side` = sparse_side_bytes() of scratch.
// Returns 1 if the launches were enqueued (the layer is done), 0 if this configuration takes the dense launch, negative on error;
// 2 on the gated conv / fc6 route (rt.gated: compress + count, the decision, and this launch behind the gate - the caller enqueues the dense
// launch behind the same gate).  planes: weight planes of the launch (weight_planes).
// (Every eligibility check comes before the first launch: a configuration that ends on the dense kernel enqueues nothing here.)
// mode: SPARSE_RUN = compress + launch; SPARSE_QUERY = would it run? (nothing is enqueued); SPARSE_RUN_COMPRESSED = the caller's encoder has
// already written the compressed planes into `side` (RPN head: encode_block, snn_encode.h)
enum { SPARSE_RUN = 0, SPARSE_QUERY = 1, SPARSE_RUN_COMPRESSED = 2 };
static int gemm3_lif_sparse(const Gemm3Args& a, bool conv, void* side, size_t side_bytes, hipStream_t s, int mode, const SparseRoute& rt, int planes) {
    SparseShape sh;
    const int Kw = conv ? a.Cw : a.Kc;                        // plane words per row
    if (!side || !a.wm || !a.periods || a.t0 != 0 || a.p.v_leak != 0.0f || (float)(a.p.v_leak - a.p.v_th) > 0.0f || (!conv && !a.out_wm) ||
        !sparse_shape(conv, a.M, Kw, a.Kc, a.Np, a.T, a.Tc, rt, &sh))      // (the plan does not depend on spike counting; whether the LIF runs in registers does: sparse_plan_lif_regs below)
        return 0;
    const SparsePlan& sp = sh.sp;
    const long long P = a.M, Pe = (long long)a.a_step;
    if (side_bytes < sparse_side_bytes(P, Pe, Kw, a.T)) return 0;
    uint32_t* cmp = (uint32_t*)side;
    const unsigned long long cmp_bytes = (unsigned long long)(a.Tc - sp.nd) * (Kw / 2) * SP_A_ARR * Pe * 4;
    // (the kernel addresses both the raw and the compressed planes by 32-bit offsets from the raw planes)
    if ((const char*)cmp < (const char*)a.A || (unsigned long long)((const char*)cmp - (const char*)a.A) + cmp_bytes > 0xffffffffULL) return 0;
    if (mode == SPARSE_QUERY) return 1;
    const void* kern = sp.fat ? (conv ? (sp.wn == 1 ? (const void*)k_gemm_lif_sparse<true, 1, true> : (const void*)k_gemm_lif_sparse<true, 2, true>) : (const void*)k_gemm_lif_sparse<false, 2, true>)
                              : conv ? (const void*)k_gemm_lif_sparse<true, 1> : sp.wn == 2 ? (const void*)k_gemm_lif_sparse<false, 2> : (const void*)k_gemm_lif_sparse<false, 1>;
    if (planes == 1)
        kern = sp.fat ? (conv ? (sp.wn == 1 ? (const void*)k_gemm_lif_sparse1<true, 1, true> : (const void*)k_gemm_lif_sparse1<true, 2, true>) : (const void*)k_gemm_lif_sparse1<false, 2, true>)
                      : conv ? (const void*)k_gemm_lif_sparse1<true, 1> : sp.wn == 2 ? (const void*)k_gemm_lif_sparse1<false, 2> : (const void*)k_gemm_lif_sparse1<false, 1>;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, sh.lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    const bool gated = rt.gated;
    if (gated && (mode != SPARSE_RUN || !rt.stat || a.cnt_img || a.cnt_row)) return fail(-3, "conv / fc6 route: gated launch outside its plan (internal)");
    if (mode != SPARSE_RUN_COMPRESSED) {
        CompressArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.enc = a.A; ca.cmp = cmp; ca.Pe = (unsigned)Pe; ca.Cw = Kw; ca.nd = sp.nd;
        const dim3 gc(cdiv(Pe, 256), Kw / 2, a.Tc - sp.nd);
        if (gated) {                                  // the counting twin, then the decision: route_stat[2] is the gate word
            // hit counters: in the side buffer's per-position spike counters (spike-rate mode only, which is never gated), a cache line apart
            int* const slots = (int*)((char*)side + align_up((size_t)cmp_bytes, 256));
            const size_t room = align_up((size_t)P * 4, 256) + 256;                         // (sparse_side_bytes: what lies behind the compressed planes)
            const int nslots = (int)min((size_t)ROUTE_SLOTS_MAX, room / (ROUTE_SLOT_STRIDE * sizeof(int)));
            if (hipMemsetAsync(slots, 0, (size_t)nslots * ROUTE_SLOT_STRIDE * sizeof(int), s) != hipSuccess) return fail(-3, "hipMemsetAsync failed");
            // rows that count: the conv's padded row space; a linear layer's M rows (fc6: the RoIs - rows of a wider plane stride belong to no block)
            const long long n_rows = conv ? Pe : min(P, Pe);
            hipLaunchKernelGGL(k_compress_count_planes, gc, dim3(256), 0, s, ca, slots, nslots, (unsigned int)n_rows);
            SNN_CHECK_LAUNCH("k_compress_count_planes");
            hipLaunchKernelGGL(k_route_decide, dim3(1), dim3(64), 0, s, (int*)rt.stat, (const int*)slots, nslots,
                               (int)(cdiv(n_rows, 16) * (Kw / 2) * (a.Tc - sp.nd)), rt.crossover, -1);
            SNN_CHECK_LAUNCH("k_route_decide");
        } else {
            hipLaunchKernelGGL(k_compress_planes, gc, dim3(256), 0, s, ca);
            SNN_CHECK_LAUNCH("k_compress_planes");
        }
    }
    SparseConvArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.enc = a.A; sa.cmp = cmp; sa.wpk = a.wpk; sa.spk = a.spk;
    sa.tl = (unsigned long long*)((char*)side + sparse_side_bytes(P, Pe, Kw, a.T));      // (diagnostic builds only: behind the head's workspace)
    sa.plane_elems = a.plane_elems; sa.spk_stride = a.spk_stride; sa.Pe = (unsigned)Pe;
    sa.M = a.M; sa.Kc = a.Kc; sa.Np = a.Np; sa.Cw = Kw; sa.n_blocks = sh.n_blocks; sa.n_tiles = sh.n_tiles; sa.n_levels = a.n_levels;
    sa.T = a.T; sa.Tc = a.Tc; sa.nd = sp.nd; sa.pb = sp.pb; sa.q = sp.q; sa.out_split = a.out_split;
    memcpy(sa.mt_plane, sp.plane, sizeof(sa.mt_plane)); memcpy(sa.mt_j, sp.j, sizeof(sa.mt_j));
    memcpy(sa.w_nd, sp.w_nd, 8); memcpy(sa.w_ns, sp.w_ns, 8);
    sa.p = a.p;
    sa.epi_general = sh.epi_general;
    sa.lif_regs = sparse_plan_lif_regs(sp, conv, a.T, a.Tc, conv ? a.cnt_img != nullptr : a.cnt_row != nullptr, sh.epi_general) ? 1 : 0;
    memcpy(sa.div, a.div, sizeof(sa.div));
    memcpy(sa.lv, a.lv, sizeof(sa.lv));
    sa.xcd_cpx = sh.xcd_cpx; sa.xcd_contig = sh.xcd_contig;
    if (gated) { sa.gate = (const int*)rt.stat + 2; sa.gate_want = 0; }
    // spike-rate mode: the LIF epilogue adds its popcounts per row (RoI: straight into the caller's counters; conv: into per-position
    // counters behind the compressed planes, summed per (level, image) by a small launch afterwards)
    uint32_t* cnt_pos = nullptr;
    if (conv && a.cnt_img) {
        cnt_pos = (uint32_t*)((char*)side + align_up((size_t)cmp_bytes, 256));
        if (hipMemsetAsync(cnt_pos, 0, (size_t)P * 4, s) != hipSuccess) return fail(-3, "hipMemsetAsync failed");
    }
    sa.cnt_row = conv ? cnt_pos : a.cnt_row;
    if (knobs().debug_occ) {
        int v = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kern, sp.fat ? 256 : 512, sh.lds);
        fprintf(stderr, "k_gemm_lif_sparse<%d, %d, %d>: pb %d x Tc %d, q %d, lds %d B, %d work-groups per CU, grid %d\n", (int)conv, sp.wn, sp.fat, sp.pb, a.Tc, sp.q, sh.lds, v, sh.grid);
    }
    void* kargs[] = {(void*)&sa};
#ifdef SNN_PINGPONG
    // round 6: the FAT conv on 4 x 1 waves (T = 7 .. 9, LIF in registers) in its ping-pong form - one persistent work-group of 8 waves per CU
    // (snn_sparse_pp.h); same plan, same arguments, bit-identical planes
    const int pp_ns = a.Tc - sp.nd;
    if (planes == 3 && conv && !gated && sp.fat && sp.wn == 1 && sa.lif_regs && knobs().conv_pp && sp.nd == 2 && pp_ns >= 4 && pp_ns <= 5 && sa.Kc >= 4) {      // (T = 7, 8; at T = 9 the 8-wave work-group has no register left: 68 bytes of scratch)
        const void* kpp = pp_ns == 4 ? (const void*)k_conv_lif_pp<4> : (const void*)k_conv_lif_pp<5>;
        e = hipFuncSetAttribute(kpp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PP_LDS);
        if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 8) cus = 256;
        const int pairs = (sh.xcd_contig * sh.xcd_cpx + 1) / 2;
        const int grid = 8 * max(1, min(cus / 8, pairs));       // one work-group per CU (148 KB of LDS), a multiple of the 8 XCDs
        e = hipLaunchKernel(kpp, dim3(grid), dim3(512), kargs, PP_LDS, s);
        if (e != hipSuccess) return fail(-3, "k_conv_lif_pp launch failed: %s", hipGetErrorString(e));
        SNN_CHECK_LAUNCH("k_conv_lif_pp");
    } else
#endif
    {
    e = hipLaunchKernel(kern, dim3(sh.grid), dim3(sp.fat ? 256 : 512), kargs, sh.lds, s);
    if (e != hipSuccess) return fail(-3, "k_gemm_lif_sparse launch failed: %s", hipGetErrorString(e));
    SNN_CHECK_LAUNCH("k_gemm_lif_sparse");
    }
    if (cnt_pos) {
        PosCountArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.cnt_pos = cnt_pos; pa.cnt_img = a.cnt_img; pa.n_levels = a.n_levels; pa.max_n = a.max_n;
        memcpy(pa.lv, a.lv, sizeof(pa.lv));
        hipLaunchKernelGGL(k_sum_pos_counts, dim3(a.n_levels * a.max_n, POSCNT_CHUNKS), dim3(256), 0, s, pa);
        SNN_CHECK_LAUNCH("k_sum_pos_counts");
    }
    return gated ? 2 : 1;
}

int snn_debug_tile_shape(int conv, long long units, int k_in, int n_cols, int num_steps, int spike_rates, int layer, int32_t* out) {
    if (!out || units <= 0 || k_in <= 0 || n_cols <= 0 || num_steps < 1 || num_steps > SNN_MAX_STEPS) return fail(-1, "snn_debug_tile_shape: bad argument");
    snn_params p;
    memset(&p, 0, sizeof(p));
    p.v_th_lif = 0.1f;                                          // (only the sign of v_leak - v_th matters for the windows)
    int Tc;
    if (conv) Tc = lif_window_full_out(num_steps).n;
    else { const DetWindows w = det_windows(&p, num_steps, spike_rates != 0); Tc = layer == 7 ? w.fc7.n : w.fc6.n; }
    memset(out, 0, 12 * sizeof(int32_t));
    // the structured-sparse plan, where the launchers take it (period planes of the default parameters: conv, fc6)
    SparseShape sh;
    const int Kw = cdiv(k_in, 32), Np = cdiv(n_cols, 32) * 32;
    if (knobs().periods && (conv || layer != 7) && sparse_shape(conv != 0, units, Kw, conv ? 9 * Kw : Kw, Np, num_steps, Tc, SPARSE_ROUTE, &sh)) {      // (spike_rates only moves a linear layer's window: Tc above)
        const SparsePlan& sp = sh.sp;
        int slots = 0;
        for (int w = 0; w < (sp.fat ? 4 : 8) / sp.wn; ++w) slots += sp.w_nd[w] + sp.w_ns[w];
        out[0] = sp.fat ? (sp.wn == 1 ? SP_MT_FAT : conv ? SP_MT2_FAT_CONV : SP_MT2_FAT) : sp.wn == 1 ? SP_MT : SP_MT2; out[1] = sp.fat; out[2] = Tc * sp.pb; out[3] = sp.pb; out[4] = Tc; out[5] = sh.n_tiles * sh.n_blocks;
        out[6] = sh.n_blocks; out[7] = sp.wn; out[8] = 1; out[9] = sp.nd; out[10] = Tc - sp.nd; out[11] = slots;
        return 0;
    }
    const int wn = g3_wn(conv != 0), n_blocks = cdiv(Np, G3_BN(wn));
    const G3Tile tl = g3_pick_tile(wn, [&](int rows) { return g3_tile_ok(Tc, rows) ? (long long)cdiv(units, rows / Tc) * n_blocks : 0ll; });
    if (!tl.mt) return fail(-4, "snn_debug_tile_shape: %d steps do not fit a row tile", num_steps);
    const int pb = tl.rows / Tc;
    out[0] = tl.mt; out[1] = tl.n_short; out[2] = tl.rows; out[3] = pb; out[4] = Tc; out[5] = (int32_t)(cdiv(units, pb) * n_blocks);
    out[6] = n_blocks; out[7] = wn; out[8] = 0; out[9] = Tc; out[10] = 0; out[11] = 0;
    return 0;
}

// what the conv + LIF launcher is told beyond the layer itself (the defaults: a stage-level call on row-major planes)
struct ConvLifOpts {
    bool wm = false;                     // encoder planes word-major [T][Cw][rows]
    bool* out_split = nullptr;           // (in: wanted, out: done) spike planes in blocks of four words (Gemm3Args.out_split; T-in-tile kernels only)
    bool periods = false;                // the encoder wrote period planes
    void* sparse_side = nullptr;         // side buffers of the structured-sparse launch (sparse_side_bytes)
    size_t sparse_bytes = 0;
    // SPARSE_QUERY: returns 1 if this call would enqueue the structured-sparse launch pair, 0 if not - and enqueues nothing;
    // SPARSE_RUN_COMPRESSED: the encoder wrote the planes e_3 .. compressed (and not raw): anything but the sparse launch is an error
    int sparse_mode = SPARSE_RUN;
    SparseRoute route = SPARSE_ROUTE;
    int planes = 3;                      // weight planes (weight_planes)
};
static int conv3x3_lif_bf16x3_impl(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in,
                                   int C_out, int T, const snn_params* p, const uint16_t* w_packed, uint32_t* spk,
                                   size_t spk_stride, unsigned long long* counts, int max_n, snn_stream_t s, const ConvLifOpts& o) {
    const bool wm = o.wm, periods = o.periods;
    const int sparse_mode = o.sparse_mode;
    const bool want_split = o.out_split && *o.out_split;
    if (o.out_split) *o.out_split = false;
    if (!spk || !p) return fail(-1, "snn_conv3x3_lif_bf16x3: bad argument");
    Gemm3Args a;
    long long P;
    int rc = conv3_common("snn_conv3x3_lif_bf16x3", enc, enc_stride, lv, n_levels, C_in, C_out, T, w_packed, a, &P);
    if (rc) return rc;
    if (wm) {                                      // encoder planes [T][Cw][rows]: enc_stride = Cw * (rows per word plane)
        if (enc_stride % a.Cw) return fail(-1, "snn_conv3x3_lif_bf16x3: word-major planes need enc_stride %% Cw == 0");
        a.wm = 1; a.a_step = enc_stride / a.Cw;
        if (a.a_step * (unsigned long long)a.Cw > 0x7fffffffULL) return fail(-1, "snn_conv3x3_lif_bf16x3: plane too large");
    }
    a.M = (int)P; a.T = T; a.spk = spk; a.spk_stride = spk_stride; a.p = make_p(p, p->v_th_lif);
    // debug / A-B knob: SNN_BF16X3_LIF=reg forces the register-resident variant (the fallback for T > 64)
    const int wn = g3_wn(true);
    const StepWindow w = lif_window_full_out(T);   // the LI heads read the shared LIF's spikes of every step: currents of steps 0 .. T-2
    a.t0 = w.t0; a.Tc = w.n;
    const int Tc = w.n;
    G3Tile tl = {0, 0, 0};
    if (!knobs().bf16x3_lif_reg) {
        a.n_blocks = cdiv(a.Np, G3_BN(wn));
        tl = g3_pick_tile(wn, [&](int rows) { return g3_tile_ok(Tc, rows) ? (long long)cdiv(P, rows / Tc) * a.n_blocks : 0ll; });
    }
    if (!tl.mt) {                                     // register-fused fallback: counts from the planes afterwards
        if (sparse_mode == SPARSE_QUERY) return 0;
        if (periods) return fail(-4, "snn_conv3x3_lif_bf16x3: period planes need the T-in-tile kernel (T=%d does not fit a row tile)", T);
        a.n_blocks = cdiv(a.Np, G3_BN(2));
        rc = launch_gemm3(G3_CONV_LIF_REG, 4, 2, a, o.planes, (hipStream_t)s);
        if (rc || !counts) return rc;
        return count_spikes_per_image(lv, n_levels, cdiv(C_out, 32), T, spk, spk_stride, counts, max_n, (hipStream_t)s);
    }
    a.pb = tl.rows / Tc; a.n_short = tl.n_short;
    a.cnt_img = counts; a.max_n = max_n;
    if (want_split && a.Np % 128 == 0) { a.out_split = 1; *o.out_split = true; }
    if (periods && set_periods(a, "snn_conv3x3_lif_bf16x3")) return -1;
    // round 4: the sparse period planes on the structured-sparse matrix-core instruction (snn_sparse.h) where the configuration allows
    rc = gemm3_lif_sparse(a, true, o.sparse_side, o.sparse_bytes, (hipStream_t)s, sparse_mode, o.route, o.planes);
    if (sparse_mode == SPARSE_QUERY) return rc > 0 ? 1 : 0;
    if (rc < 0) return rc;
    g_last_conv_sparse = rc;
    if (rc == 1) return 0;
    if (rc == 2) { a.gate = (const int*)o.route.stat + 2; a.gate_want = 1; }      // the gated route: the dense launch on the raw period planes, behind the same word
    if (sparse_mode == SPARSE_RUN_COMPRESSED) return fail(-3, "snn_conv3x3_lif_bf16x3: the encoder wrote compressed planes but the conv takes the dense launch (internal)");
    return launch_gemm3(G3_CONV_LIF_TILE, tl.mt, wn, a, o.planes, (hipStream_t)s);
}

int snn_conv3x3_lif_bf16x3(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in,
                           int C_out, int T, const snn_params* p, const uint16_t* w_packed, uint32_t* spk,
                           size_t spk_stride, snn_stream_t s) {
    ConvLifOpts o;
    o.wm = knobs().stage_wm; o.periods = knobs().stage_periods && !knobs().bf16x3_lif_reg;
    return conv3x3_lif_bf16x3_impl(enc, enc_stride, lv, n_levels, C_in, C_out, T, p, w_packed, spk, spk_stride, nullptr, 0, s, o);
}

// spikes per (level, image) from finished planes: one launch per level (fallback of the register-fused conv variant only)
static int count_spikes_per_image(const snn_rpn_level* lv, int n_levels, int Cw, int T, const uint32_t* spk, size_t stride,
                                  unsigned long long* counts, int max_n, hipStream_t s) {
    long long pb = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int hw = lv[l].H * lv[l].W;
        hipLaunchKernelGGL(k_count_spikes, dim3(lv[l].N, max(1, min(256, hw * Cw / 2048))), dim3(256), 0, s, spk + (size_t)pb * Cw,
                           (unsigned long long)stride, T, hw * Cw, counts + (size_t)l * max_n);
        SNN_CHECK_LAUNCH("k_count_spikes");
        pb += (long long)lv[l].N * hw;
    }
    return 0;
}

int snn_spike_conv3x3_bf16x3(const uint32_t* enc, size_t enc_stride, const snn_rpn_level* lv, int n_levels, int C_in,
                             int C_out, int T, const uint16_t* w_packed, float* cur, int ldo, snn_stream_t s) {
    if (!cur || ldo < C_out) return fail(-1, "snn_spike_conv3x3_bf16x3: bad argument");
    Gemm3Args a;
    long long P;
    int rc = conv3_common("snn_spike_conv3x3_bf16x3", enc, enc_stride, lv, n_levels, C_in, C_out, T, w_packed, a, &P);
    if (rc) return rc;
    a.out = cur; a.ldo = ldo; a.M = (int)(T * P);
    const int wn = g3_wn(true);
    a.n_blocks = cdiv(a.Np, G3_BN(wn));
    const int mt = g3_pick_mt([&](int m) { return (long long)cdiv(a.M, g3_bm(wn, m)) * a.n_blocks; });
    return launch_gemm3(G3_CONV, mt, wn, a, 3, (hipStream_t)s);
}

static int check_T(int T, const char* who) {
    if (T < 1 || T > SNN_MAX_STEPS) return fail(-1, "%s: num_steps %d outside [1, %d]", who, T, SNN_MAX_STEPS);
    return 0;
}

// typed features (include/snn_hip.h): a known dtype (with or without the layout bit SNN_FEAT_NHWC), and a 16-byte aligned base pointer for
// the 16-bit types and for every channels-last map
static int check_feat(const void* ptr, int fdt, const char* who) {
    const int dt = fdt & ~SNN_FEAT_NHWC;
    if (dt != SNN_FEAT_F32 && dt != SNN_FEAT_F16 && dt != SNN_FEAT_BF16) return fail(-1, "%s: unknown feat_dtype %d", who, fdt);
    if ((fdt & SNN_FEAT_NHWC) && ptr && ((uintptr_t)ptr & 15)) return fail(-1, "%s: channels-last features must be 16-byte aligned", who);
    if (dt != SNN_FEAT_F32 && ptr && ((uintptr_t)ptr & 15)) return fail(-1, "%s: half-precision features must be 16-byte aligned", who);
    return 0;
}
// the row-fed entries: pooled rows have no layout
static int check_feat_rows(const void* ptr, int fdt, const char* who) {
    if (check_feat(nullptr, fdt, who)) return -1;
    if (fdt & SNN_FEAT_NHWC) return fail(-1, "%s: SNN_FEAT_NHWC on a row-fed entry (pooled rows have no layout)", who);
    return check_feat(ptr, fdt, who);
}

int snn_encode_nchw(const float* feat, int N, int C, int H, int W, int T, const snn_params* p,
                    uint32_t* planes, size_t plane_stride, snn_stream_t s) {
    return snn_encode_nchw_typed(feat, SNN_FEAT_F32, N, C, H, W, T, p, planes, plane_stride, s);
}

int snn_encode_nchw_typed(const void* feat_v, int fdt, int N, int C, int H, int W, int T, const snn_params* p,
                          uint32_t* planes, size_t plane_stride, snn_stream_t s) {
    const float* feat = (const float*)feat_v;
    if (!feat || !planes || !p || N <= 0 || C <= 0 || H <= 0 || W <= 0)
        return fail(-1, "snn_encode_nchw: bad argument");
    if (check_T(T, "snn_encode_nchw")) return -1;
    if (check_feat(feat_v, fdt, "snn_encode_nchw")) return -1;
    const bool nhwc = (fdt & SNN_FEAT_NHWC) != 0;
    if (nhwc && C % 32) return SNN_STATUS_NO_TYPED_KERNEL;       // (channels-last kernels: whole channel words only; nothing enqueued)
    const int Cw = cdiv(C, 32), HW = H * W;
    NeuronP np = make_p(p, p->v_th_enc);
    if (knobs().stage_periods && enc_zero_rest(np)) np.v_fire = ENC_FIRED;      // (tests / tools: period planes)
    const EncTh* eth;
    const int em = g_last_enc_mode = enc_mode(np, &eth);
    const dim3 g(cdiv(HW, ENC_PB), cdiv(Cw, ENC_WB), N);
    launch_picked(encode_nchw_kernel(em, fdt), g, dim3(256), nhwc ? ENC_NHWC_LDS_BYTES(T, feat_elem_bytes(fdt)) : ENC_LDS_BYTES(T), (hipStream_t)s, feat, C,
                  HW, Cw, T, np, *eth, planes, plane_stride);
    SNN_CHECK_LAUNCH("k_encode_nchw");
    return 0;
}

int snn_affine_act_nchw(const float* x, const float* scale, const float* bias, const float* residual, int N, int C, int HW,
                        int relu, float* y, snn_stream_t s) {
    if (!x || !scale || !bias || !y || N <= 0 || C <= 0 || HW <= 0) return fail(-1, "snn_affine_act_nchw: bad argument");
    if ((long long)N * C > 0x7fffffffLL / 64) return fail(-1, "snn_affine_act_nchw: too many planes");
    AffineArgs a;
    a.x = x; a.scale = scale; a.bias = bias; a.residual = residual; a.y = y; a.C = C; a.HW = HW; a.relu = relu;
    // ~8 float4 per thread and work-group round; small planes (deep levels) take one work-group each
    const int per_wg = 256 * 4 * 8;
    const long long planes = (long long)N * C;
    a.chunks = (int)max(1LL, min((long long)cdiv(HW, per_wg), max(1LL, (64LL * g3_slots()) / planes)));
    hipLaunchKernelGGL(k_affine_act, dim3((unsigned)(planes * a.chunks)), dim3(256), 0, (hipStream_t)s, a);
    SNN_CHECK_LAUNCH("k_affine_act");
    return 0;
}

// word-major planes [T][Dw][R] need D % 32 == 0 and 16-byte aligned rows (k_encode_rows_wm)
static bool encode_rows_wm_ok(const void* x, int D) { return D % 32 == 0 && ((uintptr_t)x & 15) == 0; }

// fdt != SNN_FEAT_F32: x points at 16-bit elements; typed kernels exist for word-major planes only (else SNN_STATUS_NO_TYPED_KERNEL, nothing enqueued)
static int encode_rows_impl(const void* x_v, int R, int D, int T, const snn_params* p, uint32_t* planes,
                            size_t plane_stride, bool wm, snn_stream_t s, bool periods = false, int fdt = SNN_FEAT_F32) {
    const float* x = (const float*)x_v;
    if (!x || !planes || !p || R <= 0 || D <= 0) return fail(-1, "snn_encode_rows: bad argument");
    if (fdt != SNN_FEAT_F32 && !wm) return SNN_STATUS_NO_TYPED_KERNEL;
    if (check_T(T, "snn_encode_rows")) return -1;
    const int Dw = cdiv(D, 32);
    const size_t total = (size_t)R * Dw * 32;
    NeuronP np = make_p(p, p->v_th_enc);
    if (periods) {
        if (!enc_zero_rest(np)) return fail(-1, "snn_encode_rows: period planes need zero rest / reset potentials");
        np.v_fire = ENC_FIRED;
    }
    const EncTh* eth;
    const int em = g_last_enc_mode = enc_mode(np, &eth);
    if (wm) {
        if (!encode_rows_wm_ok(x, D)) return fail(-1, "snn_encode_rows: word-major planes need D %% 32 == 0 and 16-byte aligned rows");
        const dim3 g(cdiv(Dw, 8), cdiv(R, 32));
        launch_picked(encode_rows_wm_kernel(em, fdt), g, dim3(256), 0, (hipStream_t)s, x, R, D, T, np, *eth, planes, plane_stride);
        SNN_CHECK_LAUNCH("k_encode_rows_wm");
        return 0;
    }
    if (D % 32 == 0 && ((uintptr_t)x & 15) == 0 && !knobs().enc_rows_ballot) {   // knob: "ballot" forces the element-per-lane kernel
        const size_t n_words = (size_t)R * Dw;
        const dim3 gw((unsigned)((n_words + 255) / 256));
        if (em == ENC_QUANT) hipLaunchKernelGGL(k_encode_rows_w<ENC_QUANT>, gw, dim3(256), 0, (hipStream_t)s, x, n_words, T, np, *eth, planes, plane_stride);
        else if (em == ENC_ZR) hipLaunchKernelGGL(k_encode_rows_w<ENC_ZR>, gw, dim3(256), 0, (hipStream_t)s, x, n_words, T, np, *eth, planes, plane_stride);
        else hipLaunchKernelGGL(k_encode_rows_w<ENC_GENERIC>, gw, dim3(256), 0, (hipStream_t)s, x, n_words, T, np, *eth, planes, plane_stride);
        SNN_CHECK_LAUNCH("k_encode_rows_w");
        return 0;
    }
    const dim3 grid((unsigned)((total + 256 * ENC_U - 1) / (256 * ENC_U)));
    if (em == ENC_QUANT) hipLaunchKernelGGL(k_encode_rows<ENC_QUANT>, grid, dim3(256), 0, (hipStream_t)s, x, R, D, Dw, T, np, *eth, planes, plane_stride);
    else if (em == ENC_ZR) hipLaunchKernelGGL(k_encode_rows<ENC_ZR>, grid, dim3(256), 0, (hipStream_t)s, x, R, D, Dw, T, np, *eth, planes, plane_stride);
    else hipLaunchKernelGGL(k_encode_rows<ENC_GENERIC>, grid, dim3(256), 0, (hipStream_t)s, x, R, D, Dw, T, np, *eth, planes, plane_stride);
    SNN_CHECK_LAUNCH("k_encode_rows");
    return 0;
}

int snn_encode_rows(const float* x, int R, int D, int T, const snn_params* p, uint32_t* planes,
                    size_t plane_stride, snn_stream_t s) {
    return encode_rows_impl(x, R, D, T, p, planes, plane_stride, false, s,
                            knobs().stage_periods && p && p->v_leak == 0.0f && p->v_reset == 0.0f && !knobs().enc_generic);
}


size_t snn_nms_workspace_bytes(int n) { return (size_t)n * cdiv(n, 64) * 8; }

int snn_nms_sorted(const float* boxes_sorted, const int* category_sorted, int n, float iou_threshold, int max_keep,
                   int* keep_out, int* n_keep_out, void* ws, size_t ws_bytes, snn_stream_t s) {
    if (!boxes_sorted || !keep_out || !n_keep_out || !ws || n <= 0 || max_keep <= 0)
        return fail(-1, "snn_nms_sorted: bad argument");
    const int words = cdiv(n, 64);
    if (words > 256) return fail(-1, "snn_nms_sorted: n=%d too large (max 16384)", n);
    if (ws_bytes < snn_nms_workspace_bytes(n)) return fail(-2, "snn_nms_sorted: workspace too small");
    unsigned long long* mask = (unsigned long long*)ws;
    NmsBatch nb;
    memset(&nb, 0, sizeof(nb));
    hipLaunchKernelGGL(k_nms_mask, dim3(words, words), dim3(64), 0, (hipStream_t)s, boxes_sorted, category_sorted, n,
                       iou_threshold, mask, words, nb);
    SNN_CHECK_LAUNCH("k_nms_mask");
    const int dbl = words <= 156 ? 1 : 0;                   // two chunk buffers fit the LDS up to n = 9984
    const size_t lds = (size_t)(1 + dbl) * 64 * words * 8;
    hipError_t e = hipFuncSetAttribute((const void*)k_nms_scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_nms_scan, dim3(1), dim3(256), lds, (hipStream_t)s, mask, n, words, max_keep, dbl, keep_out, n_keep_out, nb);
    SNN_CHECK_LAUNCH("k_nms_scan");
    return 0;
}

static int roi_align_encode_impl(const snn_roi_level* levels_host, int n_levels, int C, const float* rois, const int* roi_batch,
                                 const int* roi_level, int R, int T, const snn_params* p, uint32_t* planes,
                                 size_t plane_stride, float* pooled_dbg, bool wm, snn_stream_t s, bool periods = false, int fdt = SNN_FEAT_F32) {
    if (!levels_host || n_levels <= 0 || n_levels > 4 || C <= 0 || !rois || !roi_batch || !roi_level || R <= 0 || !p ||
        !planes)
        return fail(-1, "snn_roi_align_encode: bad argument");
    if (check_T(T, "snn_roi_align_encode")) return -1;
    for (int l = 0; l < n_levels; ++l)
        if (check_feat(levels_host[l].feat, fdt, "snn_roi_align_encode")) return -1;
    RoiArgs a;
    memset(&a, 0, sizeof(a));
    for (int l = 0; l < n_levels; ++l) {
        if (!levels_host[l].feat || levels_host[l].H <= 0 || levels_host[l].W <= 0)
            return fail(-1, "snn_roi_align_encode: bad level %d", l);
        a.lv[l].feat = levels_host[l].feat; a.lv[l].H = levels_host[l].H; a.lv[l].W = levels_host[l].W;
        a.lv[l].scale = levels_host[l].spatial_scale;
    }
    a.rois = rois; a.roi_batch = roi_batch; a.roi_level = roi_level; a.pooled = pooled_dbg; a.planes = planes;
    a.plane_stride = plane_stride; a.R = R; a.C = C; a.T = T; a.Dw = cdiv(C * 49, 32);
    a.p = make_p(p, p->v_th_enc);
    if (periods) {
        if (a.p.v_leak != 0.0f || a.p.v_reset != 0.0f) return fail(-1, "snn_roi_align_encode: period planes need zero rest / reset potentials");
        a.p.v_fire = ENC_FIRED;
        const EncTh* eth;
        if (enc_mode(a.p, &eth) == ENC_QUANT) { a.quant = 1; a.eth = *eth; }
    }
    g_last_enc_mode = a.quant ? ENC_QUANT : ENC_GENERIC;        // (the RoIAlign encoders have two forms: the table, or enc_step op for op)
    // word-major planes: the table-driven kernel (sample geometry once per wave and RoI) wherever its 8-byte tap pairs and 32-bit
    // element offsets are valid; SNN_ROI_TAB=0 keeps the per-element form (bit-identical planes, A/B + test switch)
    bool tab_ok = wm && knobs().roi_tab;
    for (int l = 0; l < n_levels && tab_ok; ++l)
        tab_ok = a.lv[l].W >= 2 && (long long)C * a.lv[l].H * a.lv[l].W < (1ll << 29);
    if (fdt != SNN_FEAT_F32 && !tab_ok) return SNN_STATUS_NO_TYPED_KERNEL;      // (typed form of the table kernel only; nothing enqueued)
    if (tab_ok) {
        // work-group = 16 RoIs (4 per wave) x 2 groups of 64 elements: small blocks keep the channel window of an XCD narrow (its
        // work-groups sweep the channels in step, snn_encode.h) - 77 % L2 hits against 21 % for 32 RoIs x 7 groups, 0.25 against
        // 0.30 ms; the per-element kernel: 0.35 ms (tools/time_roi_align.py, profiles/r3_roi_align.txt).  SNN_ROI_E / SNN_ROI_RW: A/B, tests
        a.E = knobs().roi_e > 0 ? knobs().roi_e : 2;
        a.RW = knobs().roi_rw > 0 ? knobs().roi_rw : 4;
        while ((size_t)T * 2 * a.E * 16 * a.RW > 49152 && a.E > 1) --a.E;
        a.n_rg = cdiv(R, 4 * a.RW);
        const int n_eblk = cdiv(a.Dw, 2 * a.E);
        const dim3 gt(cdiv(n_eblk, 8) * 8 * a.n_rg);
        const size_t lds = (size_t)T * 2 * a.E * 16 * a.RW;
        launch_picked(roi_align_encode_tab_kernel(fdt), gt, dim3(256), lds, (hipStream_t)s, a);
    } else if (wm) hipLaunchKernelGGL(k_roi_align_encode_wm, dim3(cdiv(a.Dw, 2), cdiv(R, 32)), dim3(256), 0, (hipStream_t)s, a);
    else hipLaunchKernelGGL(k_roi_align_encode, dim3(cdiv(a.Dw * 32, 256), R), dim3(256), 0, (hipStream_t)s, a);
    SNN_CHECK_LAUNCH("k_roi_align_encode");
    return 0;
}

int snn_roi_align_encode(const snn_roi_level* levels_host, int n_levels, int C, const float* rois, const int* roi_batch,
                         const int* roi_level, int R, int T, const snn_params* p, uint32_t* planes,
                         size_t plane_stride, float* pooled_dbg, snn_stream_t s) {
    return snn_roi_align_encode_typed(levels_host, SNN_FEAT_F32, n_levels, C, rois, roi_batch, roi_level, R, T, p, planes, plane_stride, pooled_dbg, s);
}

int snn_roi_align_encode_typed(const snn_roi_level* levels_host, int fdt, int n_levels, int C, const float* rois, const int* roi_batch,
                               const int* roi_level, int R, int T, const snn_params* p, uint32_t* planes,
                               size_t plane_stride, float* pooled_dbg, snn_stream_t s) {
    if (fdt & SNN_FEAT_NHWC)                                    // (flatten-order planes are not built for channels-last maps; nothing enqueued)
        return check_feat(nullptr, fdt, "snn_roi_align_encode") ? -1 : SNN_STATUS_NO_TYPED_KERNEL;
    // (SNN_STAGE_PLANES=wm, tests / tools: the planes come back word-major [T][Dw][R] - the layout and the kernels the fused head uses)
    return roi_align_encode_impl(levels_host, n_levels, C, rois, roi_batch, roi_level, R, T, p, planes, plane_stride, pooled_dbg,
                                 knobs().stage_wm, s, knobs().stage_periods && p && p->v_leak == 0.0f && p->v_reset == 0.0f, fdt);
}

// shared by snn_conv3x3_lif (one level) and snn_rpn_head_forward (all levels in one launch)
static int launch_conv(const snn_rpn_level* lv, int n_levels, int C_in, int C_out, int T, const snn_params* p,
                       const uint32_t* enc, size_t enc_stride, const float* wpk, uint32_t* spk,
                       size_t spk_stride, unsigned long long* counts, int max_n, float* dbg_cur,
                       hipStream_t s) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.enc = enc; a.spk = spk; a.wpk = wpk; a.counts = counts; a.dbg_cur = dbg_cur;
    a.enc_stride = enc_stride; a.spk_stride = spk_stride;
    a.Cw = cdiv(C_in, 32); a.Nw = cdiv(C_out, 32); a.T = T; a.n_levels = n_levels; a.max_n = max_n;
    a.Tc = dbg_cur ? T : lif_window_full_out(T).n;          // (the test hook dumps the currents of every step)
    a.p = make_p(p, p->v_th_lif);
    int tiles = 0, pos = 0;
    for (int l = 0; l < n_levels; ++l) {
        ConvLevelDev& d = a.lv[l];
        d.pos_base = pos; d.N = lv[l].N; d.H = lv[l].H; d.W = lv[l].W;
        d.tiles_x = cdiv(lv[l].W, CONV_PW);
        d.tiles_per_img = d.tiles_x * cdiv(lv[l].H, CONV_PH);
        d.tile_begin = tiles;
        tiles += d.tiles_per_img * lv[l].N;
        pos += lv[l].N * lv[l].H * lv[l].W;
    }
    if (a.Cw > CONV_MAX_CW) return fail(-1, "conv3x3_lif: C_in=%d > %d not supported", C_in, CONV_MAX_CW * 32);
    const size_t lds = (size_t)CONV_HALO * (a.Cw * 32 + CONV_APAD) * 4;
    auto kern = dbg_cur ? k_conv3x3_lif<true> : k_conv3x3_lif<false>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(kern, dim3(tiles, cdiv(a.Nw, CONV_BNT)), dim3(512), lds, s, a);
    SNN_CHECK_LAUNCH("k_conv3x3_lif");
    return 0;
}

int snn_conv3x3_lif(const uint32_t* enc, size_t enc_stride, int N, int C_in, int C_out, int H, int W, int T,
                    const snn_params* p, const float* w_packed, uint32_t* spk, size_t spk_stride,
                    unsigned long long* counts, float* dbg_cur, snn_stream_t s) {
    if (!enc || !spk || !w_packed || !p || N <= 0 || C_in <= 0 || C_out <= 0 || H <= 0 || W <= 0)
        return fail(-1, "snn_conv3x3_lif: bad argument");
    if (check_T(T, "snn_conv3x3_lif")) return -1;
    snn_rpn_level lv; lv.feat = nullptr; lv.N = N; lv.H = H; lv.W = W; lv.reserved = 0;
    return launch_conv(&lv, 1, C_in, C_out, T, p, enc, enc_stride, w_packed, spk, spk_stride, counts, N, dbg_cur,
                       (hipStream_t)s);
}

int snn_spike_gemm(const uint32_t* a_rows, int M, int K, int N, const float* w_packed, float* cur, int ldo,
                   snn_stream_t s) {
    if (!a_rows || !w_packed || !cur || M <= 0 || K <= 0 || N <= 0 || ldo < N)
        return fail(-1, "snn_spike_gemm: bad argument");
    GemmArgs a;
    a.A = a_rows; a.wpk = w_packed; a.out = cur; a.M = M; a.Kw = cdiv(K, 32); a.Nw = cdiv(N, 32); a.ldo = ldo; a.pad = 0;
    // 128 rows x 256 columns per work-group: 8 waves, each 128 x 32
    constexpr int MT = 4;
    a.n_blocks = cdiv(a.Nw, 8);
    auto kern = k_spike_gemm<MT>;
    hipLaunchKernelGGL(kern, dim3(cdiv(M, MT * 32) * a.n_blocks), dim3(512), 2 * 128 * GEMM_AST * 4, (hipStream_t)s, a);
    SNN_CHECK_LAUNCH("k_spike_gemm");
    return 0;
}

// cur = the currents of the steps w.t0 .. w.t0+w.n-1, [w.n][R][ldc]
static int lif_scan_window(const float* cur, int T, StepWindow w, int R, int N, int ldc, const snn_params* p, uint32_t* spk,
                           size_t spk_stride, uint32_t* row_counts, snn_stream_t s) {
    const int Nw = cdiv(N, 32);
    const size_t total = (size_t)R * Nw * 32;
    hipLaunchKernelGGL(k_lif_scan, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s, cur, T, w.t0, w.n, R, N,
                       Nw, ldc, make_p(p, p->v_th_lif), spk, spk_stride, row_counts);
    SNN_CHECK_LAUNCH("k_lif_scan");
    return 0;
}

int snn_lif_scan(const float* cur, int T, int R, int N, int ldc, const snn_params* p, uint32_t* spk,
                 size_t spk_stride, uint32_t* row_counts, snn_stream_t s) {
    if (!cur || !spk || !p || R <= 0 || N <= 0 || ldc < N) return fail(-1, "snn_lif_scan: bad argument");
    if (check_T(T, "snn_lif_scan")) return -1;
    return lif_scan_window(cur, T, lif_window_all(T), R, N, ldc, p, spk, spk_stride, row_counts, s);
}

// all of W as three bf16 planes stays resident in LDS (k_li_heads_mfma)
static bool li_heads_fits(int Kw, int NOp) { return (size_t)Kw * 3 * NOp * 64 <= 96 * 1024; }

// the launch of snn_li_heads that can read spike planes in blocks of four words (k_li_heads_mfma with W resident, 8 words per row)
static bool li_heads_reads_split(int K, int NA, int NB) {
    const int Kw = cdiv(K, 32), NOp = cdiv(NA + NB, 16) * 16;
    const int force = knobs().li_heads;
    return Kw == 8 && NOp <= 64 && li_heads_fits(Kw, NOp) && (force == 0 || force == 2);
}

// which kernel takes columns col0 .. col0 + NOp - 1 of the heads: 3 k_li_heads_ksplit, 2 k_li_heads_mfma, 1 k_li_heads (fp32 VALU)
static int li_heads_kind(int Kw, int NOp, int force) {
    // matrix-core kernel where all of W (as three bf16 planes) stays resident in LDS; the streamed form is latency
    // bound on small row counts (detector heads: 164 us against 88 us for the VALU kernel) and only runs when forced
    const bool fits = li_heads_fits(Kw, NOp);
    if (NOp <= 64 && Kw >= 4 && (force ? force == 3 : !fits)) return 3;
    if (NOp <= 64 && (force ? force == 2 : fits)) return 2;
    return 1;
}

// what the launches of one heads call (single- or several-readout) share
struct LiHeadsCall {
    const uint32_t* spk; size_t spk_stride;
    const float* w;
    int M, Kw, NA, NB;
    bool half_split;
    int ldw;                      // columns of a row of the packed matrix
    int force;                    // debug / A-B knob: 1 "valu" forces the fp32 VALU kernel, 2 "mfma", 3 "ksplit"; SNN_PRECISION_F32_STRICT always takes the VALU kernel
    int step;                     // columns per launch
};
static int li_heads_call(LiHeadsCall* c, const uint32_t* spk, size_t spk_stride, int M, int K, const float* w_heads_packed, int NA, int NB,
                         const snn_params* p, bool half_split) {
    // (covers more than 64 outputs per row as well: the split planes go with one launch)
    if (half_split && !li_heads_reads_split(K, NA, NB)) return fail(-1, "snn_li_heads: split planes need the resident matrix-core kernel");
    c->spk = spk; c->spk_stride = spk_stride; c->w = w_heads_packed; c->M = M; c->Kw = cdiv(K, 32); c->NA = NA; c->NB = NB;
    c->half_split = half_split;
    c->ldw = cdiv(NA + NB, 16) * 16;
    c->force = (p && p->precision == SNN_PRECISION_F32_STRICT) ? 1 : knobs().li_heads;      // (a null p: the caller's argument check refuses it)
    // More than 64 outputs per row (num_classes >= 13: 5 K outputs - pascal 24, coco 91 of the reference's configs): one launch per
    // block of 64 columns (matrix-core kernels; the VALU kernel takes 256); every launch reads all spike planes, which is the small
    // operand here.  (Until round 4: the VALU kernel up to 256 outputs, an error beyond.)
    c->step = c->force == 1 ? 256 : 64;
    return 0;
}

// a matrix-core launch (kind 3 / 2, single- or several-readout kernel) over columns col0 .. col0 + NOp - 1: its arguments but for T and
// kap, which are the caller's; returns its LDS bytes
static size_t li_heads_plan(int kind, const LiHeadsCall& c, float* out_a, float* out_b, float* sum_a, float* sum_b, int col0, int NOp,
                            LiHeadsArgs* a) {
    memset(a, 0, sizeof(*a));
    a->spk = c.spk; a->spk_stride = c.spk_stride; a->wT = c.w; a->out_a = out_a; a->out_b = out_b; a->sum_a = sum_a; a->sum_b = sum_b;
    a->M = c.M; a->Kw = c.Kw; a->NOp = NOp; a->NA = c.NA; a->NB = c.NB; a->ldw = c.ldw; a->col0 = col0;
    if (kind == 3) return G3_LUT_BYTES + (size_t)4 * 2 * (NOp / 16) * 64 * 16;
    a->n_groups = cdiv(c.M, 64);
    a->half_split = c.half_split;
    a->resident = li_heads_fits(c.Kw, NOp);
    return G3_LUT_BYTES + (size_t)(a->resident ? c.Kw : 2) * 3 * NOp * 64;
}

// work-groups of a k_li_heads_mfma / k_li_heads_mfma_ro launch.  Resident weights: persistent work-groups (staging once per work-group),
// exactly as many as are co-resident (k_li_heads_mfma: registers allow 3 per SIMD: a grid of 4 per CU ran a third of them as a second,
// mostly empty round); streamed: one row group each.  per_cu: the co-resident work-groups per CU if the caller keeps them (the plain
// launch, which is on the timed path), else 0: asked here, `fallback` where the query fails.
static int li_heads_grid(const LiHeadsArgs& a, const void* kern, size_t lds, int per_cu, int fallback) {
    if (!a.resident) return a.n_groups;
    if (per_cu <= 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu <= 0)) per_cu = fallback;
    return min(a.n_groups, per_cu * g3_slots());
}

// columns col0 .. col0 + NOp - 1 (NOp a multiple of 16, <= 64 for the matrix-core kernels, <= 256 for the VALU kernel) of the heads
static int li_heads_cols(const LiHeadsCall& c, int T, const Kappa& kap, float* out_a, float* out_b, float* sum_a, float* sum_b, int col0,
                         int NOp, hipStream_t s) {
    const int kind = li_heads_kind(c.Kw, NOp, c.force), nt = NOp / 16, M = c.M;
    if (kind != 1) {
        LiHeadsArgs a;
        const size_t lds = li_heads_plan(kind, c, out_a, out_b, sum_a, sum_b, col0, NOp, &a);
        a.T = T; a.kap = kap;
        void* kargs[] = {(void*)&a};
        // W too large for LDS: one work-group per 16 rows, the reduction split over its 4 waves ("ksplit" forces it)
        if (kind == 3) {
            const void* kern = nt == 1 ? (const void*)k_li_heads_ksplit<1> : nt == 2 ? (const void*)k_li_heads_ksplit<2>
                             : nt == 3 ? (const void*)k_li_heads_ksplit<3> : (const void*)k_li_heads_ksplit<4>;
            hipError_t e = hipLaunchKernel(kern, dim3(cdiv(M, 16)), dim3(256), kargs, lds, s);
            if (e != hipSuccess) return fail(-3, "k_li_heads_ksplit launch failed: %s", hipGetErrorString(e));
            SNN_CHECK_LAUNCH("k_li_heads_ksplit");
            return 0;
        }
        const void* kern = nt == 1 ? (const void*)k_li_heads_mfma<1> : nt == 2 ? (const void*)k_li_heads_mfma<2>
                         : nt == 3 ? (const void*)k_li_heads_mfma<3> : (const void*)k_li_heads_mfma<4>;
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
        static int per_cu_cache[5] = {0, 0, 0, 0, 0};           // by column tiles; the LDS size of the resident form follows from them and Kw
        static size_t per_cu_lds[5] = {0, 0, 0, 0, 0};
        if (per_cu_cache[nt] == 0 || per_cu_lds[nt] != lds) {
            int v = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kern, 256, lds) != hipSuccess || v <= 0) v = 3;
            per_cu_cache[nt] = v; per_cu_lds[nt] = lds;
        }
        e = hipLaunchKernel(kern, dim3(li_heads_grid(a, kern, lds, per_cu_cache[nt], 3)), dim3(256), kargs, lds, s);
        if (e != hipSuccess) return fail(-3, "k_li_heads_mfma launch failed: %s", hipGetErrorString(e));
        SNN_CHECK_LAUNCH("k_li_heads_mfma");
        return 0;
    }
    // rows per block: as many as 256 threads can own (row, 4-output group) pairs for
    const int jg = NOp / 4;
    const int rb = (256 / jg >= 64) ? 64 : (256 / jg >= 32) ? 32 : (256 / jg >= 16) ? 16 : (256 / jg >= 8) ? 8 : 4;
    const size_t lds = ((size_t)(sum_a ? 2 : 1) * rb * (HEADS_KS + 4) + (size_t)HEADS_KS * NOp) * 4;
    if (lds > 160 * 1024) return fail(-1, "snn_li_heads: LDS budget exceeded (NOp=%d)", NOp);
    void (*kern)(const uint32_t*, size_t, int, int, int, const float*, int, int, int, int, int, const Kappa, float*, float*,
                 float*, float*) = rb == 64 ? k_li_heads<64> : rb == 32 ? k_li_heads<32> : rb == 16 ? k_li_heads<16>
                                             : rb == 8 ? k_li_heads<8> : k_li_heads<4>;
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(kern, dim3(cdiv(M, rb)), dim3(256), lds, s, c.spk, c.spk_stride, T, M, c.Kw,
                       c.w, NOp, c.ldw, col0, c.NA, c.NB, kap, out_a, out_b, sum_a, sum_b);
    SNN_CHECK_LAUNCH("k_li_heads");
    return 0;
}

static int li_heads_impl(const uint32_t* spk, size_t spk_stride, int T, int M, int K, const float* w_heads_packed,
                         int NA, int NB, const snn_params* p, float* out_a, float* out_b, float* sum_a, float* sum_b,
                         bool half_split, snn_stream_t s) {
    LiHeadsCall c;
    if (li_heads_call(&c, spk, spk_stride, M, K, w_heads_packed, NA, NB, p, half_split)) return -1;
    if (!spk || !w_heads_packed || !p || !out_a || !out_b || M <= 0 || K <= 0 || NA <= 0 || NB <= 0)
        return fail(-1, "snn_li_heads: bad argument");
    if ((sum_a == nullptr) != (sum_b == nullptr)) return fail(-1, "snn_li_heads: sum_a and sum_b go together");
    if (check_T(T, "snn_li_heads")) return -1;
    Kappa kap;
    li_kappa(p, T, &kap);
    for (int col0 = 0; col0 < c.ldw; col0 += c.step) {
        const int rc = li_heads_cols(c, T, kap, out_a, out_b, sum_a, sum_b, col0, min(c.step, c.ldw - col0), (hipStream_t)s);
        if (rc) return rc;
    }
    return 0;
}

int snn_li_heads(const uint32_t* spk, size_t spk_stride, int T, int M, int K, const float* w_heads_packed,
                 int NA, int NB, const snn_params* p, float* out_a, float* out_b, float* sum_a, float* sum_b,
                 snn_stream_t s) {
    return li_heads_impl(spk, spk_stride, T, M, K, w_heads_packed, NA, NB, p, out_a, out_b, sum_a, sum_b, false, s);
}

// ---- any-time readouts (time-step sweeps) ----------------------------------------------------------
// a readout set: T'_0 < ... < T'_{n-1} in [1, SNN_MAX_STEPS]; the pass runs at T = T'_{n-1}
static int check_steps(const int* steps, int n, const char* who) {
    if (!steps) return fail(-1, "%s: null step list", who);
    if (n < 1 || n > SNN_MAX_STEPS) return fail(-1, "%s: %d steps in the readout list (1 .. %d)", who, n, SNN_MAX_STEPS);
    for (int j = 0; j < n; ++j) {
        if (steps[j] < 1 || steps[j] > SNN_MAX_STEPS) return fail(-1, "%s: steps[%d] = %d outside [1, %d]", who, j, steps[j], SNN_MAX_STEPS);
        if (j && steps[j] <= steps[j - 1]) return fail(-1, "%s: steps must be strictly increasing (steps[%d] = %d after %d)", who, j, steps[j], steps[j - 1]);
    }
    return 0;
}
static StepList step_list(const int* steps, int n) {
    StepList st;
    memset(&st, 0, sizeof(st));
    st.n = n;
    for (int j = 0; j < n; ++j) st.steps[j] = steps[j];
    return st;
}

// outputs [n][M][NA] / [n][M][NB] (sums alike): readout j = the single-readout heads at T'_j on the first T'_j planes, bit for bit.
// Matrix-core kernels: one launch per block of up to RB readouts, from the last block down (the first launch covers the longest
// readouts, a remainder block the shortest), each over the steps its last readout needs.  fp32 VALU kernel: one launch per readout.
extern "C++" template <int NT, bool S>
static int li_heads_ro_launch(bool ksplit, const LiHeadsArgs& base, const snn_params* p, const int* steps, int n, unsigned long long st_a,
                              unsigned long long st_b, size_t lds, hipStream_t s) {
    constexpr int RB = LIH_RO_B(NT, S);
    const void* kern = ksplit ? (const void*)k_li_heads_ksplit_ro<NT, RB, S> : (const void*)k_li_heads_mfma_ro<NT, RB, S>;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    const int grid = ksplit ? cdiv(base.M, 16) : li_heads_grid(base, kern, lds, 0, 1);
    for (int hi = n; hi > 0; hi -= RB) {
        const int lo = max(0, hi - RB);
        LiReadoutArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.h = base;
        ra.h.T = steps[hi - 1];
        ra.h.out_a = base.out_a + lo * st_a; ra.h.out_b = base.out_b + lo * st_b;
        if (S) { ra.h.sum_a = base.sum_a + lo * st_a; ra.h.sum_b = base.sum_b + lo * st_b; }
        ra.ro_stride_a = st_a; ra.ro_stride_b = st_b;
        ra.n_ro = hi - lo;
        for (int j = 0; j < hi - lo; ++j) { ra.steps[j] = steps[lo + j]; li_kappa(p, steps[lo + j], &ra.kap[j]); }
        void* kargs[] = {(void*)&ra};
        e = hipLaunchKernel(kern, dim3(grid), dim3(256), kargs, lds, s);
        if (e != hipSuccess) return fail(-3, "%s launch failed: %s", ksplit ? "k_li_heads_ksplit_ro" : "k_li_heads_mfma_ro", hipGetErrorString(e));
        SNN_CHECK_LAUNCH(ksplit ? "k_li_heads_ksplit_ro" : "k_li_heads_mfma_ro");
    }
    return 0;
}

static int li_heads_readouts_impl(const uint32_t* spk, size_t spk_stride, const int* steps, int n, int M, int K, const float* w_heads_packed,
                                  int NA, int NB, const snn_params* p, float* out_a, float* out_b, float* sum_a, float* sum_b,
                                  bool half_split, snn_stream_t stream) {
    LiHeadsCall c;
    if (li_heads_call(&c, spk, spk_stride, M, K, w_heads_packed, NA, NB, p, half_split)) return -1;
    const unsigned long long st_a = (unsigned long long)M * NA, st_b = (unsigned long long)M * NB;
    hipStream_t s = (hipStream_t)stream;
    // by column tiles and time sums
    static int (*const ro_launch[4][2])(bool, const LiHeadsArgs&, const snn_params*, const int*, int, unsigned long long, unsigned long long, size_t,
                                        hipStream_t) = {{li_heads_ro_launch<1, false>, li_heads_ro_launch<1, true>},
                                                        {li_heads_ro_launch<2, false>, li_heads_ro_launch<2, true>},
                                                        {li_heads_ro_launch<3, false>, li_heads_ro_launch<3, true>},
                                                        {li_heads_ro_launch<4, false>, li_heads_ro_launch<4, true>}};
    for (int col0 = 0; col0 < c.ldw; col0 += c.step) {
        const int NOp = min(c.step, c.ldw - col0);
        const int kind = li_heads_kind(c.Kw, NOp, c.force);
        if (kind == 1) {                                       // the fp32 VALU kernel (f32_strict): one launch per readout
            for (int j = 0; j < n; ++j) {
                Kappa kap;
                li_kappa(p, steps[j], &kap);
                const int rc = li_heads_cols(c, steps[j], kap, out_a + j * st_a, out_b + j * st_b, sum_a ? sum_a + j * st_a : nullptr,
                                             sum_b ? sum_b + j * st_b : nullptr, col0, NOp, s);
                if (rc) return rc;
            }
            continue;
        }
        LiHeadsArgs a;
        const size_t lds = li_heads_plan(kind, c, out_a, out_b, sum_a, sum_b, col0, NOp, &a);
        const int rc = ro_launch[NOp / 16 - 1][sum_a != nullptr](kind == 3, a, p, steps, n, st_a, st_b, lds, s);
        if (rc) return rc;
    }
    return 0;
}

int snn_li_heads_readouts(const uint32_t* spk, size_t spk_stride, const int* steps, int n_steps, int M, int K, const float* w_heads_packed,
                          int NA, int NB, const snn_params* p, float* out_a, float* out_b, float* sum_a, float* sum_b, snn_stream_t s) {
    if (check_steps(steps, n_steps, "snn_li_heads_readouts")) return -1;
    if (!spk || !w_heads_packed || !p || !out_a || !out_b || M <= 0 || K <= 0 || NA <= 0 || NB <= 0)
        return fail(-1, "snn_li_heads_readouts: bad argument");
    if ((sum_a == nullptr) != (sum_b == nullptr)) return fail(-1, "snn_li_heads_readouts: sum_a and sum_b go together");
    return li_heads_readouts_impl(spk, spk_stride, steps, n_steps, M, K, w_heads_packed, NA, NB, p, out_a, out_b, sum_a, sum_b, false, s);
}

// ---- whole heads ---------------------------------------------------------------------------------
static long long rpn_positions(const snn_rpn_level* lv, int n_levels, int* max_n) {
    long long P = 0; int mn = 0;
    for (int l = 0; l < n_levels; ++l) { P += (long long)lv[l].N * lv[l].H * lv[l].W; mn = lv[l].N > mn ? lv[l].N : mn; }
    if (max_n) *max_n = mn;
    return P;
}

static long long rpn_positions_padded(const snn_rpn_level* lv, int n_levels) {
    long long P = 0;
    for (int l = 0; l < n_levels; ++l) P += (long long)lv[l].N * (lv[l].H + 2) * (lv[l].W + 2);
    return P;
}

// Pe = rows of an encoder plane (positions; with the zero halo for the mxfp6 path)
// bytes behind the two plane sets for the structured-sparse conv (snn_sparse.h): the compressed planes, primary + secondary (SP_A_ARR
// dwords per row and 64 k; planes e_3 .. of at most T - 1 current planes) and the per-position spike counters of spike-rate mode
static size_t sparse_side_bytes(long long P, long long Pe, int Kw, int T) {     // Kw = 32-bit words per row of a plane
    // (+ one spike counter per position for the conv's spike-rate mode)
    return align_up((size_t)max(T - 3, 1) * cdiv(Kw, 2) * SP_A_ARR * (size_t)Pe * 4, 256) + align_up((size_t)P * 4, 256) + 256;
}
static size_t rpn_sparse_bytes(long long P, long long Pe, int C, int T) { return sparse_side_bytes(P, Pe, cdiv(C, 32), T); }
static void rpn_ws_layout(long long P, long long Pe, int C, int T, int precision, size_t* o_spk, size_t* o_cur, size_t* o_cnt,
                          size_t* total) {
    const size_t plane = align_up((size_t)T * (Pe > P ? Pe : P) * cdiv(C, 32) * 4, 256);
    *o_spk = plane;
    *o_cur = 2 * plane;                                   // bf16x3: the sparse conv's side buffers (rpn_sparse_bytes); else unused
    const size_t cur = precision == SNN_PRECISION_BF16X3 ? rpn_sparse_bytes(P, Pe > P ? Pe : P, C, T) : 0;
    *o_cnt = 2 * plane + cur;
    const size_t cnt = 0;
    *total = 2 * plane + cur + cnt;
}

size_t snn_rpn_head_workspace_bytes(const snn_rpn_level* lv, int n_levels, int C, int A, int T, int precision) {
    (void)A;
    if (!lv || n_levels <= 0 || n_levels > SNN_MAX_LEVELS || C <= 0 || T < 1) return 0;
    size_t a, b, c, tot;
    rpn_ws_layout(rpn_positions(lv, n_levels, nullptr), prec_family(precision) != SNN_PRECISION_F32 ? rpn_positions_padded(lv, n_levels) : 0,
                  C, T, precision == SNN_PRECISION_BF16 ? (int)SNN_PRECISION_BF16X3 : precision, &a, &b, &c, &tot);
    return tot;
}

// everything an RPN head pass is told, whichever exported entry it came through (the entries check what is theirs alone - the step list, the
// pairs that go together, the route - fill one of these and run it)
struct RpnCall {
    const snn_rpn_level* lv; int fdt, n_levels, C, A, T;      // the feed: typed feature maps per level; T: the pass's last step
    const snn_params* p;
    const void* w_shared_packed; const float* w_heads_packed;
    float *out_logits, *out_bbox; unsigned long long* spike_counts; float *sum_logits, *sum_bbox;
    void* ws; size_t ws_bytes; snn_stream_t stream;
    int stage_mask;
    // any-time readouts (snn_rpn_head_forward_readouts): outputs [n][P][A] / [n][P][4A], counts [n][n_levels][max_n]; null: one readout at T
    const int* steps; int n_steps;
    SparseRoute route;                                         // of the conv; .gated is the plan's to decide, not the entry's
    const char* who;                                           // the name in messages
};
static RpnCall rpn_call(const snn_rpn_level* lv, int fdt, int n_levels, int C, int A, int T, const snn_params* p, const void* w_shared_packed,
                        const float* w_heads_packed, float* out_logits, float* out_bbox, unsigned long long* spike_counts, float* sum_logits,
                        float* sum_bbox, void* ws, size_t ws_bytes, snn_stream_t stream) {
    return RpnCall{lv, fdt, n_levels, C, A, T, p, w_shared_packed, w_heads_packed, out_logits, out_bbox, spike_counts, sum_logits, sum_bbox,
                   ws, ws_bytes, stream, SNN_STAGE_ALL, nullptr, 0, SPARSE_ROUTE, "snn_rpn_head_forward"};
}

// bf16x3 conv -> LI heads: spike planes in blocks of four words when the heads kernel that will run reads them so (C = 256).
// Decided up front, so that a stage-by-stage caller (bench.py's kernel breakdown) sees the same launches; a T that does
// not fit a row tile runs the register-fused conv, which writes plain rows: then the heads read plain rows
static bool rpn_planes_split(const snn_params* p, int C, int A, int T) {
    return prec_family(p) == SNN_PRECISION_BF16X3 && !knobs().spk_rows && li_heads_reads_split(C, A, 4 * A) &&
           !knobs().bf16x3_lif_reg && cdiv(C, 32) * 32 % 128 == 0 &&
           g3_some_tile_ok(lif_window_full_out(T).n, true);
}
// where an RPN pass leaves the shared LIF's spike planes (snn_rpn_head_planes_view; the pass reads its own layout from here)
static void rpn_planes_view(const snn_params* p, long long P, int C, int A, int T, size_t o_spk, snn_planes_view* v) {
    v->offset_bytes = o_spk; v->step_stride_words = (uint64_t)P * cdiv(C, 32); v->rows = P; v->words = cdiv(C, 32);
    v->layout = rpn_planes_split(p, C, A, T) ? SNN_PLANES_SPLIT4 : SNN_PLANES_ROWS;
    v->steps_formed = min(T, lif_window_full_out(T).n + 1);      // currents of steps 0 .. n - 1 form the spikes of steps 0 .. n
    v->reserved = 0;
}

// the RPN head: encoder, conv + LIF, then the LI heads - one readout at T (the plain forward), or the readout set with its spike counts
static int rpn_head_run(const RpnCall& c) {
    const snn_rpn_level* const lv = c.lv;
    const int fdt = c.fdt, n_levels = c.n_levels, C = c.C, A = c.A, T = c.T, stage_mask = c.stage_mask;
    const snn_params* const p = c.p;
    const void* const w_shared_packed = c.w_shared_packed;
    unsigned long long* const spike_counts = c.spike_counts;
    void* const ws = c.ws;
    const snn_stream_t stream = c.stream;
    if (!lv || !p || !w_shared_packed || !c.w_heads_packed || !c.out_logits || !c.out_bbox || !ws)
        return fail(-1, "%s: null argument", c.who);
    if (n_levels <= 0 || n_levels > SNN_MAX_LEVELS) return fail(-1, "%s: n_levels=%d", c.who, n_levels);
    if (C <= 0 || A <= 0) return fail(-1, "%s: bad C/A", c.who);
    if (prec_family(p) != SNN_PRECISION_F32 && prec_family(p) != SNN_PRECISION_BF16X3 && prec_family(p) != SNN_PRECISION_MXFP6)
        return fail(-1, "%s: unknown precision %d", c.who, p->precision);
    if (prec_family(p) == SNN_PRECISION_MXFP6 && (C % 128 || !mx_tile_ok(lif_window_full_out(T).n)))
        return fail(-4, "%s: the mxfp6 kernels need C %% 128 == 0 and a T that fits a 512-row tile (C=%d, T=%d)", c.who, C, T);
    if (check_T(T, c.who)) return -1;
    for (int l = 0; l < n_levels; ++l)
        if (!lv[l].feat || lv[l].N <= 0 || lv[l].H <= 0 || lv[l].W <= 0)
            return fail(-1, "%s: bad level %d", c.who, l);
    for (int l = 0; l < n_levels; ++l)
        if (check_feat(lv[l].feat, fdt, c.who)) return -1;
    const bool nhwc = (fdt & SNN_FEAT_NHWC) != 0;
    if (nhwc && C % 32) return SNN_STATUS_NO_TYPED_KERNEL;       // (channels-last kernels: whole channel words only; nothing enqueued)
    int max_n = 0;
    const long long P = rpn_positions(lv, n_levels, &max_n);
    size_t o_spk, o_cur, o_cnt, need;
    const bool mxp = prec_family(p) != SNN_PRECISION_F32;            // encoder planes with a zero halo (k_gemm_bf16x3, k_gemm_mx)
    const long long Pe = mxp ? rpn_positions_padded(lv, n_levels) : P;
    rpn_ws_layout(P, mxp ? Pe : 0, C, T, prec_family(p), &o_spk, &o_cur, &o_cnt, &need);
    if (c.ws_bytes < need) return fail(-2, "%s: workspace %zu < %zu bytes", c.who, c.ws_bytes, need);
    const int Cw = cdiv(C, 32);
    const size_t stride = (size_t)P * Cw;            // words per time plane (spike planes)
    const size_t enc_stride = (size_t)Pe * Cw;       // ... of the encoder planes
    const int Tc = lif_window_full_out(T).n;         // encoder planes / conv currents of steps 0 .. Tc-1 (dead time steps: T-1)
    // period planes (snn_common.h): the encoder writes e_n = (first spike at step n - 1), the conv tile accumulates u_n = W e_n and
    // its LIF epilogue adds up the divisors' u_n - a quarter of the operand switching in the power-limited matrix-core loop
    const bool per = knobs().periods && periods_possible(p) && g3_some_tile_ok(Tc, true);
    snn_planes_view pv;                              // the shared LIF's planes: blocks of four words or rows (rpn_planes_split)
    rpn_planes_view(p, P, C, A, T, o_spk, &pv);
    bool split = pv.layout == SNN_PLANES_SPLIT4;
    // bf16x3: encoder planes word-major [T][Cw][Pe] - a conv tile's spike words of a chunk are then 128-byte runs (L2 read
    // requests of the launch 1.98e8 -> 1.68e8, conv+LIF -1.1 %).  Round 2 kept the convolution on row-major planes because a
    // 128-byte line of a word plane is shared by horizontally adjacent tiles, which then sat on different XCDs (FETCH_SIZE
    // x 2); with the XCD-contiguous tile order of round 3 the neighbours share an L2 and the fetch traffic is the same for
    // both layouts (profiles/r3_word_major_conv.txt).  SNN_PLANES=rm switches back (bit-identical).
    const size_t wm_rows = (prec_family(p) == SNN_PRECISION_BF16X3 && knobs().planes != 1) ? (size_t)Pe : 0;
    uint32_t* enc = (uint32_t*)ws;
    uint32_t* spk = (uint32_t*)((char*)ws + o_spk);
    hipStream_t s = (hipStream_t)stream;
    // round 5: where the conv will run the structured-sparse launch, the encoder launch writes the planes e_3 .. compressed itself (no
    // k_compress_planes launch, no raw words of those planes).  Asked of the conv's own launcher (nothing is enqueued by the query), so that
    // the two stages cannot disagree - also for a stage-by-stage caller
    // conv route AUTO (snn_rpn_head_forward_routed): where the plan is the sparse one - and the call counts no spikes - the encoder leaves every
    // period plane raw (the form the dense launch reads), and the conv stage enqueues compress + count, the decision and both launches behind the
    // gate word (co.route.gated); every other configuration runs its plan as it is
    ConvLifOpts co;
    co.wm = wm_rows != 0; co.out_split = &split; co.periods = per; co.sparse_side = (char*)ws + o_cur; co.sparse_bytes = o_cnt - o_cur;
    co.route = c.route; co.planes = weight_planes(p);
    bool fold = false;
    {
        NeuronP npq = make_p(p, p->v_th_enc);
        if (per) npq.v_fire = ENC_FIRED;
        const EncTh* ethq;
        const bool want_auto = c.route.route == SNN_ROUTE_AUTO && !spike_counts && stage_mask == SNN_STAGE_ALL;
        const bool may_fold = knobs().enc_fold && enc_mode(npq, &ethq) == ENC_QUANT;
        if (prec_family(p) == SNN_PRECISION_BF16X3 && per && wm_rows && (may_fold || want_auto)) {
            bool split_q = split;
            ConvLifOpts q = co;
            q.out_split = &split_q; q.sparse_mode = SPARSE_QUERY;
            const bool sparse_plan = conv3x3_lif_bf16x3_impl(enc, enc_stride, lv, n_levels, C, C, T, p, (const uint16_t*)w_shared_packed, spk, stride, spike_counts,
                                                             max_n, stream, q) == 1;
            co.route.gated = sparse_plan && want_auto;
            fold = sparse_plan && may_fold && !co.route.gated;
        }
    }
    co.sparse_mode = fold ? SPARSE_RUN_COMPRESSED : SPARSE_RUN;
    uint32_t* enc_cmp = fold ? (uint32_t*)((char*)ws + o_cur) : nullptr;
    if (stage_mask & SNN_STAGE_ENCODE) {                        // rpn.py:101, all levels in one launch
        EncLevels el;
        memset(&el, 0, sizeof(el));
        long long pos = 0;
        int blocks = 0;
        for (int l = 0; l < n_levels; ++l) {
            if (!lv[l].feat) return fail(-1, "%s: level %d has no features", c.who, l);
            el.feat[l] = lv[l].feat; el.HW[l] = lv[l].H * lv[l].W; el.bpi[l] = cdiv(el.HW[l], ENC_PB);
            el.blk_base[l] = blocks; el.pos_base[l] = (int)pos; el.Wpad[l] = mxp ? lv[l].W : 0;
            blocks += lv[l].N * el.bpi[l];
            pos += mxp ? (long long)lv[l].N * (lv[l].H + 2) * (lv[l].W + 2) : (long long)lv[l].N * el.HW[l];
        }
        el.blk_base[n_levels] = blocks; el.n_levels = n_levels;
        // (the one-position zero halo around every image is written by the encoder launch itself: encode_block)
        NeuronP np = make_p(p, p->v_th_enc);
        if (per) np.v_fire = ENC_FIRED;
        const EncTh* eth;
        const int em = g_last_enc_mode = enc_mode(np, &eth);
        const dim3 ge(blocks, cdiv(Cw, ENC_WB));
        uint32_t* const cmp_e = em == ENC_QUANT ? enc_cmp : nullptr;         // (the compressed-plane fold: period planes by thresholds only)
        launch_picked(encode_levels_kernel(em, fdt), ge, dim3(256), nhwc ? ENC_NHWC_LDS_BYTES(Tc, feat_elem_bytes(fdt)) : ENC_LDS_BYTES(Tc), s, el, C, Cw, Tc, np,
                      *eth, enc, enc_stride, wm_rows, cmp_e, em == ENC_QUANT ? 2 : 0);
        SNN_CHECK_LAUNCH("k_encode_levels");
    }
    if (stage_mask & SNN_STAGE_CONV_LIF) {
        int conv_sparse = 0;                                     // g_last_conv_sparse of this call's conv (bf16x3 family)
        if (prec_family(p) == SNN_PRECISION_F32) {
            if (spike_counts) {
                hipError_t e = hipMemsetAsync(spike_counts, 0, sizeof(unsigned long long) * n_levels * max_n, s);
                if (e != hipSuccess) return fail(-3, "hipMemsetAsync failed: %s", hipGetErrorString(e));
            }
            int rc = launch_conv(lv, n_levels, C, C, T, p, enc, stride, (const float*)w_shared_packed, spk, stride,
                                 spike_counts, max_n, nullptr, s);
            if (rc) return rc;
        } else {
            // conv + LIF fused over T on the bf16 matrix cores (rpn.py:98-106): membrane state in registers, only
            // spike planes written (4.5 ms against 4.2 + 0.5 ms for snn_spike_conv3x3_bf16x3 + snn_lif_scan, which
            // give bit-identical planes)
            // spike-rate mode: the LIF epilogue popcounts the spike words it ballots and adds them per (level, image)
            if (spike_counts && hipMemsetAsync(spike_counts, 0, sizeof(unsigned long long) * n_levels * max_n, s) != hipSuccess)
                return fail(-3, "hipMemsetAsync failed");
            int rc = prec_family(p) == SNN_PRECISION_MXFP6
                         ? conv3x3_lif_mx_impl(enc, enc_stride, lv, n_levels, C, C, T, p, (const uint32_t*)w_shared_packed, spk, stride,
                                               spike_counts, max_n, stream)
                         : conv3x3_lif_bf16x3_impl(enc, enc_stride, lv, n_levels, C, C, T, p, (const uint16_t*)w_shared_packed,
                                                   spk, stride, spike_counts, max_n, stream, co);
            if (rc) return rc;
            conv_sparse = prec_family(p) == SNN_PRECISION_BF16X3 ? g_last_conv_sparse : 0;
        }
        // route_stat of a call that did not decide on the device: {0, 0, 0 = the sparse launch ran (and always in spike-rate mode) / 1 = dense, 0}
        if (c.route.stat && conv_sparse != 2) {
            hipLaunchKernelGGL(k_route_decide, dim3(1), dim3(64), 0, s, (int*)c.route.stat, (const int*)nullptr, 0, 0, 0.0f, (spike_counts || conv_sparse) ? 0 : 1);
            SNN_CHECK_LAUNCH("k_route_decide");
        }
    }
    if (split != (pv.layout == SNN_PLANES_SPLIT4)) return fail(-3, "%s: the conv left another spike-plane layout than planned (internal)", c.who);
    g_last_rpn_planes[0] = pv.offset_bytes; g_last_rpn_planes[1] = split ? 1 : 0; g_last_rpn_planes[2] = (unsigned long long)pv.rows;
    if (!(stage_mask & SNN_STAGE_LI_HEADS)) return 0;
    if (!c.steps)
        return li_heads_impl(spk, stride, T, (int)P, C, c.w_heads_packed, A, 4 * A, p, c.out_logits, c.out_bbox, c.sum_logits,
                             c.sum_bbox, split, stream);
    int rc = li_heads_readouts_impl(spk, stride, c.steps, c.n_steps, (int)P, C, c.w_heads_packed, A, 4 * A, p, c.out_logits, c.out_bbox,
                                    c.sum_logits, c.sum_bbox, split, stream);
    if (rc || !spike_counts) return rc;
    // [n][n_levels][max_n]: popcounts of the shared LIF's planes t < T'_j per (level, image).  The conv above ran as a spike-rate
    // forward at T (same launch) and left its counts in the first rows of spike_counts: zeroed and overwritten here
    if (hipMemsetAsync(spike_counts, 0, sizeof(unsigned long long) * c.n_steps * n_levels * max_n, s) != hipSuccess)
        return fail(-3, "hipMemsetAsync failed");
    const StepList st = step_list(c.steps, c.n_steps);
    long long pb = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int hw = lv[l].H * lv[l].W;
        const int wpi = split ? hw * 4 : hw * Cw;                // blocks of four words [T][2][P][4]: the image's words of both halves
        hipLaunchKernelGGL(k_count_spikes_ro, dim3(lv[l].N, max(1, min(256, wpi / 2048))), dim3(256), 0, s, spk + (size_t)pb * (split ? 4 : Cw),
                           (unsigned long long)stride, split ? (unsigned long long)P * 4 : 0ull, wpi, st, spike_counts + (size_t)l * max_n,
                           (unsigned long long)n_levels * max_n);
        SNN_CHECK_LAUNCH("k_count_spikes_ro");
        pb += (long long)lv[l].N * hw;
    }
    return 0;
}

int snn_rpn_head_forward_stages(const snn_rpn_level* lv, int n_levels, int C, int A, int T, const snn_params* p,
                                const void* w_shared_packed, const float* w_heads_packed, float* out_logits,
                                float* out_bbox, unsigned long long* spike_counts, float* sum_logits,
                                float* sum_bbox, void* ws, size_t ws_bytes, int stage_mask, snn_stream_t stream) {
    return snn_rpn_head_forward_stages_typed(lv, SNN_FEAT_F32, n_levels, C, A, T, p, w_shared_packed, w_heads_packed, out_logits, out_bbox,
                                             spike_counts, sum_logits, sum_bbox, ws, ws_bytes, stage_mask, stream);
}

int snn_rpn_head_forward_stages_typed(const snn_rpn_level* lv, int fdt, int n_levels, int C, int A, int T, const snn_params* p,
                                      const void* w_shared_packed, const float* w_heads_packed, float* out_logits,
                                      float* out_bbox, unsigned long long* spike_counts, float* sum_logits,
                                      float* sum_bbox, void* ws, size_t ws_bytes, int stage_mask, snn_stream_t stream) {
    RpnCall c = rpn_call(lv, fdt, n_levels, C, A, T, p, w_shared_packed, w_heads_packed, out_logits, out_bbox, spike_counts, sum_logits, sum_bbox,
                         ws, ws_bytes, stream);
    c.stage_mask = stage_mask;
    return rpn_head_run(c);
}

int snn_rpn_head_forward(const snn_rpn_level* lv, int n_levels, int C, int A, int T, const snn_params* p,
                         const void* w_shared_packed, const float* w_heads_packed, float* out_logits,
                         float* out_bbox, unsigned long long* spike_counts, float* sum_logits, float* sum_bbox,
                         void* ws, size_t ws_bytes, snn_stream_t stream) {
    return snn_rpn_head_forward_stages_typed(lv, SNN_FEAT_F32, n_levels, C, A, T, p, w_shared_packed, w_heads_packed, out_logits, out_bbox,
                                             spike_counts, sum_logits, sum_bbox, ws, ws_bytes, SNN_STAGE_ALL, stream);
}

// the routed forward's workspace: the plain forward's.  Its first plane set holds the raw planes of every period (the encoder form of the dense
// plan), its side buffer the compressed planes; the gate word is route_stat[2], in the caller's array
size_t snn_rpn_head_workspace_bytes_routed(const snn_rpn_level* lv, int n_levels, int C, int A, int T, int precision, int route) {
    if (!route_known(route)) return 0;
    return snn_rpn_head_workspace_bytes(lv, n_levels, C, A, T, precision);
}

int snn_rpn_head_forward_routed(const snn_rpn_level* lv, int fdt, int n_levels, int C, int A, int T, const snn_params* p,
                                const void* w_shared_packed, const float* w_heads_packed, float* out_logits, float* out_bbox,
                                unsigned long long* spike_counts, float* sum_logits, float* sum_bbox, void* ws, size_t ws_bytes,
                                int route, float crossover, int32_t* route_stat, snn_stream_t stream) {
    // (no p, or a shape the size query answers with 0: the pass's own message)
    const size_t need = p ? snn_rpn_head_workspace_bytes_routed(lv, n_levels, C, A, T, p->precision, route) : 0;
    if (route_check("snn_rpn_head_forward_routed", route, crossover, route_stat, ws_bytes, need)) return -1;
    RpnCall c = rpn_call(lv, fdt, n_levels, C, A, T, p, w_shared_packed, w_heads_packed, out_logits, out_bbox, spike_counts, sum_logits, sum_bbox,
                         ws, ws_bytes, stream);
    c.route = routed(route, crossover, route_stat, spike_counts != nullptr);
    return rpn_head_run(c);
}

int snn_rpn_head_forward_readouts(const snn_rpn_level* lv, int n_levels, int C, int A, const int* steps, int n_steps,
                                  const snn_params* p, const void* w_shared_packed, const float* w_heads_packed, float* out_logits,
                                  float* out_bbox, unsigned long long* spike_counts, float* sum_logits, float* sum_bbox,
                                  void* ws, size_t ws_bytes, snn_stream_t stream) {
    return snn_rpn_head_forward_readouts_typed(lv, SNN_FEAT_F32, n_levels, C, A, steps, n_steps, p, w_shared_packed, w_heads_packed, out_logits,
                                               out_bbox, spike_counts, sum_logits, sum_bbox, ws, ws_bytes, stream);
}

int snn_rpn_head_forward_readouts_typed(const snn_rpn_level* lv, int fdt, int n_levels, int C, int A, const int* steps, int n_steps,
                                        const snn_params* p, const void* w_shared_packed, const float* w_heads_packed, float* out_logits,
                                        float* out_bbox, unsigned long long* spike_counts, float* sum_logits, float* sum_bbox,
                                        void* ws, size_t ws_bytes, snn_stream_t stream) {
    if (check_steps(steps, n_steps, "snn_rpn_head_forward_readouts")) return -1;
    if ((sum_logits == nullptr) != (sum_bbox == nullptr)) return fail(-1, "snn_rpn_head_forward_readouts: sum_logits and sum_bbox go together");
    RpnCall c = rpn_call(lv, fdt, n_levels, C, A, steps[n_steps - 1], p, w_shared_packed, w_heads_packed, out_logits, out_bbox, spike_counts, sum_logits,
                         sum_bbox, ws, ws_bytes, stream);
    c.steps = steps; c.n_steps = n_steps;
    return rpn_head_run(c);
}

// ---- finished spike-rate tensors -------------------------------------------------------------------
size_t snn_rpn_rates_workspace_bytes(int n_levels, int max_n) {
    return (n_levels > 0 && max_n > 0) ? (size_t)n_levels * max_n * 2 * RATE_CH * sizeof(double) : 0;
}

int snn_rpn_rates(const snn_rpn_level* lv, int n_levels, int C, int A, int T, const unsigned long long* spike_counts,
                  const float* sum_logits, const float* sum_bbox, float* rates, void* ws, size_t ws_bytes, snn_stream_t stream) {
    if (!lv || !spike_counts || !sum_logits || !sum_bbox || !rates || !ws) return fail(-1, "snn_rpn_rates: null argument");
    if (n_levels <= 0 || n_levels > SNN_MAX_LEVELS || C <= 0 || A <= 0) return fail(-1, "snn_rpn_rates: bad argument");
    if (check_T(T, "snn_rpn_rates")) return -1;
    RpnRatesArgs a;
    memset(&a, 0, sizeof(a));
    int max_n = 0;
    long long pos = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (lv[l].N <= 0 || lv[l].H <= 0 || lv[l].W <= 0) return fail(-1, "snn_rpn_rates: bad level %d", l);
        a.pos_base[l] = (int)pos; a.N[l] = lv[l].N; a.HW[l] = lv[l].H * lv[l].W;
        pos += (long long)lv[l].N * a.HW[l];
        max_n = max(max_n, lv[l].N);
    }
    if (ws_bytes < snn_rpn_rates_workspace_bytes(n_levels, max_n)) return fail(-2, "snn_rpn_rates: workspace too small");
    a.counts = spike_counts; a.sum_l = sum_logits; a.sum_b = sum_bbox; a.part = (double*)ws; a.rates = rates;
    a.n_levels = n_levels; a.max_n = max_n; a.A = A; a.T = T; a.C = C;
    hipLaunchKernelGGL(k_rpn_rate_partials, dim3(RATE_CH, 2, n_levels * max_n), dim3(256), 0, (hipStream_t)stream, a);
    SNN_CHECK_LAUNCH("k_rpn_rate_partials");
    hipLaunchKernelGGL(k_rpn_rate_final, dim3(cdiv(n_levels * 3 * max_n, 64)), dim3(64), 0, (hipStream_t)stream, a);
    SNN_CHECK_LAUNCH("k_rpn_rate_final");
    return 0;
}

int snn_det_rates(int R, int D, int Hd, int K, int K4, int T, int only_one_bbox, const uint32_t* spk6_count,
                  const uint32_t* spk7_count, const float* sum_cls, const float* sum_bbox, float* rates, snn_stream_t stream) {
    if (!spk6_count || !spk7_count || !sum_cls || !sum_bbox || !rates) return fail(-1, "snn_det_rates: null argument");
    if (R <= 0 || D <= 0 || Hd <= 0 || K <= 0 || K4 <= 0) return fail(-1, "snn_det_rates: bad shape");
    if (check_T(T, "snn_det_rates")) return -1;
    hipLaunchKernelGGL(k_det_rates, dim3(cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, spk6_count, spk7_count, sum_cls, sum_bbox,
                       R, (long long)D, (long long)Hd, K, K4, T, only_one_bbox, rates);
    SNN_CHECK_LAUNCH("k_det_rates");
    return 0;
}

// ---- RPN proposal selection -------------------------------------------------------------------
int snn_rpn_proposals_candidates(const snn_rpn_post_level* lv, int n_levels, int A, int pre_nms_top_n) {
    if (!lv || n_levels <= 0 || n_levels > SNN_MAX_LEVELS || A <= 0 || pre_nms_top_n <= 0) return -1;
    long long k = 0;
    for (int l = 0; l < n_levels; ++l) k += min((long long)pre_nms_top_n, (long long)lv[l].H * lv[l].W * A);
    return k > 0x7fffffffLL ? -1 : (int)k;
}

// workspace of snn_rpn_proposals: candidates of the batch + one NMS list per (image, level)
// (mask_words = mask words per image: sum over the levels of k_l * ceil(k_l / 64) <= K * ceil(K / 64))
static size_t rpn_post_layout(int N, int K, size_t mask_words, size_t off[13]) {
    const size_t nk = (size_t)N * K, lists = (size_t)N * SNN_MAX_LEVELS;
    const size_t sz[13] = {nk * 4, nk * 4, nk * 16, nk * 16, nk * 4, nk * 4, nk * 4, lists * 4,
                           (size_t)N * mask_words * 8,
                           lists * sizeof(TopkState), lists * 2048 * 4 + 2 * lists * 4, lists * TOPK_CH * 1024 * 4, lists * (size_t)K * 8};
    size_t o = 0;
    for (int i = 0; i < 13; ++i) { off[i] = o; o += align_up(sz[i], 256); }
    return o;
}

size_t snn_rpn_proposals_workspace_bytes(int N, int K_candidates) {
    size_t off[13];
    // (the level split is not known here: one list of K candidates per image bounds every split)
    return (N > 0 && K_candidates > 0) ? rpn_post_layout(N, K_candidates, (size_t)K_candidates * cdiv(K_candidates, 64), off) : 0;
}

int snn_rpn_proposals(const snn_rpn_post_level* lv, int n_levels, int N, int A, const float* image_hw_host,
                      int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float score_thresh, float min_size,
                      float* out_boxes, float* out_scores, int* out_counts, float* pre_boxes, float* pre_prob,
                      void* ws, size_t ws_bytes, snn_stream_t stream) {
    if (!lv || !image_hw_host || !out_boxes || !out_scores || !out_counts || !ws)
        return fail(-1, "snn_rpn_proposals: null argument");
    if (n_levels <= 0 || n_levels > SNN_MAX_LEVELS || N <= 0 || N > RPN_MAX_IMAGES || A <= 0 || A > RPN_MAX_ANCHORS ||
        pre_nms_top_n <= 0 || post_nms_top_n <= 0)
        return fail(-1, "snn_rpn_proposals: bad argument (levels <= %d, images <= %d, anchors <= %d)", SNN_MAX_LEVELS,
                    RPN_MAX_IMAGES, RPN_MAX_ANCHORS);
    const int K = snn_rpn_proposals_candidates(lv, n_levels, A, pre_nms_top_n);
    if (K <= 0 || K > RPN_SORT_MAX) return fail(-1, "snn_rpn_proposals: %d candidates per image (max %d)", K, RPN_SORT_MAX);
    hipStream_t s = (hipStream_t)stream;
    RpnPostArgs a;
    memset(&a, 0, sizeof(a));
    NmsLists nl;
    memset(&nl, 0, sizeof(nl));
    int koff = 0, kmax = 0;
    size_t mask_words = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (!lv[l].logits || !lv[l].deltas || lv[l].H <= 0 || lv[l].W <= 0) return fail(-1, "snn_rpn_proposals: bad level %d", l);
        if ((long long)lv[l].H * lv[l].W * A * N > 0x7fffffffLL || (long long)lv[l].H * lv[l].W * A >= (1 << 28))
            return fail(-1, "snn_rpn_proposals: level %d too large", l);
        RpnPostLevel& L = a.lv[l];
        L.logits = lv[l].logits; L.deltas = lv[l].deltas; L.H = lv[l].H; L.W = lv[l].W;
        L.n = lv[l].H * lv[l].W * A; L.k = min(pre_nms_top_n, L.n); L.koff = koff; koff += L.k;
        L.sh = lv[l].stride_h; L.sw = lv[l].stride_w;
        memcpy(L.base, lv[l].base_anchors, sizeof(float) * 4 * A);
        nl.off[l] = L.koff; nl.cap[l] = L.k; nl.moff[l] = (long long)mask_words;
        mask_words += (size_t)L.k * cdiv(L.k, 64);
        kmax = max(kmax, L.k);
    }
    size_t off[13];
    // (the size query does not know the level split and bounds every one of them; the call holds the caller to the query, as every other entry
    // does, and not to the smaller layout of this split - which a caller cannot ask for)
    if (ws_bytes < snn_rpn_proposals_workspace_bytes(N, K) || ws_bytes < rpn_post_layout(N, K, mask_words, off))
        return fail(-2, "snn_rpn_proposals: workspace too small");
    for (int i = 0; i < N; ++i) { a.img_h[i] = image_hw_host[2 * i]; a.img_w[i] = image_hw_host[2 * i + 1]; }
    a.n_levels = n_levels; a.N = N; a.A = A; a.Ktot = K; a.post_n = post_nms_top_n;
    a.score_thresh = score_thresh; a.min_size = min_size; a.clip = (float)4.135166556742356;     // log(1000/16), boxes.py
    char* w = (char*)ws;
    a.cand_idx = (int*)(w + off[0]); a.cand_logit = (float*)(w + off[1]); a.boxes = (float*)(w + off[2]);
    // the pre-NMS report goes straight to the caller's buffers, in candidate order = the reference's order (rpn.py:493-499)
    a.pre = pre_boxes ? pre_boxes : (float*)(w + off[3]); a.prob = pre_prob ? pre_prob : (float*)(w + off[4]); a.skey = (float*)(w + off[5]);
    int* keep = (int*)(w + off[6]);
    int* n_keep = (int*)(w + off[7]);
    unsigned long long* mask = (unsigned long long*)(w + off[8]);
    {   // top-k per (level, image): three (histogram, pick) rounds, gather, sort
        TopkState* st = (TopkState*)(w + off[9]);
        uint32_t* g_hist = (uint32_t*)(w + off[10]);
        uint32_t* g_hist3 = (uint32_t*)(w + off[11]);
        unsigned long long* sel = (unsigned long long*)(w + off[12]);
        const int lists = N * n_levels;
        // (behind the histograms: per-list count / largest coordinate of the candidates that pass the filters, for the NMS)
        a.list_cnt = (int*)(g_hist + (size_t)N * SNN_MAX_LEVELS * 2048);
        a.list_max = (uint32_t*)(a.list_cnt + (size_t)N * SNN_MAX_LEVELS);
        const size_t n_clear = (size_t)N * SNN_MAX_LEVELS * 2048 + 2 * (size_t)N * SNN_MAX_LEVELS;     // (inside region 10: rpn_post_layout)
        hipLaunchKernelGGL(k_topk_clear, dim3(min(cdiv((long long)n_clear, 256), 1024)), dim3(256), 0, s, g_hist, n_clear);
        SNN_CHECK_LAUNCH("k_topk_clear");
        for (int pass = 0; pass < 3; ++pass) {
            hipLaunchKernelGGL(k_topk_hist, dim3(TOPK_CH, n_levels, N), dim3(256), 0, s, a, pass, st, g_hist, g_hist3);
            SNN_CHECK_LAUNCH("k_topk_hist");
            hipLaunchKernelGGL(k_topk_pick, dim3(lists), dim3(1024), 0, s, a, pass, st, g_hist);
            SNN_CHECK_LAUNCH("k_topk_pick");
        }
        hipLaunchKernelGGL(k_topk_gather, dim3(TOPK_CH, n_levels, N), dim3(256), 0, s, a, st, g_hist3, sel, K);
        SNN_CHECK_LAUNCH("k_topk_gather");
        hipLaunchKernelGGL(k_topk_sort, dim3(n_levels, N), dim3(1024), 0, s, a, sel, K);
        SNN_CHECK_LAUNCH("k_topk_sort");
    }
    hipLaunchKernelGGL(k_rpn_decode, dim3(cdiv((long long)N * K, 256)), dim3(256), 0, s, a);
    SNN_CHECK_LAUNCH("k_rpn_decode");
    // NMS: one list per (image, level) - the candidates of a level already are in score order (k_rpn_topk), the filtered
    // ones start out removed
    nl.boxes = a.boxes; nl.skey = a.skey; nl.n_dev = nullptr; nl.img_stride = K; nl.mask_img = (long long)mask_words; nl.L = n_levels;
    nl.max_keep0 = nl.max_keep = post_nms_top_n;
    nl.trick_cnt = a.list_cnt; nl.trick_max = a.list_max; nl.trick_c0 = 0;     // all levels of an image are one batched_nms call
    const int wmax = cdiv(kmax, 64);
    hipLaunchKernelGGL(k_nms_mask_lists, dim3(wmax, wmax, N * n_levels), dim3(64), 0, s, nl, nms_thresh, mask);
    SNN_CHECK_LAUNCH("k_nms_mask_lists");
    const size_t lds = (size_t)2 * 64 * wmax * 8;
    hipError_t e = hipFuncSetAttribute((const void*)k_nms_scan_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_nms_scan_lists, dim3(N * n_levels), dim3(256), lds, s, nl, mask, keep, n_keep);
    SNN_CHECK_LAUNCH("k_nms_scan_lists");
    hipLaunchKernelGGL(k_rpn_merge, dim3(N), dim3(1024), 0, s, a, keep, n_keep, out_boxes, out_scores, out_counts);
    SNN_CHECK_LAUNCH("k_rpn_merge");
    return 0;
}

// ---- detection post-processing ------------------------------------------------------------------
static size_t det_post_layout(int N, int K, int Rmax, size_t off[9]) {
    const size_t lk = (size_t)N * K * Rmax, L = (size_t)N * K;
    const size_t sz[9] = {lk * 16, lk * 4, lk * 16, lk * 4, lk * 4, 2 * L * 4, lk * 4, L * 4, lk * cdiv(Rmax, 64) * 8};
    size_t o = 0;
    for (int i = 0; i < 9; ++i) { off[i] = o; o += align_up(sz[i], 256); }
    return o;
}

size_t snn_det_postprocess_workspace_bytes(int N, int max_rois_per_image, int K) {
    size_t off[9];
    if (N <= 0 || max_rois_per_image <= 0 || K < 2) return 0;
    return det_post_layout(N, K, max_rois_per_image, off);
}

// the launches of both entry points.  counts_dev = nullptr: compacted rows, a.roi_base[] filled (snn_det_postprocess); else rows [N][Rmax]
// with the count of image i read from counts_dev[i] on the device, and the output rows behind the detections zeroed
static int det_post_run(DetPostArgs& a, const int* counts_dev, float nms_thresh, float* out_boxes, float* out_scores, int* out_labels,
                        int* out_counts, void* ws, size_t ws_bytes, hipStream_t s, const char* who) {
    const int N = a.N, K = a.K, rmax = a.Rmax;
    size_t off[9];
    if (ws_bytes < det_post_layout(N, K, rmax, off)) return fail(-2, "%s: workspace too small", who);
    char* w = (char*)ws;
    a.boxes = (float*)(w + off[0]); a.skey = (float*)(w + off[1]);
    a.s_boxes = (float*)(w + off[2]); a.s_score = (float*)(w + off[3]); a.s_roi = (int*)(w + off[4]); a.n_valid = (int*)(w + off[5]);
    int* keep = (int*)(w + off[6]);
    int* n_keep = (int*)(w + off[7]);
    unsigned long long* mask = (unsigned long long*)(w + off[8]);
    const int L = N * K;
    if (counts_dev) {
        hipLaunchKernelGGL(k_det_candidates_padded, dim3(cdiv(rmax, 256), L), dim3(256), 0, s, a, counts_dev);
        SNN_CHECK_LAUNCH("k_det_candidates_padded");
    } else {
        hipLaunchKernelGGL(k_det_candidates, dim3(cdiv(rmax, 256), L), dim3(256), 0, s, a);
        SNN_CHECK_LAUNCH("k_det_candidates");
    }
    int np2 = 1;
    while (np2 < rmax) np2 <<= 1;
    const size_t sort_lds = max((size_t)np2 * 8, (size_t)256);
    hipError_t e = hipFuncSetAttribute((const void*)k_sort_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    uint32_t* list_max = (uint32_t*)(a.n_valid + L);
    hipLaunchKernelGGL(k_sort_lists, dim3(L), dim3(1024), sort_lds, s, a.skey, a.boxes, rmax, a.s_boxes, a.s_score, a.s_roi, a.n_valid, list_max);
    SNN_CHECK_LAUNCH("k_sort_lists");
    // NMS: one list per (image, class); a foreground class stops after detections_per_img kept boxes, the background list keeps all
    NmsLists nl;
    memset(&nl, 0, sizeof(nl));
    const int wmax = cdiv(rmax, 64);
    nl.boxes = a.s_boxes; nl.skey = nullptr; nl.n_dev = a.n_valid; nl.img_stride = (long long)K * rmax;
    nl.mask_img = (long long)K * rmax * wmax; nl.L = K;
    for (int c = 0; c < K; ++c) { nl.off[c] = c * rmax; nl.cap[c] = rmax; nl.moff[c] = (long long)c * rmax * wmax; }
    nl.max_keep0 = rmax; nl.max_keep = a.det_per_img;
    nl.trick_cnt = a.n_valid; nl.trick_max = list_max; nl.trick_c0 = 1;    // the foreground classes of an image are one batched_nms call
    hipLaunchKernelGGL(k_nms_mask_lists, dim3(wmax, wmax, L), dim3(64), 0, s, nl, nms_thresh, mask);
    SNN_CHECK_LAUNCH("k_nms_mask_lists");
    const size_t lds = (size_t)2 * 64 * wmax * 8;
    if (lds > 160 * 1024) return fail(-4, "%s: %d RoIs per image need %zu B of LDS for the NMS walk", who, rmax, lds);
    e = hipFuncSetAttribute((const void*)k_nms_scan_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_nms_scan_lists, dim3(L), dim3(256), lds, s, nl, mask, keep, n_keep);
    SNN_CHECK_LAUNCH("k_nms_scan_lists");
    hipLaunchKernelGGL(k_det_merge, dim3(N), dim3(1024), 0, s, a, keep, n_keep, out_boxes, out_scores, out_labels, out_counts);
    SNN_CHECK_LAUNCH("k_det_merge");
    if (counts_dev) {
        hipLaunchKernelGGL(k_det_zero_tail, dim3(cdiv(a.out_cap, 256), N), dim3(256), 0, s, out_counts, a.out_cap, out_boxes, out_scores, out_labels);
        SNN_CHECK_LAUNCH("k_det_zero_tail");
    }
    return 0;
}

static void det_post_fill(DetPostArgs& a, const float* class_logits, const float* box_regression, const float* proposals, int N, int K,
                          int rmax, const float* image_hw_host, const float* box_weights_host, float score_thresh, int detections_per_img,
                          float min_size, float* all_scores, float* all_boxes, int out_cap) {
    for (int i = 0; i < N; ++i) { a.img_h[i] = image_hw_host[2 * i]; a.img_w[i] = image_hw_host[2 * i + 1]; }
    a.logits = class_logits; a.deltas = box_regression; a.props = proposals;
    a.N = N; a.K = K; a.Rmax = rmax; a.det_per_img = detections_per_img; a.out_cap = out_cap;
    a.score_thresh = score_thresh; a.min_size = min_size; a.clip = (float)4.135166556742356;
    a.wx = box_weights_host[0]; a.wy = box_weights_host[1]; a.ww = box_weights_host[2]; a.wh = box_weights_host[3];
    a.all_scores = all_scores; a.all_boxes = all_boxes;
}

int snn_det_postprocess(const float* class_logits, const float* box_regression, const float* proposals,
                        const int* rois_per_image_host, int N, int K, const float* image_hw_host,
                        const float* box_weights_host, float score_thresh, float nms_thresh, int detections_per_img,
                        float min_size, float* all_scores, float* all_boxes, float* out_boxes, float* out_scores,
                        int* out_labels, int* out_counts, int out_cap, void* ws, size_t ws_bytes, snn_stream_t stream) {
    if (!class_logits || !box_regression || !proposals || !rois_per_image_host || !image_hw_host || !box_weights_host || !all_scores ||
        !all_boxes || !out_boxes || !out_scores || !out_labels || !out_counts || !ws)
        return fail(-1, "snn_det_postprocess: null argument");
    if (N <= 0 || N > RPN_MAX_IMAGES || K < 2 || K > NMS_MAX_CAT || detections_per_img <= 0)
        return fail(-1, "snn_det_postprocess: bad argument (images <= %d, classes <= %d)", RPN_MAX_IMAGES, NMS_MAX_CAT);
    DetPostArgs a;
    memset(&a, 0, sizeof(a));
    int rmax = 0;
    for (int i = 0; i < N; ++i) {
        if (rois_per_image_host[i] < 0) return fail(-1, "snn_det_postprocess: negative RoI count");
        a.roi_base[i + 1] = a.roi_base[i] + rois_per_image_host[i];
        rmax = max(rmax, rois_per_image_host[i]);
    }
    if (rmax == 0) {
        if (hipMemsetAsync(out_counts, 0, sizeof(int) * 2 * N, (hipStream_t)stream) != hipSuccess) return fail(-3, "hipMemsetAsync failed");
        return 0;
    }
    if (rmax > DET_SORT_MAX) return fail(-4, "snn_det_postprocess: %d RoIs per image (max %d)", rmax, DET_SORT_MAX);
    if ((long long)(K - 1) * min(detections_per_img, rmax) > DET_MERGE_MAX)
        return fail(-4, "snn_det_postprocess: (K-1) * detections_per_img = %lld exceeds %d", (long long)(K - 1) * detections_per_img, DET_MERGE_MAX);
    if (out_cap < detections_per_img + rmax) return fail(-1, "snn_det_postprocess: out_cap %d < %d", out_cap, detections_per_img + rmax);
    det_post_fill(a, class_logits, box_regression, proposals, N, K, rmax, image_hw_host, box_weights_host, score_thresh, detections_per_img,
                  min_size, all_scores, all_boxes, out_cap);
    return det_post_run(a, nullptr, nms_thresh, out_boxes, out_scores, out_labels, out_counts, ws, ws_bytes, (hipStream_t)stream,
                        "snn_det_postprocess");
}

#define DET_PADDED_MAX_ROIS 10240                 // 2 x 64 x ceil(cap / 64) x 8 B of LDS for the NMS walk <= 160 KB
int snn_det_postprocess_padded(const float* class_logits, const float* box_regression, const float* proposals,
                               const int* roi_counts_dev, int N, int cap, int K, const float* image_hw_host,
                               const float* box_weights_host, float score_thresh, float nms_thresh, int detections_per_img,
                               float min_size, float* all_scores, float* all_boxes, float* out_boxes, float* out_scores,
                               int* out_labels, int* out_counts, int out_cap, void* ws, size_t ws_bytes, snn_stream_t stream) {
    if (!class_logits || !box_regression || !proposals || !roi_counts_dev || !image_hw_host || !box_weights_host || !all_scores ||
        !all_boxes || !out_boxes || !out_scores || !out_labels || !out_counts || !ws)
        return fail(-1, "snn_det_postprocess_padded: null argument");
    if (N <= 0 || N > RPN_MAX_IMAGES || cap <= 0 || K < 2 || K > NMS_MAX_CAT || detections_per_img <= 0)
        return fail(-1, "snn_det_postprocess_padded: bad argument (1 <= images <= %d, cap >= 1, 2 <= classes <= %d)", RPN_MAX_IMAGES, NMS_MAX_CAT);
    if (cap > DET_PADDED_MAX_ROIS) return fail(-4, "snn_det_postprocess_padded: cap = %d rows per image (max %d)", cap, DET_PADDED_MAX_ROIS);
    if ((long long)(K - 1) * min(detections_per_img, cap) > DET_MERGE_MAX)
        return fail(-4, "snn_det_postprocess_padded: (K-1) * detections_per_img = %lld exceeds %d", (long long)(K - 1) * detections_per_img, DET_MERGE_MAX);
    if (out_cap < detections_per_img + cap) return fail(-1, "snn_det_postprocess_padded: out_cap %d < %d", out_cap, detections_per_img + cap);
    DetPostArgs a;
    memset(&a, 0, sizeof(a));
    det_post_fill(a, class_logits, box_regression, proposals, N, K, cap, image_hw_host, box_weights_host, score_thresh, detections_per_img,
                  min_size, all_scores, all_boxes, out_cap);
    return det_post_run(a, roi_counts_dev, nms_thresh, out_boxes, out_scores, out_labels, out_counts, ws, ws_bytes, (hipStream_t)stream,
                        "snn_det_postprocess_padded");
}

// ---- RoI table of the fused RoIAlign encoder from padded proposals ---------------------------------
int snn_roi_assign(const float* boxes, const int* counts_dev, int N, int cap, int k_min, int k_max, float canonical_scale,
                   float canonical_level, float* rois, int* roi_batch, int* roi_level, snn_stream_t stream) {
    if (!boxes || !counts_dev || !rois || !roi_batch || !roi_level) return fail(-1, "snn_roi_assign: null argument");
    if (N <= 0 || N > RPN_MAX_IMAGES || cap <= 0 || cap > DET_PADDED_MAX_ROIS)
        return fail(-1, "snn_roi_assign: bad argument (1 <= images <= %d, 1 <= cap <= %d)", RPN_MAX_IMAGES, DET_PADDED_MAX_ROIS);
    if (k_min > k_max || k_max - k_min >= SNN_MAX_LEVELS || !(canonical_scale > 0.0f))
        return fail(-1, "snn_roi_assign: bad level range (k_min <= k_max < k_min + %d, canonical_scale > 0)", SNN_MAX_LEVELS);
    hipLaunchKernelGGL(k_roi_assign, dim3(cdiv((long long)N * cap, 256)), dim3(256), 0, (hipStream_t)stream, boxes, counts_dev, N, cap,
                       k_min, k_max, canonical_scale, canonical_level, rois, roi_batch, roi_level);
    SNN_CHECK_LAUNCH("k_roi_assign");
    return 0;
}

// ---- padded detections -> the exchange rows of the data-parallel path ------------------------------
#define PACK_MAX_DET (1 << 24)                    // counts ride the all-gather as fp32 (dp.all_gather_detection_tensors): exact below 2^24
int snn_pack_padded_detections(const float* out_boxes, const float* out_scores, const int32_t* out_labels, const int32_t* out_counts,
                               int N, int out_cap, int max_det, float* payload, int32_t* counts, snn_stream_t stream) {
    if (!out_boxes || !out_scores || !out_labels || !out_counts || !payload || !counts)
        return fail(-1, "snn_pack_padded_detections: null argument");
    if (N <= 0 || N > RPN_MAX_IMAGES || out_cap <= 0 || max_det <= 0)
        return fail(-1, "snn_pack_padded_detections: bad argument (1 <= images <= %d, out_cap >= 1, max_det >= 1)", RPN_MAX_IMAGES);
    if (((uintptr_t)out_boxes & 15) || ((uintptr_t)payload & 7))
        return fail(-1, "snn_pack_padded_detections: out_boxes must be 16-byte aligned and payload 8-byte aligned");
    if (max_det > PACK_MAX_DET) return fail(-4, "snn_pack_padded_detections: max_det = %d (max %d)", max_det, PACK_MAX_DET);
    const dim3 grid(min(cdiv(max_det, PACK_ROWS), 64), N);
    if (max_det % 2 == 0 && ((uintptr_t)payload & 15) == 0)    // every image's stripe of 24 * max_det bytes starts on a 16-byte boundary
        hipLaunchKernelGGL(k_pack_padded_detections<4>, grid, dim3(PACK_ROWS), 0, (hipStream_t)stream, out_boxes, out_scores, out_labels,
                           out_counts, out_cap, max_det, payload, counts);
    else
        hipLaunchKernelGGL(k_pack_padded_detections<2>, grid, dim3(PACK_ROWS), 0, (hipStream_t)stream, out_boxes, out_scores, out_labels,
                           out_counts, out_cap, max_det, payload, counts);
    SNN_CHECK_LAUNCH("k_pack_padded_detections");
    return 0;
}

#define DET_SYNC_BYTES 16384                    // (a guard gap between the spike planes and the raw encoder planes; round 4 kept tile counters here)
static void det_ws_layout(int R, int D, int Hd, int T, size_t* o_enc, size_t* o_cur, size_t* o_s6, size_t* o_s7,
                          size_t* total) {
    const size_t enc = align_up((size_t)T * R * cdiv(D, 32) * 4, 256);
    // currents [T R][Hd] of the un-fused paths; in the fused bf16x3 path the region holds the side buffers of the structured-sparse fc6
    // (snn_sparse.h) instead, so it is at least that large
    const size_t cur = max(align_up((size_t)T * R * cdiv(Hd, 32) * 32 * 4, 256), align_up(sparse_side_bytes(R, R, cdiv(D, 32), T), 256));
    const size_t sp = align_up((size_t)T * R * cdiv(Hd, 32) * 4, 256);
    *o_enc = 0; *o_cur = enc; *o_s6 = enc + cur; *o_s7 = enc + cur + sp; *total = enc + cur + 2 * sp + DET_SYNC_BYTES + enc;
}
static size_t det_ws_perm_offset(int R, int D, int Hd, int T) {        // the encoder planes in permuted reduction order (k_permute_planes): the last `enc` bytes
    size_t a, b, c, d, tot;
    det_ws_layout(R, D, Hd, T, &a, &b, &c, &d, &tot);
    return tot - b;                                                   // (b = o_cur = size of the encoder planes)
}

size_t snn_det_head_workspace_bytes(int R, int D, int Hd, int K, int K4, int T, int precision) {
    (void)K; (void)K4; (void)precision;
    if (R <= 0 || D <= 0 || Hd <= 0 || T < 1) return 0;
    size_t a, b, c, d, tot;
    det_ws_layout(R, D, Hd, T, &a, &b, &c, &d, &tot);
    return tot;
}

// the detector's bf16x3 path with both linear layers fused with their LIF (one row tile holds all T steps)
static bool det_b3_tiles(const snn_params* p, const DetWindows& w) {
    return prec_family(p) == SNN_PRECISION_BF16X3 && g3_some_tile_ok(w.fc6.n) && g3_some_tile_ok(w.fc7.n);
}
// ... which takes its encoder planes word-major [T][D/32][R] (and hands fc6's spikes to fc7 that way)
static bool det_planes_wm(const snn_params* p, const DetWindows& w) { return det_b3_tiles(p, w) && knobs().planes != 1; }

// everything a detector head pass is told, whichever exported entry it came through (the entries check what is theirs alone - the step list,
// the pairs that go together, the route - fill one of these and run it)
struct DetCall {
    bool roi_fed;                                              // the feed: rows of typed features x [R][D] (feed_rows) ...
    const void* x; int D;
    const snn_roi_level* levels_host; int n_levels, C;         // ... or RoIAlign over typed level maps, D = 49 C (feed_roialign)
    const float* rois; const int *roi_batch, *roi_level;
    int fdt, R, Hd, K, K4, T;                                  // T: the pass's last step
    const snn_params* p;
    const void* w6_packed; int w6_inner; const void* w7_packed; const float* w_heads_packed;
    float *out_cls, *out_bbox; uint32_t *spk6_count, *spk7_count; float *sum_cls, *sum_bbox;
    void* ws; size_t ws_bytes; snn_stream_t stream;
    // any-time readouts (snn_det_head_forward_readouts): outputs [n][R][K] / [n][R][K4], counts [n][R]; null: one readout at T
    const int* steps; int n_steps;
    SparseRoute route;                                         // of fc6; .gated is the plan's to decide (DetPlan), not the entry's
    const char* who;                                           // the name in messages: the feed's plain entry
};
// what every detector entry is told in the same words; the feed follows
static DetCall det_call(int fdt, int R, int Hd, int K, int K4, int T, const snn_params* p, const void* w6_packed, int w6_inner,
                        const void* w7_packed, const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                        uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes, snn_stream_t stream) {
    DetCall c = {};
    c.fdt = fdt; c.R = R; c.Hd = Hd; c.K = K; c.K4 = K4; c.T = T; c.p = p;
    c.w6_packed = w6_packed; c.w6_inner = w6_inner; c.w7_packed = w7_packed; c.w_heads_packed = w_heads_packed;
    c.out_cls = out_cls; c.out_bbox = out_bbox; c.spk6_count = spk6_count; c.spk7_count = spk7_count; c.sum_cls = sum_cls; c.sum_bbox = sum_bbox;
    c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream;
    c.route = SPARSE_ROUTE;
    return c;
}
static void feed_rows(DetCall& c, const void* x, int D) { c.roi_fed = false; c.x = x; c.D = D; c.who = "snn_det_head_forward"; }
static void feed_roialign(DetCall& c, const snn_roi_level* levels_host, int n_levels, int C, const float* rois, const int* roi_batch,
                          const int* roi_level) {
    c.roi_fed = true; c.levels_host = levels_host; c.n_levels = n_levels; c.C = C; c.rois = rois; c.roi_batch = roi_batch; c.roi_level = roi_level;
    c.who = "snn_det_head_forward_roialign";
}

// the readout entry points' own checks, before those of the pass: the step list, then the arguments that go in pairs
static int det_readouts_check(const char* who, const int* steps, int n, const uint32_t* c6, const uint32_t* c7, const float* sum_cls,
                              const float* sum_bbox) {
    if (check_steps(steps, n, who)) return -1;
    if ((c6 == nullptr) != (c7 == nullptr)) return fail(-1, "%s: spk6_count and spk7_count go together", who);
    if ((sum_cls == nullptr) != (sum_bbox == nullptr)) return fail(-1, "%s: sum_cls and sum_bbox go together", who);
    return 0;
}

// what a detector pass decides before its encoder launch, whichever feed (rows or RoIAlign) it has
struct DetPlan {
    size_t o_enc, o_cur, o_s6, o_s7;     // det_ws_layout
    size_t o_raw;                        // where the unfolded encoder writes: o_enc, or the last region for permuted fc6 weights (det_ws_perm_offset)
    DetWindows win;
    bool wm, per;                        // encoder planes word-major (det_planes_wm); fc6 on the encoder's period planes (snn_common.h)
    bool bin_major;                      // an unfolded encoder already wrote RAW planes in fc6's bin-major order at o_enc (channels-last RoIAlign): no k_permute_planes
    // fc6 route AUTO (snn_det_head_forward_routed): this call enqueues compress + count, the decision and both fc6 launches
    // behind the gate word - where fc6's plan is the sparse launch on bin-major period planes and the call counts no spikes and reads out
    // once; every other configuration runs its plan as it is.  The encoder then leaves every period plane raw (no fold)
    bool gated;
};

// where a detector pass with this plan leaves lif6's / lif7's spike planes (snn_det_head_planes_view; the pass reads its own layout from here).
// Currents of steps t0 .. t0 + n - 1 (zero before t0) form the spikes of steps 0 .. t0 + n
static void det_planes_views(const DetPlan& dp, int R, int Hd, int T, snn_planes_view* v6, snn_planes_view* v7) {
    const int Hw = cdiv(Hd, 32);
    for (int i = 0; i < 2; ++i) {
        snn_planes_view* v = i ? v7 : v6;
        if (!v) continue;
        const StepWindow& w = i ? dp.win.fc7 : dp.win.fc6;
        v->offset_bytes = i ? dp.o_s7 : dp.o_s6; v->step_stride_words = (uint64_t)R * Hw; v->rows = R; v->words = Hw;
        v->layout = (!i && dp.wm) ? SNN_PLANES_WORD_MAJOR : SNN_PLANES_ROWS;          // (fc7's spikes feed the LI heads row-major)
        v->steps_formed = min(T, w.t0 + w.n + 1);
        v->reserved = 0;
    }
}

// will fc6 run the structured-sparse launch on the word-major period planes at o_enc?  fc6's own launcher is asked (nothing is enqueued)
static bool det_fc6_sparse_plan(const DetCall& c, int D, const DetPlan& dp) {
    Gemm3Args a6;
    G3Tile t6;
    return spike_gemm_lif_bf16x3_args((const uint32_t*)((char*)c.ws + dp.o_enc), c.T, c.R, D, c.Hd, c.p, (const uint16_t*)c.w6_packed,
                                      (uint32_t*)((char*)c.ws + dp.o_s6), (size_t)c.R * cdiv(c.Hd, 32), c.spk6_count, true, true, &dp.win.fc6, true,
                                      &a6, &t6) == 0 &&
           gemm3_lif_sparse(a6, false, (char*)c.ws + dp.o_cur, dp.o_s6 - dp.o_cur, (hipStream_t)c.stream, SPARSE_QUERY, c.route, weight_planes(c.p)) == 1;
}

static int det_plan(const DetCall& c, int D, bool wm_ok, DetPlan* dp) {
    size_t need;
    det_ws_layout(c.R, D, c.Hd, c.T, &dp->o_enc, &dp->o_cur, &dp->o_s6, &dp->o_s7, &need);
    if (c.ws_bytes < need) return fail(-2, "%s: workspace %zu < %zu bytes", c.who, c.ws_bytes, need);
    if (check_T(c.T, c.who)) return -1;
    dp->o_raw = c.w6_inner > 1 ? det_ws_perm_offset(c.R, D, c.Hd, c.T) : dp->o_enc;
    dp->bin_major = false;
    dp->win = det_windows(c.p, c.T, c.spk6_count != nullptr);
    dp->wm = det_planes_wm(c.p, dp->win) && wm_ok;
    dp->per = knobs().periods && periods_possible(c.p) && det_b3_tiles(c.p, dp->win);
    dp->gated = c.route.route == SNN_ROUTE_AUTO && c.route.stat && !c.spk6_count && !c.steps && c.w6_inner == 49 && dp->wm && dp->per &&
                det_fc6_sparse_plan(c, D, *dp);
    return 0;
}

// rounds 5 / 6: where fc6 will run the structured-sparse launch on bin-major planes, ONE encoder launch writes them - permuted, e_3 ..
// compressed - instead of encoder + k_permute_planes + k_compress_planes.  fc6's own launcher is asked (nothing is enqueued).  feed_ok:
// the feed's own conditions; *np, *eth: the folded encoder's neuron and threshold table
static bool det_fc6_folds(bool feed_ok, const DetCall& c, int D, const DetPlan& dp, NeuronP* np, const EncTh** eth) {
    if (dp.gated || !knobs().enc_fold || !feed_ok || c.w6_inner != 49 || !dp.wm || !dp.per) return false;      // (the gated fc6 route reads raw planes)
    *np = make_p(c.p, c.p->v_th_enc);
    np->v_fire = ENC_FIRED;
    if (!enc_zero_rest(*np) || enc_mode(*np, eth) != ENC_QUANT) return false;
    return det_fc6_sparse_plan(c, D, dp);
}

// the LI heads at the end of a detector pass: one readout at T (the plain forward), or the readout set with its spike counts
static int det_heads_tail(const DetCall& c, const uint32_t* s6, const uint32_t* s7, bool s6_wm) {
    const int R = c.R, Hw = cdiv(c.Hd, 32);
    if (!c.steps)
        return snn_li_heads(s7, (size_t)R * Hw, c.T, R, c.Hd, c.w_heads_packed, c.K, c.K4, c.p, c.out_cls, c.out_bbox, c.sum_cls, c.sum_bbox, c.stream);
    int rc = li_heads_readouts_impl(s7, (size_t)R * Hw, c.steps, c.n_steps, R, c.Hd, c.w_heads_packed, c.K, c.K4, c.p, c.out_cls, c.out_bbox, c.sum_cls,
                                    c.sum_bbox, false, c.stream);
    if (rc || !c.spk6_count) return rc;
    const StepList st = step_list(c.steps, c.n_steps);
    hipLaunchKernelGGL(k_count_rows_ro, dim3(cdiv(R, 256)), dim3(256), 0, (hipStream_t)c.stream, s6, (unsigned long long)R * Hw, R, Hw, s6_wm ? 1 : 0, st, c.spk6_count);
    SNN_CHECK_LAUNCH("k_count_rows_ro");
    hipLaunchKernelGGL(k_count_rows_ro, dim3(cdiv(R, 256)), dim3(256), 0, (hipStream_t)c.stream, s7, (unsigned long long)R * Hw, R, Hw, 0, st, c.spk7_count);
    SNN_CHECK_LAUNCH("k_count_rows_ro");
    return 0;
}

// route_stat of a routed detector call that did not decide on the device: {0, 0, 0 = the sparse fc6 launch ran (and always in spike-rate
// mode) / 1 = dense, 0}; nothing on every other entry
static int fc6_route_fixed(int32_t* route_stat, int route_taken, hipStream_t s) {
    if (!route_stat) return 0;
    hipLaunchKernelGGL(k_route_decide, dim3(1), dim3(64), 0, s, (int*)route_stat, (const int*)nullptr, 0, 0, 0.0f, route_taken);
    SNN_CHECK_LAUNCH("k_route_decide");
    return 0;
}

// the pass behind its encoder launch, whichever feed wrote the planes: fc6 + LIF, fc7 + LIF, the LI heads
static int det_head_from_planes(const DetCall& c, int D, const DetPlan& dp, bool folded) {
    // folded (round 5): the encoder launch already wrote the planes in fc6's permuted order, e_3 .. compressed (k_encode_rows_perm): no
    // k_permute_planes, no k_compress_planes - fc6 must then run the structured-sparse launch (it was asked beforehand)
    const int R = c.R, Hd = c.Hd, T = c.T, k_inner = c.w6_inner, planes = weight_planes(c.p);
    const snn_params* const p = c.p;
    const void *const w6_packed = c.w6_packed, *const w7_packed = c.w7_packed;
    uint32_t *const spk6_count = c.spk6_count, *const spk7_count = c.spk7_count;
    void* const ws = c.ws;
    const snn_stream_t stream = c.stream;
    const size_t o_enc = dp.o_enc, o_cur = dp.o_cur, o_s6 = dp.o_s6, o_s7 = dp.o_s7;
    SparseRoute rt = c.route;
    rt.gated = dp.gated;
    const DetWindows& win = dp.win;
    const bool enc_wm = dp.wm, enc_periods = dp.per;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* enc = (uint32_t*)((char*)ws + o_enc);
    float* cur = (float*)((char*)ws + o_cur);
    uint32_t* s6 = (uint32_t*)((char*)ws + o_s6);
    uint32_t* s7 = (uint32_t*)((char*)ws + o_s7);
    const int Hw = cdiv(Hd, 32), Hp = Hw * 32;
    snn_planes_view v6, v7;
    det_planes_views(dp, R, Hd, T, &v6, &v7);
    g_last_det_planes[0] = v6.offset_bytes; g_last_det_planes[1] = v7.offset_bytes; g_last_det_planes[2] = v6.layout == SNN_PLANES_WORD_MAJOR ? 1 : 0;
    int rc;
    if (k_inner > 1 && !folded && !dp.bin_major) {
        // fc6's weights were packed in the permuted reduction order k' = s * C + c (snn_pack_linear_weight_bf16x3_perm): bring the
        // encoder's planes into the same order (snn_sparse.h: k_permute_planes).  Word-major planes of the fused bf16x3 layers only.
        const int C = D / k_inner;
        if (D % k_inner || C % 32 || !enc_wm || !det_b3_tiles(p, win))
            return fail(-4, "snn_det_head_forward: permuted fc6 weights (inner = %d) need D = C * inner, C %% 32 == 0 and the fused bf16x3 path", k_inner);
        // (the encoder wrote its planes into the LAST region of the workspace; the permuted ones go to the front, where fc6 reads them -
        // the sparse kernel addresses its side buffers as 32-bit offsets from the planes, so these must lie in front of them)
        const uint32_t* enc_raw = (const uint32_t*)((char*)ws + dp.o_raw);
        const int Dw = cdiv(D, 32);
        if (k_inner != 49) return fail(-4, "snn_det_head_forward: permuted fc6 weights: inner = %d (only 49 = 7 x 7 bins is built)", k_inner);
        hipLaunchKernelGGL(k_permute_planes<49>, dim3(cdiv(R, 32), win.enc_steps), dim3(256), 0, s, enc_raw, enc, Dw, R, C);
        SNN_CHECK_LAUNCH("k_permute_planes");
    }
    if (spk6_count) { if (hipMemsetAsync(spk6_count, 0, sizeof(uint32_t) * R, s) != hipSuccess) return fail(-3, "hipMemsetAsync failed"); }
    if (spk7_count) { if (hipMemsetAsync(spk7_count, 0, sizeof(uint32_t) * R, s) != hipSuccess) return fail(-3, "hipMemsetAsync failed"); }
    const bool b3 = prec_family(p) == SNN_PRECISION_BF16X3, mx = prec_family(p) == SNN_PRECISION_MXFP6;
    if (prec_family(p) != SNN_PRECISION_F32 && !b3 && !mx) return fail(-1, "snn_det_head_forward: unknown precision %d", p->precision);
    if (mx) {
        if (D % 128 || Hd % 128)
            return fail(-4, "snn_det_head_forward: the mxfp6 kernels need D, Hd %% 128 == 0");
        // (spike-rate mode: per-RoI counts come out of the LIF epilogues)
        if (!mx_tile_ok(win.fc6.n) || !mx_tile_ok(win.fc7.n)) return fail(-4, "snn_det_head_forward: T=%d does not fit a 512-row tile of the mxfp6 kernels", T);
        if ((rc = fc6_route_fixed(rt.stat, spk6_count ? 0 : 1, s))) return rc;
        if ((rc = spike_gemm_lif_mx_impl(enc, T, R, D, Hd, p, (const uint32_t*)w6_packed, s6, (size_t)R * Hw, spk6_count, stream, &win.fc6))) return rc;
        if ((rc = spike_gemm_lif_mx_impl(s6, T, R, Hd, Hd, p, (const uint32_t*)w7_packed, s7, (size_t)R * Hw, spk7_count, stream, &win.fc7))) return rc;
        return det_heads_tail(c, s6, s7, false);
    }
    if ((enc_wm || enc_periods) && !det_b3_tiles(p, win)) return fail(-1, "snn_det_head_forward: word-major / period planes without the fused bf16x3 layers");
    if (det_b3_tiles(p, win)) {
        // fc6 + LIF and fc7 + LIF, each one launch: a row tile holds all T steps of its RoIs, the currents never
        // leave the chip (faster_rcnn.py:498-501)
        // (spike-rate mode: per-RoI counts come out of the LIF epilogues)
        // (word-major planes between the stages: encoder -> fc6 -> fc7; fc7's spikes feed the LI heads row-major)
        // (dead time steps, lif_windows: fc6 forms the currents of steps 0 .. T-3, fc7 of steps 1 .. T-2)
        Gemm3Args a6, a7;
        G3Tile t6, t7;
        if ((rc = spike_gemm_lif_bf16x3_args(enc, T, R, D, Hd, p, (const uint16_t*)w6_packed, s6, (size_t)R * Hw, spk6_count, enc_wm, enc_wm, &win.fc6, enc_periods, &a6, &t6))) return rc;
        if ((rc = spike_gemm_lif_bf16x3_args(s6, T, R, Hd, Hd, p, (const uint16_t*)w7_packed, s7, (size_t)R * Hw, spk7_count, enc_wm, false, &win.fc7, false, &a7, &t7))) return rc;
        const int wn = g3_wn();
        // round 4: fc6's sparse period planes e_3 .. on the structured-sparse matrix-core instruction (snn_sparse.h); its side buffers
        // live in the currents region of the workspace, which the fused layers never write
        rc = gemm3_lif_sparse(a6, false, (char*)ws + o_cur, o_s6 - o_cur, s, folded ? SPARSE_RUN_COMPRESSED : SPARSE_RUN, rt, planes);
        if (rc < 0) return rc;
        if (folded && rc != 1) return fail(-3, "snn_det_head_forward: the encoder wrote compressed planes but fc6 takes the dense launch (internal)");
        if (rt.gated && rc != 2) return fail(-3, "snn_det_head_forward: fc6 route: the gated pair was planned but fc6 did not enqueue it (internal)");
        g_last_fc_sparse = rc;
        if (rc == 2) { a6.gate = (const int*)rt.stat + 2; a6.gate_want = 1; }      // the gated route: the dense launch on the same raw planes and weights, behind the same word
        else if ((rc = fc6_route_fixed(rt.stat, (spk6_count || rc == 1) ? 0 : 1, s))) return rc;
        if (g_last_fc_sparse != 1 && (rc = launch_gemm3(G3_FC_LIF_TILE, t6.mt, wn, a6, planes, s))) return rc;
        if ((rc = launch_gemm3(G3_FC_LIF_TILE, t7.mt, wn, a7, planes, s))) return rc;
        return det_heads_tail(c, s6, s7, enc_wm);
    }
    // fc6 for all (live) time steps at once: rows m = (t - t0)*R + r   (faster_rcnn.py:498)
    if ((rc = fc6_route_fixed(rt.stat, spk6_count ? 0 : 1, s))) return rc;
    const uint32_t* a6 = enc + (size_t)win.fc6.t0 * R * cdiv(D, 32);
    rc = b3 ? spike_gemm_bf16x3_impl(a6, win.fc6.n * R, D, Hd, (const uint16_t*)w6_packed, cur, Hp, planes, stream)
            : snn_spike_gemm(a6, win.fc6.n * R, D, Hd, (const float*)w6_packed, cur, Hp, stream);
    if (rc) return rc;
    if ((rc = lif_scan_window(cur, T, win.fc6, R, Hd, Hp, p, s6, (size_t)R * Hw, spk6_count, stream))) return rc;   // :499
    const uint32_t* a7 = s6 + (size_t)win.fc7.t0 * R * Hw;
    rc = b3 ? spike_gemm_bf16x3_impl(a7, win.fc7.n * R, Hd, Hd, (const uint16_t*)w7_packed, cur, Hp, planes, stream)
            : snn_spike_gemm(a7, win.fc7.n * R, Hd, Hd, (const float*)w7_packed, cur, Hp, stream);                       // :500
    if (rc) return rc;
    if ((rc = lif_scan_window(cur, T, win.fc7, R, Hd, Hp, p, s7, (size_t)R * Hw, spk7_count, stream))) return rc;   // :501
    return det_heads_tail(c, s6, s7, false);                                                             // :505-510
}

// the rows feed behind the plan: what it asks of the plan, then its encoder launch - folded (k_encode_rows_perm) or encode_rows_impl
static int det_encode_rows(const DetCall& c, const DetPlan& dp, bool* folded) {
    const void* const x = c.x;
    const int R = c.R, D = c.D;
    if (c.w6_inner > 1 && !dp.wm) return fail(-4, "snn_det_head_forward: permuted fc6 weights need the word-major fused bf16x3 path (D %% 32 == 0, x 16-byte aligned)");
    NeuronP np;
    const EncTh* eth_f = nullptr;
    const bool fold = *folded = det_fc6_folds(D % (49 * 64) == 0, c, D, dp, &np, &eth_f);
    if (fold) {
        const int Te = dp.win.enc_steps, C = D / 49;
        const int rb = knobs().encp_rb ? (knobs().encp_rb == 16 ? 16 : 8) : (Te <= ENCP_LDS_WORDS / (2 * 49 * 16) ? 16 : 8);     // (one pass through LDS where 16 RoIs per block allow it)
        const size_t lds = (size_t)min(Te, ENCP_LDS_WORDS / (2 * 49 * rb)) * 2 * 49 * rb * 4;
        // eight waves per block where only two blocks fit a CU's LDS (T_det = 12: -2 us, T_det = 24: -10 us), four where three fit (T_det = 16: eight
        // were 9 us slower) - profiles/r5_encoder_nw_ab.txt
        const int nw = knobs().encp_nw ? (knobs().encp_nw == 4 ? 4 : 8) : (lds > 53 * 1024 ? 8 : 4);
        const void* kern = encode_rows_perm_kernel(rb, nw, c.fdt);
        g_last_enc_mode = ENC_QUANT;                            // (det_fc6_folds: the folded encoder exists in the threshold form only)
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(-3, "hipFuncSetAttribute failed: %s", hipGetErrorString(e));
        uint32_t* planes_f = (uint32_t*)((char*)c.ws + dp.o_enc);
        uint32_t* cmp_f = (uint32_t*)((char*)c.ws + dp.o_cur);
        const int nd_f = 2;
        void* kargs[] = {(void*)&x, (void*)&R, (void*)&C, (void*)&Te, (void*)&nd_f, (void*)eth_f, (void*)&planes_f, (void*)&cmp_f};
        e = hipLaunchKernel(kern, dim3(cdiv(R, rb), C / 64), dim3(64 * nw), kargs, lds, (hipStream_t)c.stream);
        if (e != hipSuccess) return fail(-3, "k_encode_rows_perm launch failed: %s", hipGetErrorString(e));
        SNN_CHECK_LAUNCH("k_encode_rows_perm");
        return 0;
    }
    // (SNN_STATUS_NO_TYPED_KERNEL included: nothing has been enqueued)
    return encode_rows_impl(x, R, D, dp.win.enc_steps, c.p, (uint32_t*)((char*)c.ws + dp.o_raw), (size_t)R * cdiv(D, 32), dp.wm, c.stream, dp.per, c.fdt);
}

// the RoIAlign feed behind the plan: what it asks of the plan and of its maps, then its encoder launch - k_roi_align_encode_perm (folded, or
// channels-last maps) or roi_align_encode_impl
static int det_encode_roialign(const DetCall& c, int D, DetPlan& dp, bool* folded) {
    const snn_roi_level* const levels_host = c.levels_host;
    const int fdt = c.fdt, n_levels = c.n_levels, C = c.C, R = c.R;
    if (c.w6_inner > 1 && (!dp.wm || c.w6_inner != 49)) return fail(-4, "snn_det_head_forward_roialign: permuted fc6 weights need inner = 49 and the word-major fused bf16x3 path");
    // the feature dtype / layout code and every level's base pointer, once, before anything is asked of fc6 or enqueued
    if (check_feat(nullptr, fdt, "snn_det_head_forward_roialign")) return -1;
    for (int l = 0; levels_host && n_levels <= 4 && l < n_levels; ++l)
        if (check_feat(levels_host[l].feat, fdt, "snn_det_head_forward_roialign")) return -1;
    // round 6: the RoIAlign encoder folds as the row encoder does since round 5 (k_roi_align_encode_perm).
    // Planned for windows of up to 12 planes (T_det <= 14): measured on the bench's pyramid, 2000 RoIs (profiles/r6_roi_fold_ab.txt, same lease) the fused
    // head takes 0.943 against 0.948 ms at T_det = 12 - the launch itself is 30 us slower than the table kernel (7 of 8 lanes per bin row, a second
    // pass that transposes the ballots) and saves k_permute_planes + k_compress_planes (38 us) and their two 31-MB plane copies - but 2.04 against
    // 1.88 ms at T_det = 24, where its 44 KB of LDS leave three work-groups per CU to a launch that lives on loads in flight.
    bool feed_geo = knobs().roi_tab && C % 64 == 0 && levels_host && c.rois && c.roi_batch && c.roi_level && n_levels > 0 && n_levels <= 4;
    for (int l = 0; l < n_levels && feed_geo; ++l)
        feed_geo = levels_host[l].feat && levels_host[l].H > 0 && levels_host[l].W >= 2 && (long long)C * levels_host[l].H * levels_host[l].W < (1ll << 29);
    const bool feed_ok = feed_geo && dp.win.enc_steps <= 12;
    NeuronP np;
    const EncTh* eth_f = nullptr;
    const bool fold = *folded = det_fc6_folds(feed_ok, c, D, dp, &np, &eth_f);
    // channels-last maps (SNN_FEAT_NHWC): one kernel, for the plans in which fc6 reads bin-major period planes - folded as above, or (longer windows,
    // a dense fc6) every plane raw in bin-major order where k_permute_planes would have put it, k_compress_planes following as before
    const bool nhwc = (fdt & SNN_FEAT_NHWC) != 0;
    bool nhwc_raw = false;
    if (nhwc && !fold) {
        nhwc_raw = feed_geo && c.w6_inner == 49 && dp.wm && dp.per;
        if (nhwc_raw) {
            np = make_p(c.p, c.p->v_th_enc);
            np.v_fire = ENC_FIRED;
            nhwc_raw = enc_zero_rest(np) && enc_mode(np, &eth_f) == ENC_QUANT;
        }
        if (!nhwc_raw) return SNN_STATUS_NO_TYPED_KERNEL;       // (nothing has been enqueued)
    }
    if (fold || nhwc_raw) {
        constexpr int RW = 4;
        RoiArgs fa;
        memset(&fa, 0, sizeof(fa));
        for (int l = 0; l < n_levels; ++l) {
            fa.lv[l].feat = levels_host[l].feat; fa.lv[l].H = levels_host[l].H; fa.lv[l].W = levels_host[l].W; fa.lv[l].scale = levels_host[l].spatial_scale;
        }
        fa.p = np; fa.quant = 1; fa.eth = *eth_f;
        fa.rois = c.rois; fa.roi_batch = c.roi_batch; fa.roi_level = c.roi_level;
        fa.planes = (uint32_t*)((char*)c.ws + dp.o_enc); fa.cmp = fold ? (uint32_t*)((char*)c.ws + dp.o_cur) : nullptr; fa.nd = 2;
        fa.plane_stride = (unsigned long long)R * cdiv(D, 32); fa.R = R; fa.C = C; fa.T = dp.win.enc_steps; fa.Dw = cdiv(D, 32);
        fa.RW = RW; fa.n_rg = cdiv(R, 4 * RW);
        const int n_cp = C / 64, n_items = fa.n_rg * 7;
        const int grid = (8 % n_cp == 0) ? 8 * cdiv(n_items, 8 / n_cp) : n_cp * n_items;
        const size_t lds = (size_t)fa.T * (nhwc ? 7 : 7 + 8) * 4 * RW * 8;       // word pairs + raw ballots (channels-last: word pairs only)
        g_last_enc_mode = ENC_QUANT;
        launch_picked(roi_align_encode_perm_kernel<RW>(fdt), dim3(grid), dim3(256), lds, (hipStream_t)c.stream, fa);
        SNN_CHECK_LAUNCH("k_roi_align_encode_perm");
        dp.bin_major = nhwc_raw;
        return 0;
    }
    // (SNN_STATUS_NO_TYPED_KERNEL included: nothing has been enqueued)
    return roi_align_encode_impl(levels_host, n_levels, C, c.rois, c.roi_batch, c.roi_level, R, dp.win.enc_steps, c.p,
                                 (uint32_t*)((char*)c.ws + dp.o_raw), (size_t)R * cdiv(D, 32), nullptr, dp.wm, c.stream, dp.per, fdt);
}

// the detector head: the checks and the plan both feeds share, the feed's encoder launch, then fc6, fc7 and the LI heads
static int det_head_run(const DetCall& c) {
    if ((!c.roi_fed && !c.x) || !c.p || !c.w6_packed || !c.w7_packed || !c.w_heads_packed || !c.out_cls || !c.out_bbox || !c.ws)
        return fail(-1, "%s: null argument", c.who);
    if (c.R <= 0 || (c.roi_fed ? c.C : c.D) <= 0 || c.Hd <= 0 || c.K <= 0 || c.K4 <= 0) return fail(-1, "%s: bad shape", c.who);
    const int D = c.roi_fed ? c.C * 49 : c.D;
    // (the row-fed entry points check T before the workspace, and their feature code before the plan)
    if (!c.roi_fed && (check_T(c.T, c.who) || check_feat_rows(c.x, c.fdt, c.who))) return -1;
    DetPlan dp;
    int rc;
    if ((rc = det_plan(c, D, c.roi_fed || encode_rows_wm_ok(c.x, D), &dp))) return rc;
    bool folded = false;
    if ((rc = c.roi_fed ? det_encode_roialign(c, D, dp, &folded) : det_encode_rows(c, dp, &folded))) return rc;
    return det_head_from_planes(c, D, dp, folded);
}

int snn_det_head_forward(const float* x, int R, int D, int Hd, int K, int K4, int T, const snn_params* p,
                         const void* w6_packed, const void* w7_packed, const float* w_heads_packed,
                         float* out_cls, float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count,
                         float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes, snn_stream_t stream) {
    return snn_det_head_forward_k_typed(x, SNN_FEAT_F32, R, D, Hd, K, K4, T, p, w6_packed, 0, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count,
                                        spk7_count, sum_cls, sum_bbox, ws, ws_bytes, stream);
}

int snn_det_head_forward_k(const float* x, int R, int D, int Hd, int K, int K4, int T, const snn_params* p,
                           const void* w6_packed, int w6_inner, const void* w7_packed, const float* w_heads_packed,
                           float* out_cls, float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count,
                           float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes, snn_stream_t stream) {
    return snn_det_head_forward_k_typed(x, SNN_FEAT_F32, R, D, Hd, K, K4, T, p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox,
                                        spk6_count, spk7_count, sum_cls, sum_bbox, ws, ws_bytes, stream);
}

int snn_det_head_forward_k_typed(const void* x, int fdt, int R, int D, int Hd, int K, int K4, int T, const snn_params* p,
                                 const void* w6_packed, int w6_inner, const void* w7_packed, const float* w_heads_packed,
                                 float* out_cls, float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count,
                                 float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes, snn_stream_t stream) {
    DetCall c = det_call(fdt, R, Hd, K, K4, T, p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls,
                         sum_bbox, ws, ws_bytes, stream);
    feed_rows(c, x, D);
    return det_head_run(c);
}

// spike-rate readouts: the pass runs as a spike-rate forward at T (same launches, windows of every lif6 step); its per-RoI counts land in
// the first rows of the count buffers, which the readout counts then overwrite in stream order
int snn_det_head_forward_readouts(const float* x, int R, int D, int Hd, int K, int K4, const int* steps, int n_steps, const snn_params* p,
                                  const void* w6_packed, int w6_inner, const void* w7_packed, const float* w_heads_packed,
                                  float* out_cls, float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count,
                                  float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes, snn_stream_t stream) {
    return snn_det_head_forward_readouts_typed(x, SNN_FEAT_F32, R, D, Hd, K, K4, steps, n_steps, p, w6_packed, w6_inner, w7_packed, w_heads_packed,
                                               out_cls, out_bbox, spk6_count, spk7_count, sum_cls, sum_bbox, ws, ws_bytes, stream);
}

int snn_det_head_forward_readouts_typed(const void* x, int fdt, int R, int D, int Hd, int K, int K4, const int* steps, int n_steps,
                                        const snn_params* p, const void* w6_packed, int w6_inner, const void* w7_packed,
                                        const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                        uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes, snn_stream_t stream) {
    if (det_readouts_check("snn_det_head_forward_readouts", steps, n_steps, spk6_count, spk7_count, sum_cls, sum_bbox)) return -1;
    DetCall c = det_call(fdt, R, Hd, K, K4, steps[n_steps - 1], p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls,
                         sum_bbox, ws, ws_bytes, stream);
    feed_rows(c, x, D);
    c.steps = steps; c.n_steps = n_steps;
    return det_head_run(c);
}

int snn_det_head_forward_roialign(const snn_roi_level* levels_host, int n_levels, int C, const float* rois,
                                  const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                  const snn_params* p, const void* w6_packed, const void* w7_packed,
                                  const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                  uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes,
                                  snn_stream_t stream) {
    return snn_det_head_forward_roialign_k_typed(levels_host, SNN_FEAT_F32, n_levels, C, rois, roi_batch, roi_level, R, Hd, K, K4, T, p, w6_packed, 0,
                                                 w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls, sum_bbox, ws,
                                                 ws_bytes, stream);
}

int snn_det_head_forward_roialign_k(const snn_roi_level* levels_host, int n_levels, int C, const float* rois,
                                    const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                    const snn_params* p, const void* w6_packed, int w6_inner, const void* w7_packed,
                                    const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                    uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes,
                                    snn_stream_t stream) {
    return snn_det_head_forward_roialign_k_typed(levels_host, SNN_FEAT_F32, n_levels, C, rois, roi_batch, roi_level, R, Hd, K, K4, T, p, w6_packed,
                                                 w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls, sum_bbox,
                                                 ws, ws_bytes, stream);
}

int snn_det_head_forward_roialign_k_typed(const snn_roi_level* levels_host, int fdt, int n_levels, int C, const float* rois,
                                          const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                          const snn_params* p, const void* w6_packed, int w6_inner, const void* w7_packed,
                                          const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                          uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes,
                                          snn_stream_t stream) {
    DetCall c = det_call(fdt, R, Hd, K, K4, T, p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls,
                         sum_bbox, ws, ws_bytes, stream);
    feed_roialign(c, levels_host, n_levels, C, rois, roi_batch, roi_level);
    return det_head_run(c);
}

int snn_det_head_forward_roialign_readouts(const snn_roi_level* levels_host, int n_levels, int C, const float* rois,
                                           const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, const int* steps,
                                           int n_steps, const snn_params* p, const void* w6_packed, int w6_inner, const void* w7_packed,
                                           const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                           uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes,
                                           snn_stream_t stream) {
    return snn_det_head_forward_roialign_readouts_typed(levels_host, SNN_FEAT_F32, n_levels, C, rois, roi_batch, roi_level, R, Hd, K, K4, steps,
                                                        n_steps, p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count,
                                                        spk7_count, sum_cls, sum_bbox, ws, ws_bytes, stream);
}

int snn_det_head_forward_roialign_readouts_typed(const snn_roi_level* levels_host, int fdt, int n_levels, int C, const float* rois,
                                                 const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, const int* steps,
                                                 int n_steps, const snn_params* p, const void* w6_packed, int w6_inner, const void* w7_packed,
                                                 const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                                 uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes,
                                                 snn_stream_t stream) {
    if (det_readouts_check("snn_det_head_forward_roialign_readouts", steps, n_steps, spk6_count, spk7_count, sum_cls, sum_bbox)) return -1;
    DetCall c = det_call(fdt, R, Hd, K, K4, steps[n_steps - 1], p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls,
                         sum_bbox, ws, ws_bytes, stream);
    feed_roialign(c, levels_host, n_levels, C, rois, roi_batch, roi_level);
    c.steps = steps; c.n_steps = n_steps;
    return det_head_run(c);
}

// ---- fc6 route of the detector head ----
// the routed forward's workspace: the plain forward's.  Its front region holds the raw bin-major planes of every period, the currents region the
// compressed planes and the hit counters; the gate word is route_stat[2], in the caller's array
size_t snn_det_head_workspace_bytes_routed(int R, int D, int Hd, int K, int K4, int T, int precision, int route) {
    if (!route_known(route)) return 0;
    return snn_det_head_workspace_bytes(R, D, Hd, K, K4, T, precision);
}


int snn_det_head_forward_routed(const void* x, int fdt, int R, int D, int Hd, int K, int K4, int T, const snn_params* p,
                                const void* w6_packed, int w6_inner, const void* w7_packed, const float* w_heads_packed,
                                float* out_cls, float* out_bbox, uint32_t* spk6_count, uint32_t* spk7_count,
                                float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes, int route, float crossover,
                                int32_t* route_stat, snn_stream_t stream) {
    const size_t need = p ? snn_det_head_workspace_bytes_routed(R, D, Hd, K, K4, T, p->precision, route) : 0;      // (no p: the pass's own message)
    if (route_check("snn_det_head_forward_routed", route, crossover, route_stat, ws_bytes, need)) return -1;
    DetCall c = det_call(fdt, R, Hd, K, K4, T, p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls,
                         sum_bbox, ws, ws_bytes, stream);
    feed_rows(c, x, D);
    c.route = routed(route, crossover, route_stat, spk6_count != nullptr);
    return det_head_run(c);
}

int snn_det_head_forward_roialign_routed(const snn_roi_level* levels_host, int fdt, int n_levels, int C, const float* rois,
                                         const int* roi_batch, const int* roi_level, int R, int Hd, int K, int K4, int T,
                                         const snn_params* p, const void* w6_packed, int w6_inner, const void* w7_packed,
                                         const float* w_heads_packed, float* out_cls, float* out_bbox, uint32_t* spk6_count,
                                         uint32_t* spk7_count, float* sum_cls, float* sum_bbox, void* ws, size_t ws_bytes,
                                         int route, float crossover, int32_t* route_stat, snn_stream_t stream) {
    const size_t need = p ? snn_det_head_workspace_bytes_routed(R, C > 0 && C < (1 << 24) ? C * 49 : 0, Hd, K, K4, T, p->precision, route) : 0;
    if (route_check("snn_det_head_forward_roialign_routed", route, crossover, route_stat, ws_bytes, need)) return -1;
    DetCall c = det_call(fdt, R, Hd, K, K4, T, p, w6_packed, w6_inner, w7_packed, w_heads_packed, out_cls, out_bbox, spk6_count, spk7_count, sum_cls,
                         sum_bbox, ws, ws_bytes, stream);
    feed_roialign(c, levels_host, n_levels, C, rois, roi_batch, roi_level);
    c.route = routed(route, crossover, route_stat, spk6_count != nullptr);
    return det_head_run(c);
}

int snn_det_exchange_payload(const float* class_logits, const float* box_regression, int N, int rois_per_image, int K,
                             int max_det, float* payload, int* counts, snn_stream_t s) {
    if (!class_logits || !box_regression || !payload || !counts || N <= 0 || rois_per_image <= 0 || K < 2 || max_det <= 0)
        return fail(-1, "snn_det_exchange_payload: bad argument");
    if (rois_per_image > 4096 || K > 0xFFFF) return fail(-4, "snn_det_exchange_payload: %d RoIs per image (max 4096)", rois_per_image);
    int npad = 64;
    while (npad < rois_per_image) npad <<= 1;
    if (npad <= 1024)
        hipLaunchKernelGGL(k_det_payload<1>, dim3(N), dim3(npad), (size_t)npad * 8, (hipStream_t)s, class_logits,
                           box_regression, rois_per_image, K, max_det, npad, payload, counts);
    else
        hipLaunchKernelGGL(k_det_payload<4>, dim3(N), dim3(1024), (size_t)npad * 8, (hipStream_t)s, class_logits,
                           box_regression, rois_per_image, K, max_det, npad, payload, counts);
    SNN_CHECK_LAUNCH("k_det_payload");
    return 0;
}

// ---- spike taps (kernels: snn_taps.h) ----
static_assert(SNN_PLANES_ROWS == TAP_LAYOUT_ROWS && SNN_PLANES_SPLIT4 == TAP_LAYOUT_SPLIT4 && SNN_PLANES_WORD_MAJOR == TAP_LAYOUT_WORD_MAJOR,
              "snn_taps.h addresses the layouts of include/snn_hip.h");

// host-only: the plan code of rpn_head_run answers (rpn_ws_layout, rpn_planes_view), nothing is enqueued
int snn_rpn_head_planes_view(const snn_rpn_level* lv, int n_levels, int C, int A, int T, const snn_params* p, int route, int spike_rates,
                             snn_planes_view* shared_lif) {
    (void)spike_rates;                               // (the shared LIF's planes are the same with and without the side outputs)
    if (!lv || !p || !shared_lif) return fail(-1, "snn_rpn_head_planes_view: null argument");
    if (n_levels <= 0 || n_levels > SNN_MAX_LEVELS || C <= 0 || A <= 0) return fail(-1, "snn_rpn_head_planes_view: bad n_levels / C / A");
    if (!route_known(route)) return fail(-1, "snn_rpn_head_planes_view: unknown route %d", route);
    if (prec_family(p) != SNN_PRECISION_F32 && prec_family(p) != SNN_PRECISION_BF16X3 && prec_family(p) != SNN_PRECISION_MXFP6)
        return fail(-1, "snn_rpn_head_planes_view: unknown precision %d", p->precision);
    if (check_T(T, "snn_rpn_head_planes_view")) return -1;
    for (int l = 0; l < n_levels; ++l)
        if (lv[l].N <= 0 || lv[l].H <= 0 || lv[l].W <= 0) return fail(-1, "snn_rpn_head_planes_view: bad level %d", l);
    const long long P = rpn_positions(lv, n_levels, nullptr);
    size_t o_spk, o_cur, o_cnt, need;
    rpn_ws_layout(P, prec_family(p) != SNN_PRECISION_F32 ? rpn_positions_padded(lv, n_levels) : 0, C, T, prec_family(p), &o_spk, &o_cur, &o_cnt, &need);
    rpn_planes_view(p, P, C, A, T, o_spk, shared_lif);
    return 0;
}

// host-only: det_plan answers (the plan of det_head_run for both feeds; a row-fed x is taken as 16-byte aligned), nothing is enqueued
int snn_det_head_planes_view(int R, int D, int Hd, int K, int K4, int T, const snn_params* p, int w6_inner, int route, int spike_rates,
                             snn_planes_view* lif6, snn_planes_view* lif7) {
    if (!p || (!lif6 && !lif7)) return fail(-1, "snn_det_head_planes_view: null argument");
    if (R <= 0 || D <= 0 || Hd <= 0 || K <= 0 || K4 <= 0) return fail(-1, "snn_det_head_planes_view: bad shape");
    if (!route_known(route)) return fail(-1, "snn_det_head_planes_view: unknown route %d", route);
    if (prec_family(p) != SNN_PRECISION_F32 && prec_family(p) != SNN_PRECISION_BF16X3 && prec_family(p) != SNN_PRECISION_MXFP6)
        return fail(-1, "snn_det_head_planes_view: unknown precision %d", p->precision);
    uint32_t counted = 0;                            // (the plan asks only whether the side outputs are there)
    DetCall c = det_call(SNN_FEAT_F32, R, Hd, K, K4, T, p, nullptr, w6_inner, nullptr, nullptr, nullptr, nullptr, spike_rates ? &counted : nullptr,
                         spike_rates ? &counted : nullptr, nullptr, nullptr, nullptr, ~(size_t)0, nullptr);
    feed_rows(c, nullptr, D);
    c.who = "snn_det_head_planes_view";
    c.route = routed(route, 0.0f, nullptr, spike_rates != 0);       // (no route_stat: nothing is gated - the gate moves no spike plane)
    DetPlan dp;
    const int rc = det_plan(c, D, encode_rows_wm_ok(nullptr, D), &dp);
    if (rc) return rc;
    det_planes_views(dp, R, Hd, T, lif6, lif7);
    return 0;
}

// what the three taps check of their view; -> the kernels' form of it
static int tap_view(const char* who, const void* ws, const snn_planes_view* v, int T, TapView* out) {
    if (!ws || !v) return fail(-1, "%s: null workspace or view", who);
    if (v->layout != SNN_PLANES_ROWS && v->layout != SNN_PLANES_SPLIT4 && v->layout != SNN_PLANES_WORD_MAJOR)
        return fail(-1, "%s: unknown plane layout %d", who, v->layout);
    if (v->rows <= 0 || v->rows > 0x7fffffffLL || v->words <= 0 || v->words > TAP_MAX_WORDS || (v->layout == SNN_PLANES_SPLIT4 && v->words % 4) ||
        v->offset_bytes % 4 || v->step_stride_words < (uint64_t)v->rows * v->words)
        return fail(-1, "%s: bad view (1 <= rows < 2^31, 1 <= words <= %d - a multiple of 4 in blocks of four -, a step stride of at least rows x words)", who, TAP_MAX_WORDS);
    if (v->steps_formed < 1 || v->steps_formed > SNN_MAX_STEPS) return fail(-1, "%s: steps_formed = %d outside [1, %d]", who, v->steps_formed, SNN_MAX_STEPS);
    if (T < 1 || T > v->steps_formed) return fail(-1, "%s: %d steps asked of a view whose pass forms %d", who, T, v->steps_formed);
    out->planes = (const uint32_t*)((const char*)ws + v->offset_bytes);
    out->step_stride = v->step_stride_words; out->rows = v->rows; out->words = v->words; out->layout = v->layout;
    return 0;
}

int snn_planes_counts(const void* ws, const snn_planes_view* view, const int64_t* group_row_start, int n_groups, int n_cols, int T,
                      unsigned long long* per_step, uint32_t* per_col, uint32_t* per_row, snn_stream_t stream) {
    TapView v;
    if (tap_view("snn_planes_counts", ws, view, T, &v)) return -1;
    if (!group_row_start || n_groups < 1 || n_groups > TAP_MAX_GROUPS) return fail(-1, "snn_planes_counts: 1 .. %d groups", TAP_MAX_GROUPS);
    if (n_cols < 1 || n_cols > 32 * v.words) return fail(-1, "snn_planes_counts: n_cols = %d outside 1 .. 32 x words = %d", n_cols, 32 * v.words);
    TapGroups g;
    g.n = n_groups;
    long long most = 0;
    for (int i = 0; i <= n_groups; ++i) {
        const long long r = group_row_start[i];
        if (r < 0 || r > v.rows || (i && r < group_row_start[i - 1]))
            return fail(-1, "snn_planes_counts: group_row_start[%d] = %lld (non-decreasing values in 0 .. rows = %lld)", i, r, v.rows);
        if (i) most = max(most, r - group_row_start[i - 1]);
        g.start[i] = (int)r;
    }
    hipStream_t s = (hipStream_t)stream;
    if (!per_step && !per_col && !per_row) return 0;
    const size_t n_step = (size_t)T * n_groups, n_col = (size_t)n_groups * n_cols, n_row = (size_t)v.rows;
    hipLaunchKernelGGL(k_planes_clear, dim3(min(cdiv((long long)max(n_step, max(n_col, n_row)), 256), 1024)), dim3(256), 0, s, per_step, n_step, per_col,
                       n_col, per_row, n_row);
    SNN_CHECK_LAUNCH("k_planes_clear");
    if (!most) return 0;
    hipLaunchKernelGGL(k_planes_counts, dim3(min(cdiv(most, TAP_ROWS), 1024), n_groups), dim3(256), TAP_COUNTS_LDS(v.words), s, v, g, n_cols, T,
                       per_step, per_col, per_row);
    SNN_CHECK_LAUNCH("k_planes_counts");
    return 0;
}

int snn_planes_raster_nchw(const void* ws, const snn_planes_view* view, int64_t row0, int N, int C, int H, int W, int T, uint8_t* out,
                           snn_stream_t stream) {
    TapView v;
    if (tap_view("snn_planes_raster_nchw", ws, view, T, &v)) return -1;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || C > 32 * v.words || (long long)H * W > 0x7fffffffLL || (long long)T * N > 65535)
        return fail(-1, "snn_planes_raster_nchw: bad shape (C <= 32 x words = %d, T' x N <= 65535)", 32 * v.words);
    const long long HW = (long long)H * W;
    if (row0 < 0 || row0 + N * HW > v.rows) return fail(-1, "snn_planes_raster_nchw: rows %lld .. %lld outside the view's %lld", (long long)row0, (long long)row0 + N * HW, v.rows);
    if (!out) return 0;
    const int vec = HW % 16 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(k_planes_raster_nchw, dim3(cdiv(HW, TAP_ROWS), cdiv(cdiv(C, 32), TAP_TW), T * N), dim3(256), 0, (hipStream_t)stream, v,
                       (long long)row0, N, C, (int)HW, out, vec);
    SNN_CHECK_LAUNCH("k_planes_raster_nchw");
    return 0;
}

int snn_planes_raster_rows(const void* ws, const snn_planes_view* view, int n_cols, int T, uint8_t* out, snn_stream_t stream) {
    TapView v;
    if (tap_view("snn_planes_raster_rows", ws, view, T, &v)) return -1;
    if (n_cols < 1 || n_cols > 32 * v.words) return fail(-1, "snn_planes_raster_rows: n_cols = %d outside 1 .. 32 x words = %d", n_cols, 32 * v.words);
    if (!out) return 0;
    const int vec = n_cols % 16 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(k_planes_raster_rows, dim3(cdiv(v.rows, TAP_ROWS), cdiv(cdiv(n_cols, 32), TAP_TW), T), dim3(256), 0, (hipStream_t)stream, v,
                       n_cols, out, vec);
    SNN_CHECK_LAUNCH("k_planes_raster_rows");
    return 0;
}

// ---- readout weight gradients (kernels: snn_wgrad.h) ----
static int wgrad_shape_ok(long long rows, int n_cols, int NA, int NB) {
    return rows >= 1 && rows <= 0x7fffffffLL && n_cols >= 1 && n_cols <= 32 * TAP_MAX_WORDS && NA >= 0 && NB >= 0 && NA + NB >= 1 && NA + NB <= WG_MAX_OUT;
}
// row slabs of a call: every slab owns at least one tile
static int wgrad_slabs(long long rows) { return (int)min((rows + WG_ROWS - 1) / WG_ROWS, (long long)WG_MAX_SLABS); }

size_t snn_li_heads_wgrad_workspace_bytes(int64_t rows, int n_cols, int NA, int NB) {
    if (!wgrad_shape_ok(rows, n_cols, NA, NB)) return 0;
    return (size_t)wgrad_slabs(rows) * (size_t)(NA + NB) * (size_t)n_cols * sizeof(float);
}

int snn_li_heads_wgrad(const void* planes, const snn_planes_view* view, int n_cols, int T_prime, const snn_params* p, const float* grad_a,
                       const float* grad_b, int NA, int NB, float* gw_a, float* gw_b, int accumulate, void* scratch, size_t scratch_bytes,
                       snn_stream_t stream) {
    WgradArgs a;
    if (tap_view("snn_li_heads_wgrad", planes, view, T_prime, &a.v)) return -1;
    if (!p) return fail(-1, "snn_li_heads_wgrad: null parameters");
    if (p->li_order != 0 && p->li_order != 1) return fail(-1, "snn_li_heads_wgrad: li_order = %d (0 jump-first, 1 voltage-first)", p->li_order);
    if (n_cols < 1 || n_cols > 32 * a.v.words) return fail(-1, "snn_li_heads_wgrad: n_cols = %d outside 1 .. 32 x words = %d", n_cols, 32 * a.v.words);
    if (!wgrad_shape_ok(a.v.rows, n_cols, NA, NB))
        return fail(-1, "snn_li_heads_wgrad: NA = %d, NB = %d (each >= 0, 1 <= NA + NB <= %d)", NA, NB, WG_MAX_OUT);
    if ((NA && (!grad_a || !gw_a)) || (NB && (!grad_b || !gw_b))) return fail(-1, "snn_li_heads_wgrad: null gradient or result of a head with outputs");
    if (accumulate != 0 && accumulate != 1) return fail(-1, "snn_li_heads_wgrad: accumulate = %d (0 or 1)", accumulate);
    const size_t need = snn_li_heads_wgrad_workspace_bytes(a.v.rows, n_cols, NA, NB);
    if (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 3)) return fail(-1, "snn_li_heads_wgrad: scratch %zu < %zu bytes (or null / misaligned)", scratch_bytes, need);
    Kappa kap;
    li_kappa(p, T_prime, &kap);
    for (int t = 0; t < SNN_MAX_STEPS; ++t) a.kappa[t] = kap.last[t];
    a.ga = grad_a; a.gb = grad_b; a.NA = NA; a.NB = NB; a.n_cols = n_cols; a.T = T_prime;
    a.tiles = cdiv(a.v.rows, WG_ROWS); a.n_slabs = wgrad_slabs(a.v.rows);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_li_wgrad_partial, dim3(a.n_slabs, cdiv(cdiv(n_cols, 32), WG_WORDS), cdiv(NA + NB, WG_JW)), dim3(256), 0, s, a, (float*)scratch);
    SNN_CHECK_LAUNCH("k_li_wgrad_partial");
    hipLaunchKernelGGL(k_li_wgrad_reduce, dim3(cdiv((long long)(NA + NB) * n_cols, WG_RED)), dim3(256), 0, s, (const float*)scratch, a.n_slabs, NA, NB, n_cols,
                       gw_a, gw_b, accumulate);
    SNN_CHECK_LAUNCH("k_li_wgrad_reduce");
    return 0;
}

// ---- readout fine-tuning: target matching and the two head losses (kernels: snn_loss.h) ----
static inline int misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

size_t snn_match_targets_workspace_bytes(int64_t total_boxes, int N) {
    if (N < 1 || N > LS_MAX_IMAGES || total_boxes < 0 || total_boxes > 0x7fffffffLL) return 0;
    // per-GT maxima of every work-group (at most total / 256 + N of them), then the per-GT maxima of every image
    return ((size_t)(total_boxes / LS_BLOCK) + 2 * (size_t)N) * LS_MAX_GT * sizeof(uint32_t);
}

int snn_match_targets(const float* boxes, const int64_t* box_start, const float* gt_boxes, const int64_t* gt_labels, const int64_t* gt_start, int N,
                      float high, float low, int allow_low_quality, const float* weights, int32_t* matched_idx, int32_t* label, float* reg_target,
                      void* scratch, size_t scratch_bytes, snn_stream_t stream) {
    if (!box_start || !gt_start || !weights) return fail(-1, "snn_match_targets: null box_start / gt_start / weights");
    if (N < 1) return fail(-1, "snn_match_targets: N = %d images", N);
    if (N > LS_MAX_IMAGES) return fail(-4, "snn_match_targets: N = %d images (max %d)", N, LS_MAX_IMAGES);
    if (allow_low_quality != 0 && allow_low_quality != 1) return fail(-1, "snn_match_targets: allow_low_quality = %d (0 or 1)", allow_low_quality);
    if (box_start[0] != 0 || gt_start[0] != 0) return fail(-1, "snn_match_targets: box_start[0] and gt_start[0] must be 0");
    MatchArgs a;
    int blocks = 0;
    for (int n = 0; n < N; ++n) {
        const int64_t B = box_start[n + 1] - box_start[n], G = gt_start[n + 1] - gt_start[n];
        if (B < 0 || G < 0) return fail(-1, "snn_match_targets: box_start / gt_start must not decrease (image %d)", n);
        if (box_start[n + 1] > 0x7fffffffLL) return fail(-4, "snn_match_targets: %lld boxes (max 2^31 - 1)", (long long)box_start[n + 1]);
        if (G > LS_MAX_GT) return fail(-4, "snn_match_targets: image %d has %lld ground-truth boxes (max %d)", n, (long long)G, LS_MAX_GT);
        a.box_start[n] = (int)box_start[n]; a.gt_start[n] = (int)gt_start[n]; a.blk_start[n] = blocks;
        blocks += cdiv(B, LS_BLOCK);
    }
    a.box_start[N] = (int)box_start[N]; a.gt_start[N] = (int)gt_start[N]; a.blk_start[N] = blocks;
    for (int n = N + 1; n <= LS_MAX_IMAGES; ++n) a.box_start[n] = a.gt_start[n] = a.blk_start[n] = 0;
    const int total = a.box_start[N], total_gt = a.gt_start[N];
    if (total == 0) return 0;
    if (!boxes || !matched_idx || !label || !reg_target || (total_gt && !gt_boxes)) return fail(-1, "snn_match_targets: null boxes, ground truth or output");
    if (misaligned16(boxes) || misaligned16(gt_boxes) || misaligned16(reg_target)) return fail(-1, "snn_match_targets: boxes, gt_boxes and reg_target must be 16-byte aligned");
    const size_t need = snn_match_targets_workspace_bytes(total, N);
    if (allow_low_quality && (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 3)))
        return fail(-1, "snn_match_targets: scratch %zu < %zu bytes (or null / misaligned)", scratch_bytes, need);
    a.boxes = (const float4*)boxes; a.gt = (const float4*)gt_boxes; a.gt_labels = (const long long*)gt_labels;
    a.N = N; a.allow_lq = allow_low_quality; a.high = high; a.low = low;
    a.wx = weights[0]; a.wy = weights[1]; a.ww = weights[2]; a.wh = weights[3];
    hipStream_t s = (hipStream_t)stream;
    uint32_t* part = (uint32_t*)scratch;
    uint32_t* gtmax = part ? part + (size_t)blocks * LS_MAX_GT : nullptr;
    if (allow_low_quality && total_gt) {
        hipLaunchKernelGGL(k_match_partial, dim3(blocks), dim3(LS_BLOCK), 0, s, a, part);
        SNN_CHECK_LAUNCH("k_match_partial");
        hipLaunchKernelGGL(k_match_gtmax, dim3(N), dim3(LS_BLOCK), 0, s, a, (const uint32_t*)part, gtmax);
        SNN_CHECK_LAUNCH("k_match_gtmax");
    }
    hipLaunchKernelGGL(k_match_finish, dim3(blocks), dim3(LS_BLOCK), 0, s, a, (const uint32_t*)gtmax, matched_idx, label, (float4*)reg_target);
    SNN_CHECK_LAUNCH("k_match_finish");
    return 0;
}

size_t snn_rpn_loss_grad_workspace_bytes(int64_t anchors) {
    if (anchors < 1 || anchors > 0x7fffffffLL) return 0;
    return LS_HEADER + (size_t)cdiv(anchors, LS_BLOCK) * 3 * sizeof(double);
}

int snn_rpn_loss_grad(const snn_rpn_level* levels, int n_levels, int A, int N, const float* logits, const float* deltas, const int32_t* label,
                      const uint8_t* sampled, const float* reg_target, float* loss, float* g_logits, float* g_deltas, void* scratch,
                      size_t scratch_bytes, snn_stream_t stream) {
    if (!levels || !logits || !deltas || !label || !sampled || !reg_target || !loss || !g_logits || !g_deltas)
        return fail(-1, "snn_rpn_loss_grad: null argument");
    if (n_levels < 1 || A < 1 || N < 1) return fail(-1, "snn_rpn_loss_grad: n_levels = %d, A = %d, N = %d (each >= 1)", n_levels, A, N);
    if (n_levels > LS_MAX_LEVELS) return fail(-4, "snn_rpn_loss_grad: %d levels (max %d)", n_levels, LS_MAX_LEVELS);
    if (A > LS_MAX_A) return fail(-4, "snn_rpn_loss_grad: A = %d anchors per position (max %d)", A, LS_MAX_A);
    RpnLossArgs a;
    long long rows = 0, per_image = 0;
    for (int l = 0; l < LS_MAX_LEVELS; ++l) { a.row_start[l] = 0; a.hw[l] = 1; a.anc_off[l] = 0; }
    for (int l = 0; l < n_levels; ++l) {
        if (levels[l].N != N || levels[l].H < 1 || levels[l].W < 1)
            return fail(-1, "snn_rpn_loss_grad: level %d is %d x %d x %d (N = %d, H and W >= 1)", l, levels[l].N, levels[l].H, levels[l].W, N);
        const long long hw = (long long)levels[l].H * levels[l].W;
        if ((rows + hw * N) * A > 0x7fffffffLL) return fail(-4, "snn_rpn_loss_grad: more than 2^31 - 1 anchors");
        a.row_start[l] = (int)rows; a.hw[l] = (int)hw; a.anc_off[l] = (int)(per_image * A);
        rows += hw * N; per_image += hw;
    }
    a.n_levels = n_levels; a.A = A; a.per_image = (int)(per_image * A); a.total = (int)(rows * A);
    if (misaligned16(deltas) || misaligned16(reg_target) || misaligned16(g_deltas))
        return fail(-1, "snn_rpn_loss_grad: deltas, reg_target and g_deltas must be 16-byte aligned");
    const size_t need = snn_rpn_loss_grad_workspace_bytes(a.total);
    if (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 7)) return fail(-1, "snn_rpn_loss_grad: scratch %zu < %zu bytes (or null / misaligned)", scratch_bytes, need);
    int* n_dev = (int*)scratch;
    double* part = (double*)((char*)scratch + LS_HEADER);
    const int nb = cdiv(a.total, LS_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rpn_loss<false>, dim3(nb), dim3(LS_BLOCK), 0, s, a, logits, (const float4*)deltas, label, sampled, (const float4*)reg_target, part,
                       (const int*)n_dev, g_logits, (float4*)g_deltas);
    SNN_CHECK_LAUNCH("k_rpn_loss<false>");
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(LS_BLOCK), 0, s, (const double*)part, nb, loss, n_dev);
    SNN_CHECK_LAUNCH("k_loss_finish");
    hipLaunchKernelGGL(k_rpn_loss<true>, dim3(nb), dim3(LS_BLOCK), 0, s, a, logits, (const float4*)deltas, label, sampled, (const float4*)reg_target, part,
                       (const int*)n_dev, g_logits, (float4*)g_deltas);
    SNN_CHECK_LAUNCH("k_rpn_loss<true>");
    return 0;
}

size_t snn_det_loss_grad_workspace_bytes(int R, int K) {
    if (R < 1 || K < 2 || K > LS_MAX_K || (long long)R * K * 4 > 0x7fffffffLL) return 0;
    return LS_HEADER + (size_t)cdiv(R, DL_ROWS) * 3 * sizeof(double);
}

int snn_det_loss_grad(const float* logits, const float* box, const int32_t* label, const float* reg_target, int R, int K, int K4, float* loss,
                      float* g_logits, float* g_box, void* scratch, size_t scratch_bytes, snn_stream_t stream) {
    if (!logits || !box || !label || !reg_target || !loss || !g_logits || !g_box) return fail(-1, "snn_det_loss_grad: null argument");
    if (R < 1 || K < 2) return fail(-1, "snn_det_loss_grad: R = %d rows, K = %d classes (R >= 1, K >= 2)", R, K);
    if (K4 != 4 * K) return fail(-1, "snn_det_loss_grad: K4 = %d box outputs for K = %d classes (the loss indexes one box per class: K4 = 4 K)", K4, K);
    if (K > LS_MAX_K) return fail(-4, "snn_det_loss_grad: K = %d classes (max %d)", K, LS_MAX_K);
    if ((long long)R * K4 > 0x7fffffffLL) return fail(-4, "snn_det_loss_grad: R x 4K = %lld elements (max 2^31 - 1)", (long long)R * K4);
    if (misaligned16(logits) || misaligned16(box) || misaligned16(reg_target) || misaligned16(g_logits) || misaligned16(g_box))
        return fail(-1, "snn_det_loss_grad: logits, box, reg_target, g_logits and g_box must be 16-byte aligned");
    const size_t need = snn_det_loss_grad_workspace_bytes(R, K);
    if (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 7)) return fail(-1, "snn_det_loss_grad: scratch %zu < %zu bytes (or null / misaligned)", scratch_bytes, need);
    int* n_dev = (int*)scratch;
    double* part = (double*)((char*)scratch + LS_HEADER);
    const int nb = cdiv(R, DL_ROWS);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_det_loss<false>, dim3(nb), dim3(LS_BLOCK), 0, s, logits, (const float4*)box, label, (const float4*)reg_target, R, K, part,
                       (const int*)n_dev, g_logits, (float4*)g_box);
    SNN_CHECK_LAUNCH("k_det_loss<false>");
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(LS_BLOCK), 0, s, (const double*)part, nb, loss, n_dev);
    SNN_CHECK_LAUNCH("k_loss_finish");
    hipLaunchKernelGGL(k_det_loss<true>, dim3(nb), dim3(LS_BLOCK), 0, s, logits, (const float4*)box, label, (const float4*)reg_target, R, K, part,
                       (const int*)n_dev, g_logits, (float4*)g_box);
    SNN_CHECK_LAUNCH("k_det_loss<true>");
    return 0;
}

// ---- hidden-layer gradients of fc7 -> lif7: SuperSpike LIF adjoint and the spike-fed linear layer's weight gradient (DESIGN.md 4.15;
// kernels: snn_hidden.h) ----
static inline long long cdivll(long long a, long long b) { return (a + b - 1) / b; }

int snn_planes_to_rows(const void* ws, const snn_planes_view* view, int T_prime, uint32_t* out, snn_stream_t stream) {
    TapView v;
    if (tap_view("snn_planes_to_rows", ws, view, T_prime, &v)) return -1;
    if (!out) return fail(-1, "snn_planes_to_rows: null result");
    const long long total = (long long)T_prime * v.rows * v.words;
    hipLaunchKernelGGL(k_planes_to_rows, dim3((unsigned)min(cdivll(total, 256), 65536LL)), dim3(256), 0, (hipStream_t)stream, v, T_prime, out);
    SNN_CHECK_LAUNCH("k_planes_to_rows");
    return 0;
}

int snn_lif_surrogate_bwd(const float* cur, int ldc, const uint32_t* z_rows, int Tc, int R, int N, const snn_params* p, float alpha, const float* gz,
                          const float* gu, float* d_cur, snn_stream_t stream) {
    if (!cur || !z_rows || !d_cur || !p) return fail(-1, "snn_lif_surrogate_bwd: null currents, planes, result or parameters");
    if (!gz && !gu) return fail(-1, "snn_lif_surrogate_bwd: gz and gu are both null (no upstream gradient)");
    if (Tc < 1 || Tc > SNN_MAX_STEPS - 1) return fail(-1, "snn_lif_surrogate_bwd: Tc = %d outside [1, %d]", Tc, SNN_MAX_STEPS - 1);
    if (R < 1 || N < 1 || N > HB_MAX_N || ldc < N) return fail(-1, "snn_lif_surrogate_bwd: R = %d, N = %d, ldc = %d (R >= 1, 1 <= N <= %d, ldc >= N)", R, N, ldc, HB_MAX_N);
    if (!(alpha >= 0.0f) || !__builtin_isfinite(alpha)) return fail(-1, "snn_lif_surrogate_bwd: alpha = %g (finite and >= 0)", (double)alpha);
    if (p->li_order != 0 && p->li_order != 1) return fail(-1, "snn_lif_surrogate_bwd: li_order = %d (0 jump-first, 1 voltage-first)", p->li_order);
    LifBwdArgs a;
    a.cur = cur; a.z = z_rows; a.gz = gz; a.gu = gu; a.d_cur = d_cur;
    a.ldc = ldc; a.Tc = Tc; a.R = R; a.N = N; a.Nw = cdiv(N, 32);
    a.a = p->dt_tau_mem; a.b = p->neg_dt_tau_syn; a.v_leak = p->v_leak; a.v_reset = p->v_reset; a.th = p->v_th_lif; a.alpha = alpha;
    Kappa kap;
    li_kappa(p, Tc + 1, &kap);
    for (int t = 0; t < SNN_MAX_STEPS; ++t) a.kappa[t] = kap.last[t];
    hipLaunchKernelGGL(k_lif_surrogate_bwd, dim3((unsigned)min(cdivll((long long)R * N, 256), 1LL << 20)), dim3(256), 0, (hipStream_t)stream, a);
    SNN_CHECK_LAUNCH("k_lif_surrogate_bwd");
    return 0;
}

static int spike_wgrad_shape_ok(long long rows, int K, int N, int T) {
    return rows >= 1 && rows <= 0x7fffffffLL && K >= 1 && K <= SW_MAX_DIM && N >= 1 && N <= SW_MAX_DIM && T >= 1 && T <= SNN_MAX_STEPS;
}
// row slabs of the reduction over M = T' x rows: a function of M alone; every slab but the last holds slab_rows rows (a multiple of the batch)
static int spike_wgrad_slabs(long long M, long long* slab_rows) {
    const long long want = min(cdivll(M, SW_SLAB_ROWS), (long long)SW_MAX_SLABS);
    const long long per = cdivll(cdivll(M, want), SW_BATCH) * SW_BATCH;
    if (slab_rows) *slab_rows = per;
    return (int)cdivll(M, per);
}

size_t snn_spike_linear_wgrad_workspace_bytes(int64_t rows, int K, int N, int T_prime) {
    if (!spike_wgrad_shape_ok(rows, K, N, T_prime)) return 0;
    return (size_t)spike_wgrad_slabs((long long)rows * T_prime, nullptr) * (size_t)N * (size_t)K * sizeof(float);
}

int snn_spike_linear_wgrad(const uint32_t* a_rows, const float* d_cur, int ldd, int T_prime, int64_t rows, int K, int N, float* gw, int accumulate,
                           void* scratch, size_t scratch_bytes, snn_stream_t stream) {
    if (!a_rows || !d_cur || !gw) return fail(-1, "snn_spike_linear_wgrad: null planes, gradient or result");
    if (!spike_wgrad_shape_ok(rows, K, N, T_prime))
        return fail(-1, "snn_spike_linear_wgrad: rows = %lld, K = %d, N = %d, T' = %d (1 <= rows < 2^31, 1 <= K, N <= %d, 1 <= T' <= %d)", (long long)rows, K, N,
                    T_prime, SW_MAX_DIM, SNN_MAX_STEPS);
    if (ldd < N || ldd >= (1 << 28)) return fail(-1, "snn_spike_linear_wgrad: ldd = %d (N = %d <= ldd < 2^28)", ldd, N);
    if (accumulate != 0 && accumulate != 1) return fail(-1, "snn_spike_linear_wgrad: accumulate = %d (0 or 1)", accumulate);
    const size_t need = snn_spike_linear_wgrad_workspace_bytes(rows, K, N, T_prime);
    if (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 3)) return fail(-1, "snn_spike_linear_wgrad: scratch %zu < %zu bytes (or null / misaligned)", scratch_bytes, need);
    SpikeWgradArgs a;
    a.a = a_rows; a.d = d_cur; a.M = (long long)rows * T_prime; a.ldd = ldd; a.K = K; a.Kw = cdiv(K, 32); a.N = N;
    a.n_slabs = spike_wgrad_slabs(a.M, &a.slab_rows);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_spike_wgrad_partial, dim3(cdiv(K, SW_TK), cdiv(N, SW_TN), a.n_slabs), dim3(256), 0, s, a, (float*)scratch);
    SNN_CHECK_LAUNCH("k_spike_wgrad_partial");
    const size_t n = (size_t)N * K;
    hipLaunchKernelGGL(k_spike_wgrad_reduce, dim3((unsigned)min(cdivll((long long)n, 256), 1LL << 20)), dim3(256), 0, s, (const float*)scratch, a.n_slabs, n, gw,
                       accumulate);
    SNN_CHECK_LAUNCH("k_spike_wgrad_reduce");
    return 0;
}

// ---- the spike-fed weight gradient on the bf16 matrix cores: d_cur split into three bf16 planes on the fly (kernels:
// snn_spike_wgrad_x3.h) ----
static int wgrad3_shape_ok(long long rows, int K, int N, int T) {
    return rows >= 1 && rows <= 0x7fffffffLL && K >= 1 && K <= W3_MAX_K && N >= 1 && N <= W3_MAX_N && T >= 1 && T <= SNN_MAX_STEPS;
}
// row slabs of the reduction over M = T' x rows: a pure function of (M, K, N) - one when the output tiles alone fill the device, otherwise
// as many as it takes to fill it; every slab but the last holds slab_rows rows (a multiple of the stage)
static int wgrad3_slabs(long long M, int K, int N, long long* slab_rows) {
    const long long tiles = (long long)cdiv(N, W3_TN) * cdiv(K, W3_TK);
    const long long want = tiles >= W3_FILL ? 1 : min(min(cdivll(W3_FILL, tiles), cdivll(M, W3_SLAB_ROWS)), (long long)W3_MAX_SLABS);
    const long long per = cdivll(cdivll(M, want), W3_MB) * W3_MB;
    if (slab_rows) *slab_rows = per;
    return (int)cdivll(M, per);
}

// slabs N K <= min(ceil(M / 256) capped at 32, 256 / tiles + 1) N K, and N K / tiles <= 128 x 256: both bounds are monotone in every argument
// (the slab count itself is not: it falls as the tiles grow), so their minimum is
size_t snn_spike_wgrad_bf16x3_workspace_bytes(int64_t rows, int K, int N, int T_prime) {
    if (!wgrad3_shape_ok(rows, K, N, T_prime)) return 0;
    const size_t nk = (size_t)N * (size_t)K;
    const size_t by_rows = (size_t)min(cdivll((long long)rows * T_prime, W3_SLAB_ROWS), (long long)W3_MAX_SLABS) * nk;
    const size_t by_fill = (size_t)W3_FILL * W3_TN * W3_TK + nk;
    return (by_rows < by_fill ? by_rows : by_fill) * sizeof(float);                 // (no min(): the device headers' overloads narrow to int)
}

// the launch plan's slab count (and the rows of every slab but the last), host only: what the header documents, observable
int snn_spike_wgrad_bf16x3_slabs(int64_t rows, int K, int N, int T_prime, int64_t* slab_rows) {
    if (slab_rows) *slab_rows = 0;
    if (!wgrad3_shape_ok(rows, K, N, T_prime)) return 0;
    long long per = 0;
    const int n = wgrad3_slabs((long long)rows * T_prime, K, N, &per);
    if (slab_rows) *slab_rows = per;
    return n;
}

int snn_spike_wgrad_bf16x3(const uint32_t* a_rows, const float* d_cur, int ldd, int T_prime, int64_t rows, int K, int N, float* gw, int accumulate,
                           void* scratch, size_t scratch_bytes, snn_stream_t stream) {
    if (!a_rows || !d_cur || !gw) return fail(-1, "snn_spike_wgrad_bf16x3: null planes, gradient or result");
    if (!wgrad3_shape_ok(rows, K, N, T_prime))
        return fail(-1, "snn_spike_wgrad_bf16x3: rows = %lld, K = %d, N = %d, T' = %d (1 <= rows < 2^31, 1 <= K <= %d, 1 <= N <= %d, 1 <= T' <= %d)",
                    (long long)rows, K, N, T_prime, W3_MAX_K, W3_MAX_N, SNN_MAX_STEPS);
    if (ldd < N || ldd >= (1 << 28)) return fail(-1, "snn_spike_wgrad_bf16x3: ldd = %d (N = %d <= ldd < 2^28)", ldd, N);
    if (accumulate != 0 && accumulate != 1) return fail(-1, "snn_spike_wgrad_bf16x3: accumulate = %d (0 or 1)", accumulate);
    const size_t need = snn_spike_wgrad_bf16x3_workspace_bytes(rows, K, N, T_prime);
    if (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 3)) return fail(-1, "snn_spike_wgrad_bf16x3: scratch %zu < %zu bytes (or null / misaligned)", scratch_bytes, need);
    Wgrad3Args a;
    a.a = a_rows; a.d = d_cur; a.M = (long long)rows * T_prime; a.ldd = ldd; a.K = K; a.Kw = cdiv(K, 32); a.N = N; a.accumulate = accumulate;
    a.n_slabs = wgrad3_slabs(a.M, K, N, &a.slab_rows);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_wgrad3_partial, dim3(cdiv(K, W3_TK), cdiv(N, W3_TN), a.n_slabs), dim3(256), 0, s, a, (float*)scratch, gw);
    SNN_CHECK_LAUNCH("k_wgrad3_partial");
    if (a.n_slabs > 1) {
        const size_t n = (size_t)N * K;
        hipLaunchKernelGGL(k_wgrad3_reduce, dim3((unsigned)min(cdivll((long long)n, 256), 1LL << 20)), dim3(256), 0, s, (const float*)scratch, a.n_slabs, n, gw,
                           accumulate);
        SNN_CHECK_LAUNCH("k_wgrad3_reduce");
    }
    return 0;
}

}  // extern "C"
