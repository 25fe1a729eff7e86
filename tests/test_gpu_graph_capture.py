"""Every stream-only entry of ops.py captured into a hipGraph and replayed on new data (the protocol of tests/_graph_capture.py).

include/snn_hip.h promises that a call enqueues its work on the caller's stream and nothing else.  Each test here warms the caches, runs the
eager twin of every input set (inside poisoned outputs, on a pinned GuardedWorkspace armed with zeros; the twin of set 0 meets the oracle with
zero flips through the builders of tests/_entry_cases.py), captures ONE call on one stream, and replays it at least four times over at least
two input sets with the workspace re-armed 0xff / 0x5a / 0x00 / 0xff: every replay is bit-equal to the eager twin of its set in everything a
caller can observe (outputs, time sums, integer spike counts, rate rows, route_stat, device-side counts, the rows behind the counts, the
hidden planes), the guards and the tail behind the region are intact, and where the builders have an oracle for the set the replay meets it
too.  Nothing runs at the workload's size; no synchronising entry (tests/_graph_capture.SYNCHRONISING) is ever called inside a capture.

Which case reaches which entry and launch plan:

  entry                                  cases
  rpn_head_forward                       (a) HEADS rpn T4 (dense conv) / T5 T8 T12 T16 (sparse), C64 / C128 / C256 split planes / 1x1 pyramid, f32, bf16, mxfp6,
                                         every variant of _ws_state.ENTRIES (plain, rates + the rates workspace, sparse, dense, auto_never, auto_always);
                                         (b) ROUTES auto at the header's crossover, capture on either side; (c) TYPED fp16 / bf16 NCHW, fp16 channels-last; (f)
  rpn_head_forward_readouts              (a) T12 plain / rates
  det_head_forward                       (a) det T4 .. T24, R 1 / 17 / 29 / 65, C32 (dense fc6) / C64 (sparse), f32, bf16, mxfp6, every variant; (b); (c) fp16 rows,
                                         a plan without a typed kernel (the widening fall-back inside the capture), a misaligned half view (the clone inside it)
  det_head_forward_readouts              (a) plain / rates
  det_head_forward_roialign              (a) plain / dense / auto_never / auto_always / rates; (c) fp16 / bf16 NCHW, fp16 channels-last; (f)
  det_head_forward_roialign_readouts     (a) plain / rates
  nms_keep_mask                          (e) n 65 / 129, 1 and 3 categories
  rpn_proposals                          (e) r_t3_cut: counts at post_nms_top_n, below it, zero; (f)
  det_postprocess                        (e) d_k5_small: counts at detections_per_img, below it, zero
  det_postprocess_padded                 (e) d_k5_small likewise; d_k5_big under the device counts (70, 37, 0) / (0, 70, 5) / zeros; (f)
  roi_assign                             (d) counts (70, 37, 0) / (0, 70, 5); (f)
  encode_nchw  encode_rows               (d) fp32 maps; rows D = 3136 (word-major) and D = 100 (row-major)
  conv3x3_lif_bf16x3  spike_conv3x3_bf16x3  spike_gemm_lif_bf16x3  spike_gemm_bf16x3      (d)
  conv3x3_lif_mx  spike_conv3x3_mx  spike_gemm_lif_mx  spike_gemm_mx                      (d)
  conv3x3_lif  spike_gemm  lif_scan      (d) fp32 path, spike counts on
  li_heads  li_heads_readouts            (d) tests/_li_grid.py cases, sums on: valu (K32), mfma resident (K256), ksplit (K1024), mfma streamed (K1024 forced),
                                         readouts resident and ksplit
  roi_align_encode  det_exchange_payload  det_rates  affine_act_nchw (residual, relu, in place)   (d)
  pack_conv3x3  pack_linear  pack_linear_mx  pack_conv3x3_mx                              (d) the packers without a verdict
  static.heads_padded                    (f) T 8 / 12, the 128 x 256 pyramid, b = 2: cap 40 and cap 1000 at score_thresh 0.5, three feature sets; bf16
  ops._Workspace (no seam)               (g) two graphs, a larger eager call on both stream keys, replays, one graph deleted"""
import numpy as np
import pytest
import torch

from tests import _conv_route as CR
from tests import _entry_cases as E
from tests import _fc6_route as FR
from tests import _graph_capture as GC
from tests import _ws_state as W
from tests._entry_cases import det, post, roi, rpn, spec_id

pytestmark = pytest.mark.gpu


# ---- the seam (as tests/test_gpu_ws_state.py) ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def buffers(gpu_device):
    return W.GuardedWorkspace(gpu_device), W.GuardedWorkspace(gpu_device, 1 << 20)


@pytest.fixture
def seam(buffers, monkeypatch):
    from snn_automotive_object_detection_amd import ops
    monkeypatch.setattr(ops, "_WS", buffers[0])
    monkeypatch.setattr(ops, "_WS_RATES", buffers[1])
    for b in buffers:
        b.short_by = 0
        b.arm(0x00)
    return buffers


def _protocol(case, seam):
    cap = GC.run_protocol(case, GC.HipGraph(), seam)
    assert cap.n_replays >= 4 and len(cap.seen) == case.n_sets
    assert seam[0].sizes, "the captured call never asked for a workspace"
    return cap


# ---- (a) both heads, every variant of _ws_state.ENTRIES --------------------------------------------------------------------------------------
RO = dict(entry="rpn_head_forward_readouts")
DRO = dict(entry="det_head_forward_readouts")
RRO = dict(entry="det_head_forward_roialign_readouts")
RPN_SETS, DET_SETS, ROI_SETS = ("mixed", "case"), ("case", "full"), ("draw0", "draw1")


def _heads():
    out = [(rpn(64, T, "mixed"), RPN_SETS) for T in (4, 5, 8, 12, 16)]
    out += [(rpn(64, 8, "mixed", v), RPN_SETS) for v in W.HEAD_VARIANTS[1:]] + [(rpn(64, 8, "mixed", "rates", ws="_WS_RATES"), RPN_SETS)]
    out += [(rpn(128, 16, "full", v), ("full", "mixed")) for v in ("plain", "auto_never")]
    out += [(rpn(256, 8, "mixed", "plain", shapes=W.SPLIT_PYRAMID), ("mixed", "full")), (rpn(64, 5, "full", in_shapes=W.ONE_BY_ONE), ("full", "silent"))]
    out += [(rpn(64, 4, "mixed", v), RPN_SETS) for v in ("rates", "auto_always")]
    out += [(rpn(64, 8, "mixed", precision="f32"), RPN_SETS), (rpn(64, 8, "mixed", precision="bf16"), RPN_SETS), (rpn(128, 8, "mixed", precision="mxfp6"), RPN_SETS)]
    out += [(rpn(64, 12, "mixed", v, **RO), RPN_SETS) for v in ("plain", "rates")] + [(rpn(64, 12, "mixed", "rates", ws="_WS_RATES", **RO), RPN_SETS)]
    out += [(det(29, 64, T), DET_SETS) for T in (4, 5, 8, 12, 16, 24)]
    out += [(det(R, C, 12), DET_SETS) for R, C in ((1, 64), (17, 32), (65, 64))]
    out += [(det(29, 64, 12, "case", v), DET_SETS) for v in W.HEAD_VARIANTS[1:]]
    out += [(det(29, 64, 12, precision="f32"), DET_SETS), (det(29, 64, 12, precision="bf16"), DET_SETS), (det(37, 128, 12, precision="mxfp6"), ("case", "mixed"))]
    out += [(det(29, 64, 12, "case", v, **DRO), DET_SETS) for v in ("plain", "rates")]
    out += [(roi(v), ROI_SETS) for v in W.ENTRIES[("det_head_forward_roialign", "_WS")]] + [(roi("rates"), ROI_SETS)]
    out += [(roi(v, **RRO), ROI_SETS) for v in ("plain", "rates")]
    return out


HEADS = _heads()
# ---- (c) typed features ------------------------------------------------------------------------------------------------------------------
TYPED = ([(rpn(64, 8, "case", feat=f, nhwc=n), ("case", "mixed")) for f, n in (("fp16", False), ("bf16", False), ("fp16", True))]
         + [(roi("plain", feat=f, nhwc=n), ROI_SETS) for f, n in (("fp16", False), ("bf16", False), ("fp16", True))]
         + [(det(29, 64, 12, feat="fp16"), DET_SETS)])


def _ids(cases):
    return ["%s-then-%s" % (spec_id(s) if s["kind"] != "roi" else spec_id(s) + "-" + inputs[0], "-".join(inputs[1:])) for s, inputs in cases]


@pytest.mark.parametrize("s,inputs", HEADS, ids=_ids(HEADS))
def test_heads_replay_equals_eager_and_oracle(gpu_device, seam, s, inputs):
    _protocol(GC.EntryCase(s, gpu_device, inputs), seam)


@pytest.mark.parametrize("s,inputs", TYPED, ids=_ids(TYPED))
def test_typed_features_replay_equals_eager_and_oracle(gpu_device, seam, s, inputs):
    from snn_automotive_object_detection_amd import ops
    before = dict(ops.feature_calls)
    _protocol(GC.EntryCase(s, gpu_device, inputs), seam)
    assert ops.feature_calls["no_typed_kernel"] == before["no_typed_kernel"]                  # (these plans have typed kernels: nothing was widened)
    assert ops.feature_calls[{"fp16": "f16", "bf16": "bf16"}[s["feat"]]] >= before[{"fp16": "f16", "bf16": "bf16"}[s["feat"]]] + 4
    if s.get("nhwc"):
        assert ops.feature_calls["nhwc"] >= before["nhwc"] + 4


def _half_det(gpu_device, C, Hd, R, misaligned):
    """det_head_forward on fp16 rows [R, 49 C] of an exact-grid case -> (FnCase, the ops module)"""
    from snn_automotive_object_detection_amd import ops
    from tests import _exact_grid as G
    case = G.det_case(R, C, Hd, 9, 12, 900 + C, "wide")
    d = FR.head_for(case, gpu_device, "bf16x3")
    D = 49 * C
    args = d._pass_args(D, "rows")
    sets = [(case["x"].flatten(1).to(torch.float16),), (G.full_nibble_values((R, C, 7, 7), 12, torch.Generator().manual_seed(5)).flatten(1).to(torch.float16),)]

    def to_device(t):
        if not misaligned:
            return t.to(gpu_device)
        raw = torch.zeros(t.numel() + 8, dtype=t.dtype, device=gpu_device)
        view = raw[1:1 + t.numel()].view(t.shape)               # 2 bytes past a 16-byte boundary: ops._feat clones it, inside the capture too
        view.copy_(t)
        assert view.data_ptr() % 16 == 2
        return view

    def fn(x):
        cls, bbox, _ = ops.det_head_forward(x, T=12, **args)
        return cls, bbox
    fc = GC.FnCase(("det_head_forward",), gpu_device, sets, fn, to_device)
    fc.keep = (d, case)
    return fc, ops


def test_a_plan_without_a_typed_kernel_widens_inside_the_capture(gpu_device, seam):
    """half rows with D = 49 * 8 = 392 (D % 32 != 0): the typed entry returns SNN_STATUS_NO_TYPED_KERNEL with nothing enqueued and _typed_call
    widens and calls again - at warm-up, in every eager twin and once inside the capture"""
    fc, ops = _half_det(gpu_device, 8, 40, 17, False)
    before = ops.feature_calls["no_typed_kernel"]
    _protocol(fc, seam)
    assert ops.feature_calls["no_typed_kernel"] == before + 4    # warm-up, two eager twins, the capture (a replay has no host half)


def test_a_misaligned_half_view_is_cloned_inside_the_capture(gpu_device, seam):
    fc, ops = _half_det(gpu_device, 64, 128, 29, True)
    before = dict(ops.feature_calls)
    _protocol(fc, seam)
    assert ops.feature_calls["f16"] == before["f16"] + 4 and ops.feature_calls["no_typed_kernel"] == before["no_typed_kernel"]


# ---- (b) routes that flip under replay ---------------------------------------------------------------------------------------------------
ROUTES = [(rpn(128, 8, a, "auto"), (a, b)) for a, b in (("full", "silent"), ("silent", "full"), ("mixed", "full"), ("full", "mixed"))]
ROUTES += [(det(29, 64, 12, a, "auto"), (a, b)) for a, b in (("full", "silent"), ("silent", "full"), ("mixed", "silent"))]
ROUTES += [(det(29, 64, 8, "decided_" + a, "auto"), ("decided_" + a, "decided_" + b)) for a, b in (("randn_1", "randn_4"), ("randn_4", "randn_1"))]


@pytest.mark.parametrize("s,inputs", ROUTES, ids=_ids(ROUTES))
def test_route_flips_under_replay(gpu_device, seam, s, inputs):
    """`auto` at the header's crossover, the two input sets on DIFFERENT sides of it by the numpy restatement (asserted on the host first).  The
    graph is captured on the side set 1 takes (the last eager twin leaves it loaded) and replayed on set 0 first: the decision is made on the
    device on every replay.  After each replay route_stat holds the hits, blocks and route of ITS input (the oracle of tests/_entry_cases.py
    compares all four words with _stat_want) and outputs and planes are those of the eager call that took that route"""
    from snn_automotive_object_detection_amd import _lib
    case = GC.EntryCase(s, gpu_device, inputs)
    case.prepare()
    sides = []
    for n in inputs:
        x = case.ctx["host"][n][0]
        if s["kind"] == "rpn":
            hits, blocks = CR.route_counts(x, s["T"])
            sides.append(FR.route_of(hits, blocks, _lib.ROUTE_DEFAULT_CROSSOVER))
        else:
            hits, blocks = FR.route_counts(x.float(), s["T"])
            sides.append(FR.route_of(hits, blocks, _lib.FC6_ROUTE_DEFAULT_CROSSOVER))
    assert sorted(sides) == [0, 1], "the input sets %s take the routes %s: nothing flips" % (inputs, sides)
    cap = _protocol(case, seam)
    assert case.last["path"] == 2                                # the gated pair was captured: both routes are nodes of the graph
    seen = {}
    for i in (0, 1):
        cap.replay(i, 0x5a)
        seen[i] = case.last["stat"]
        assert seen[i][2] == sides[i] and seen[i][1] > 0, (inputs[i], seen[i])
    assert seen[0][2] != seen[1][2]


# ---- (e) post-processing -----------------------------------------------------------------------------------------------------------------
POST = [(post("nms_keep_mask", n=n, ncat=ncat, layout=lay), ("spec", "reversed", "one_box"), None) for n, lay in ((65, 3), (129, 5)) for ncat in (1, 3)]
POST += [(post("rpn_proposals", spec=W.RPN_POST_SPEC), ("spec", "fewer", "none"), ("spec",)),
         (post("det_postprocess", spec=W.DET_POST_SPEC), ("spec", "fewer", "none"), ("spec",)),
         (post("det_postprocess_padded", spec=W.DET_POST_SPEC), ("spec", "fewer", "none"), ("spec",)),
         (post("det_postprocess_padded", spec="d_k5_big"), ("counts_a", "counts_b", "counts_0"), ())]


def _counts(snap, part):
    return snap[part].view(torch.int32).tolist()


@pytest.mark.parametrize("s,inputs,oracle_sets", POST, ids=["%s-%s-%s" % (s["entry"], s.get("spec", "n%d_cat%d" % (s.get("n", 0), s.get("ncat", 0))), inputs[0]) for s, inputs, _ in POST])
def test_post_processing_replay_equals_eager(gpu_device, seam, s, inputs, oracle_sets):
    """the input sets differ in the COUNTS they produce: at the cap in set 0, below it in set 1, zero in set 2.  The rows behind the counts are rows
    of the snapshot (zero in the padded forms, still poisoned in the compacted one); set 0 meets the exact expectation of tests/_post_grid.py"""
    from tests import _post_grid as PG
    cap = _protocol(GC.EntryCase(s, gpu_device, inputs, oracle_sets), seam)
    if s["entry"] == "rpn_proposals":
        spec = PG.rpn_spec(s["spec"])
        c = [_counts(e, 3) for e in cap.eager]                   # snapshot(boxes, scores, counts, ..): part 0 is the list header
        print("rpn_proposals counts per input set", c)
        assert c[0] == [spec["post"]] * spec["N"], c             # at post_nms_top_n
        assert c[1][0] == spec["post"] and sum(c[1][1:]) < spec["post"] * (spec["N"] - 1) and not any(c[1][2:]) and not any(c[2]), c
    elif s["entry"].startswith("det_postprocess"):
        spec = PG.det_spec(s["spec"])
        c = [np.asarray(_counts(e, 4)).reshape(-1, 2) for e in cap.eager]
        print("det_postprocess counts (fg, bg) per input set", [x.tolist() for x in c])
        if inputs[0] == "spec":
            assert c[0][:, 0].max() == spec["det"], c[0]         # at detections_per_img
            assert c[1][:, 0].sum() < c[0][:, 0].sum() and c[1][:, 0].max() < spec["det"] and not c[2][:, 0].any(), c
        else:
            assert c[0].sum(1).tolist()[2] == 0 and c[1].sum(1).tolist()[0] == 0 and not c[2].any(), c
            assert c[0].sum() > 0 and c[1].sum() > 0
    else:
        kept = [int(e[1].numel()) // 8 for e in cap.eager]
        assert kept[2] == 1 and kept[0] > 1 and kept[1] > 1, kept


# ---- (d) stage entries and small kernels -------------------------------------------------------------------------------------------------
def _params():
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd.ops import LIFParameters
    return ops.make_params(LIFParameters(v_th=torch.tensor(0.25)), LIFParameters(alpha=100, v_th=torch.tensor(0.1)))


def _bits(shape, density, seed):
    """random spike planes: int32 words [T, M, Kw] for shape (T, M, K), rows [M, Kw] for shape (M, K)"""
    from tests._util import dense_to_planes
    z = (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < density).numpy()
    return dense_to_planes(z) if len(shape) == 3 else dense_to_planes(z[None])[0]


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bf16(w):
    return w.to(torch.bfloat16).float()                          # (one bf16 plane: splits exactly, so the packers' verdict is not needed)


CONV_SHAPES = [(1, 7, 9), (2, 3, 4)]
CONV_P = sum(n * h * w for n, h, w in CONV_SHAPES)


def _stage(name, dev):
    """-> (entries, input sets, fn) of the stage case `name`; weights are packed here, before anything is captured"""
    from snn_automotive_object_detection_amd import ops
    p = _params()
    if name in ("encode_nchw", "encode_rows_word_major", "encode_rows_row_major"):
        shape = {"encode_nchw": (2, 64, 5, 7), "encode_rows_word_major": (17, 3136), "encode_rows_row_major": (17, 100)}[name]
        f = ops.encode_nchw if name == "encode_nchw" else ops.encode_rows
        return (f.__name__,), [(_randn(shape, 1, 2.0),), (_randn(shape, 2, 2.0),)], lambda x: f(x, 8, p)
    if name in ("conv3x3_lif_bf16x3", "spike_conv3x3_bf16x3", "conv3x3_lif_mx", "spike_conv3x3_mx"):
        mx = name.endswith("_mx")
        Ci, Co, T = (128, 64, 8) if mx else (64, 64, 8)          # (shapes the eager tests of each path run)
        w = _bf16(_randn((Co, Ci, 3, 3), 3, 0.05)).to(dev)
        wp = ops.pack_conv3x3_mx(w) if mx else ops.pack_conv3x3_bf16x3(w)
        sets = [(_bits((T, CONV_P, Ci), 0.2, 4),), (_bits((T, CONV_P, Ci), 0.4, 5),)]
        if mx:                                                   # (the mx conv reads zero-halo planes)
            sets = [(ops.pad_planes(s[0], CONV_SHAPES),) for s in sets]
        f = getattr(ops, name)
        return (name,), sets, (lambda e: f(e, CONV_SHAPES, Ci, Co, p, wp)) if "lif" in name else (lambda e: f(e, CONV_SHAPES, Ci, Co, wp))
    if name in ("spike_gemm_lif_bf16x3", "spike_gemm_lif_mx", "spike_gemm_bf16x3", "spike_gemm_mx", "spike_gemm"):
        T, R, K, N = 8, 45, 384, 70
        w = _bf16(_randn((N, K), 6, 0.08)).to(dev)
        wp = ops.pack_linear_mx(w) if name.endswith("_mx") else ops.pack_linear(w) if name == "spike_gemm" else ops.pack_linear_bf16x3(w)
        f = getattr(ops, name)
        if "lif" in name:
            return (name,), [(_bits((T, R, K), 0.3, 7),), (_bits((T, R, K), 0.1, 8),)], lambda a: f(a, K, N, p, wp)
        return (name,), [(_bits((T * R, K), 0.3, 7),), (_bits((T * R, K), 0.1, 8),)], lambda a: f(a, K, N, wp)
    if name == "conv3x3_lif":
        N_, C, H, Wd, T = 2, 64, 6, 7, 8
        wp = ops.pack_conv3x3(_randn((C, C, 3, 3), 9, 0.1).to(dev))
        return (name,), [(_bits((T, N_ * H * Wd, C), 0.2, 10),), (_bits((T, N_ * H * Wd, C), 0.5, 11),)], lambda e: ops.conv3x3_lif(e, N_, C, C, H, Wd, p, wp, want_counts=True)
    if name == "lif_scan":
        return (name,), [(_randn((8, 37, 96), 12, 0.2),), (_randn((8, 37, 96), 13, 0.4),)], lambda c: ops.lif_scan(c, 70, p, want_counts=True)
    if name == "roi_align_encode":
        pool, feats, boxes, shapes = FR.roi_setup(64, 38, 52)
        feats2 = FR.roi_setup(64, 38, 53)[1]
        dev_feats = {k: v.to(dev) for k, v in feats.items()}
        flist, scales, rois, lvl = pool.assign(dev_feats, [b.to(dev) for b in boxes], shapes)
        r4, rb = rois[:, 1:5].contiguous(), rois[:, 0].contiguous()

        def fn(f0, f1):
            return ops.roi_align_encode([f0, f1], scales, r4, rb, lvl, 8, p, want_pooled=True)
        return (name,), [(feats["0"], feats["1"]), (feats2["0"], feats2["1"])], fn
    if name == "roi_assign":
        g = torch.Generator().manual_seed(14)
        xy = torch.rand((3, 70, 2), generator=g) * 100.0
        boxes = torch.cat([xy, xy + torch.exp(torch.rand((3, 70, 2), generator=g) * 5.0 + 1.4)], 2)
        return (name,), [(boxes, torch.tensor([70, 37, 0], dtype=torch.int32)), (boxes.flip(1).contiguous(), torch.tensor([0, 70, 5], dtype=torch.int32))], \
            lambda b, c: ops.roi_assign(b, c, 2, 5)
    if name == "det_exchange_payload":
        return (name,), [(_randn((2 * 50, 9), 15), _randn((2 * 50, 36), 16)), (_randn((2 * 50, 9), 17, 3.0), _randn((2 * 50, 36), 18))], \
            lambda c, r: ops.det_exchange_payload(c, r, 2, 20)
    if name == "det_rates":
        R = 37
        mk = lambda seed: (torch.randint(0, 3000, (R,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32),
                           torch.randint(0, 1500, (R,), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.int32),
                           _randn((R, 9), seed + 2), _randn((R, 36), seed + 3))
        return (name,), [mk(19), mk(29)], lambda c6, c7, sc, sb: ops.det_rates((c6, c7, sc, sb), 3136, 128, 9, 36, 12, False)
    if name == "affine_act_nchw":
        scale, bias = _randn((24,), 20).to(dev), _randn((24,), 21).to(dev)
        return (name,), [(_randn((2, 24, 5, 7), 22), _randn((2, 24, 5, 7), 23)), (_randn((2, 24, 5, 7), 24), _randn((2, 24, 5, 7), 25))], \
            lambda x, r: ops.affine_act_nchw(x, scale, bias, r, True, out=x)           # in place: load(i) puts the operand back before every replay
    if name.startswith("pack_"):
        shape = (70, 384) if "linear" in name else (64, 128, 3, 3)
        f = getattr(ops, name)
        return (name,), [(_randn(shape, 26, 0.05),), (_randn(shape, 27, 0.1),)], lambda w: f(w)
    raise KeyError(name)


STAGES = ["encode_nchw", "encode_rows_word_major", "encode_rows_row_major", "conv3x3_lif_bf16x3", "spike_conv3x3_bf16x3", "conv3x3_lif_mx", "spike_conv3x3_mx",
          "spike_gemm_lif_bf16x3", "spike_gemm_lif_mx", "spike_gemm_bf16x3", "spike_gemm_mx", "spike_gemm", "conv3x3_lif", "lif_scan", "roi_align_encode", "roi_assign",
          "det_exchange_payload", "det_rates", "affine_act_nchw", "pack_conv3x3", "pack_linear", "pack_linear_mx", "pack_conv3x3_mx"]
STAGE_ENTRIES = {n: ("encode_rows" if n.startswith("encode_rows") else n) for n in STAGES}


@pytest.mark.parametrize("name", STAGES)
def test_stage_entries_replay_equals_eager(gpu_device, name):
    entries, sets, fn = _stage(name, gpu_device)
    assert entries == (STAGE_ENTRIES[name],)
    cap = GC.run_protocol(GC.FnCase(entries, gpu_device, sets, fn), GC.HipGraph())
    assert cap.n_replays == 4


# (case id of tests/_li_grid.stage_grid, SNN_LI_HEADS, the kernel family of tests/test_gpu_li_grid.py's table)
LI_CASES = [("K32_N15_jump_first", "valu", "k_li_heads"), ("K256_N15_jump_first", None, "mfma resident"), ("K1024_N45_jump_first", None, "ksplit"),
            ("K1024_N45_jump_first", "mfma", "mfma streamed"), ("ro_a2_b2_T12_n4_83x256x15", None, "mfma_ro"), ("ro_a2_b2_T12_n4_17x1024x45", None, "ksplit_ro")]


@pytest.mark.parametrize("cid,form,family", LI_CASES, ids=["%s-%s" % (c, f or "default") for c, f, _ in LI_CASES])
def test_li_heads_replay_equals_eager_and_the_exact_expectation(gpu_device, monkeypatch, cid, form, family):
    """set 0 = the case's planes: outputs and time sums equal the integer expectation of tests/_li_grid.py bit for bit (eagerly and after every
    replay of set 0); set 1 = the same planes with the rows reversed"""
    from snn_automotive_object_detection_amd import ops
    from tests import _li_grid as L
    from tests import _neuron_constants as NC
    from tests._util import dense_to_planes
    if form is not None:
        monkeypatch.setenv("SNN_LI_HEADS", form)
    case = L.stage_case(**dict(L.stage_grid())[cid])
    K, NA, NB = case["K"], case["NA"], case["NB"]
    p = NC.abi_params(case["constants"], case["li_order"])
    wh = ops.pack_heads(case["w"][:NA].to(gpu_device), case["w"][NA:].to(gpu_device))
    planes = dense_to_planes(case["spk"])
    steps = case["steps"] if case["readouts"] else None
    exp = [torch.from_numpy(case["last"]), torch.from_numpy(case["sum"]) if case["sums"] else None]

    def fn(pl):
        if steps is None:
            return ops.li_heads(pl, K, wh, NA, NB, p, want_sums=True)
        return ops.li_heads_readouts(pl, K, wh, NA, NB, p, steps, want_sums=True)

    class LiCase(GC.FnCase):
        def check(self):
            o = [t.cpu() for t in self.results[-1]]
            o = [t[None] for t in o] if steps is None else o
            assert torch.equal(torch.cat([o[0], o[1]], -1), exp[0])
            assert exp[1] is None or torch.equal(torch.cat([o[2], o[3]], -1), exp[1])

        def oracle(self):
            self.check()

        def after_replay(self, k, i):
            if i == 0:
                self.check()
    entry = "li_heads" if steps is None else "li_heads_readouts"
    GC.run_protocol(LiCase((entry,), gpu_device, [(planes,), (planes.flip(1).contiguous(),)], fn), GC.HipGraph())


# ---- (f) the static path, end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(gpu_device):
    """the configuration of tests/test_gpu_static.py: T = 8 / 12, 9 classes"""
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(1234)
    model = S.create_model("cityscapes", 9, True, True, 0, False, False, num_steps_rpn=8, num_steps_detector=12).eval()
    model.rpn.to(gpu_device)
    model.roi_heads.to(gpu_device)
    with torch.no_grad():
        model.rpn.head.shared_conv.weight.mul_(5.0)
    model.roi_heads.score_thresh = 0.05
    return model


class StaticCase(GC.Case):
    """static.heads_padded on static feature maps; a snapshot = every key of the returned dict, then every tensor of static.unpad of it"""
    entries = ("rpn_head_forward", "rpn_proposals", "roi_assign", "det_head_forward_roialign", "det_postprocess_padded")

    def __init__(self, model, dev, sets, dtype=torch.float32):
        self.model, self.dev, self.sets, self.dtype = model, dev, sets, dtype
        self.n_sets = len(sets)
        self.outs = []

    def prepare(self):
        from collections import OrderedDict
        from tests.test_gpu_static import _images
        self.images = _images()
        self.feats = OrderedDict((k, v.to(self.dev).to(self.dtype)) for k, v in self.sets[0].items())

    def load(self, i):
        for k, v in self.sets[i].items():
            self.feats[k].copy_(v)

    def call(self):
        from snn_automotive_object_detection_amd import static
        out = static.heads_padded(self.model, self.feats, self.images)
        self.outs.append(out)

        def source():
            self.roi_counts = out["roi_counts"].tolist()
            unpadded = [[d[k] for k in sorted(d)] for d in static.unpad(out)]
            return W.snapshot([out[k] for k in sorted(out)], unpadded)
        return source


def _static_sets(seed=21):
    """saturating features, the same at a fifth of the amplitude (fewer neurons fire: other counts), all-silent features"""
    from tests.test_gpu_static import LEVELS, NAMES
    g = torch.Generator().manual_seed(seed)
    a = {n: 2 * torch.randn((2, 256, h, w), generator=g) for n, (h, w) in zip(NAMES, LEVELS)}
    b = {n: 0.2 * v.flip(0) for n, v in a.items()}
    b["0"][1] *= 0.25
    return [a, b, {n: torch.zeros_like(v) for n, v in a.items()}]


# (not here: the same capture with conv_route = fc6_route = "auto".  Its first replay - workspace armed 0xff, feature set 0, the graph captured on the
# silent set - ended in a GPU memory fault whose cause is not found ("Graph capture"); the eager twins of that configuration pass, and
# so do the routed entries under replay at the shapes of (b))
STATIC = {"cap40": dict(cap=40), "cap1000_thresh": dict(cap=1000, thresh=0.5), "cap40_bf16": dict(cap=40, bf16=True)}


@pytest.fixture(scope="module")
def big_buffers(gpu_device):
    """the detector head on 2 x 1000 rows asks for 172 MiB"""
    return W.GuardedWorkspace(gpu_device, 256 << 20), W.GuardedWorkspace(gpu_device, 1 << 20)


@pytest.fixture
def big_seam(big_buffers, monkeypatch):
    from snn_automotive_object_detection_amd import ops
    monkeypatch.setattr(ops, "_WS", big_buffers[0])
    monkeypatch.setattr(ops, "_WS_RATES", big_buffers[1])
    for b in big_buffers:
        b.arm(0x00)
    return big_buffers


@pytest.mark.parametrize("name", list(STATIC))
def test_static_path_replay_equals_eager(gpu_device, big_seam, detector, name):
    """the capture DESIGN.md 4.7 asks about: static.heads_padded from FPN features to padded detections, replayed on three feature sets; every key of
    the returned dict and static.unpad of it equal the eager run's"""
    from tests.test_gpu_static import _set_post_nms
    cfg = STATIC[name]
    heads = (detector.rpn.head, detector.roi_heads.box_head_and_predictor)
    _set_post_nms(detector, cfg["cap"])
    detector.rpn.score_thresh = cfg.get("thresh", 0.0)
    try:
        if cfg.get("bf16"):
            for h in heads:
                h.precision = "bf16"
        case = StaticCase(detector, gpu_device, _static_sets(), torch.bfloat16 if cfg.get("bf16") else torch.float32)
        cap = GC.capture_case(case, GC.HipGraph(), big_seam)
        counts = []
        for k, i in enumerate((0, 1, 2, 0, 1, 2)):
            cap.replay(i, GC.REPLAY_FILLS[k % 4])
            counts.append(case.roi_counts)
        print("roi_counts per replay", counts)
        assert counts[:3] == counts[3:]
        if cfg["cap"] == 40 and not cfg.get("bf16"):
            assert counts[0] == [40, 40]                          # saturated on set 0 (tests/test_gpu_static.py)
        if cfg["cap"] == 1000:
            assert max(counts[0]) < 1000 and any(c[0] != c[1] for c in counts[:3]), counts    # unsaturated, the images differ
    finally:
        detector.rpn.score_thresh = 0.0
        for h in heads:
            h.precision = "bf16x3"


# ---- (g) workspace lifetime: the REAL ops._Workspace ----------------------------------------------------------------------------------------
def test_workspace_outlives_later_larger_calls(gpu_device, monkeypatch):
    """two graphs hold workspaces of ops._Workspace (grow-only, keyed by device and stream); a larger eager call on the capture stream's key and on
    the default stream's replaces the buffers of both keys.  The buffers handed out during the captures stay alive (ops._Workspace.captured), so
    the replays after it are bit-equal to their eager twins; deleting one graph leaves the other intact.  The first graph's buffer is one the
    capture stream already had from an eager call (general pool, not the graph's): without `captured` the larger call would have freed it"""
    from snn_automotive_object_detection_amd import ops
    ws, ws_rates = ops._Workspace(), ops._Workspace()
    monkeypatch.setattr(ops, "_WS", ws)
    monkeypatch.setattr(ops, "_WS_RATES", ws_rates)
    small, large, larger = det(1, 64, 6), det(29, 64, 12), det(65, 64, 24)       # workspace queries of 25 KB, 506 KB, 2.4 MB

    def outputs_case(s):
        """the spec's call in spike-rate mode, observed through its outputs, time sums and spike counts alone: the plane readers of
        tests/_planes.py look into the workspace of the CURRENT stream, which is not the one a graph captured on the side stream holds"""
        ctx = E.prepare(s, gpu_device, ("case", "full"))
        args = dict(ctx["args"], spike_rates=True)
        fc = GC.FnCase((s["entry"],), gpu_device, [tuple(ctx["sets"][n]) for n in ("case", "full")], lambda x4: ops.det_head_forward(x4.flatten(1), T=s["T"], **args))
        fc.keep = ctx
        return fc

    torch.cuda.graph(torch.cuda.CUDAGraph())                      # (constructing the context makes torch's one capture stream; nothing is captured)
    side = torch.cuda.graph.default_capture_stream
    assert side is not None and side != torch.cuda.current_stream()
    key = lambda st: (gpu_device.type, gpu_device.index, st.cuda_stream)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # an eager call of the small case on the capture stream: its buffer comes from the general pool
        E.run(small, gpu_device)["oracle"]()
    torch.cuda.synchronize()
    pre = ws.buf[key(side)]
    a = GC.capture_case(outputs_case(small), GC.HipGraph())
    assert ws.buf[key(side)] is pre and any(c is pre for c in ws.captured), "graph A was not handed the buffer the stream already had"
    b = GC.capture_case(outputs_case(large), GC.HipGraph())
    held_b = ws.buf[key(side)]
    assert held_b is not pre and held_b.numel() > pre.numel() and any(c is held_b for c in ws.captured)
    with torch.cuda.stream(side):
        E.run(larger, gpu_device)["oracle"]()
    E.run(larger, gpu_device)["oracle"]()
    torch.cuda.synchronize()
    assert ws.buf[key(side)].numel() > held_b.numel() and ws.buf[key(side)] is not held_b
    assert [c.data_ptr() for c in ws.captured[:2]] == [pre.data_ptr(), held_b.data_ptr()]       # still alive, at the addresses the graphs hold
    a.replay(1)
    b.replay(1)
    a.replay(0)
    b.strategy.release()
    del b
    a.replay(1)
    a.replay(0)


def entries_reached():
    """the ops functions the cases of this file replay (tests/test_graph_capture_cpu.py compares it with the classification)"""
    out = {s["entry"] for s, _ in HEADS + TYPED + ROUTES} | {s["entry"] for s, _, _ in POST} | set(STAGE_ENTRIES.values())
    return out | {"li_heads", "li_heads_readouts"} | set(StaticCase.entries)
