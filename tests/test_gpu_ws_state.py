"""Heads and post-processing must not depend on what their workspace held before, and must stay inside the size they asked for.

Every call here reaches the library through the seam of tests/_ws_state.py: ops._WS / ops._WS_RATES are GuardedWorkspaces, so the library is
told EXACTLY the size its own query returned, the bytes around that region are guarded, and the region's prior contents are chosen.  Outputs
are allocated by ops inside W.poisoned_outputs(): NaN / 0x5a before the call.  The cases are the smallest of the suite's own exact builders
(tests/_exact_grid.py, tests/_conv_route.py, tests/_fc6_route.py, tests/_post_grid.py), so the expectation is the oracle with zero flips and
not only self-agreement; each case asserts the launch plan it is meant to reach (snn_debug_last_conv_path / snn_debug_last_fc6_path).

  (b) sequences on one buffer (they come first in the file: they run before the fills): each step returns the bits of the same call alone
      on freshly armed zeros - large then small, the product's order, route flips, counter sharing, plane forms, precisions, T;
  (a) per entry of _ws_state.ENTRIES and per fill 0x00 / 0x5a / 0xff: guards and tail intact, the snapshot bit-equal to the 0x00 one, and the
      0x00 one equal to the oracle (hidden planes and counts with zero flips, outputs within CUR_TOL of fp64 on those planes and 1e-4 of the
      oracle, post-processing with the zero-tolerance asserts of tests/test_gpu_post_grid.py);
  (c) a workspace one byte too small: an error, nothing enqueued - poisoned outputs stay poisoned, the armed buffer stays armed.
A snapshot = outputs, time sums, spike counts, rate rows, route_stat and the hidden planes (through the debug accessors)."""
import functools

import numpy as np
import pytest
import torch

from tests import _conv_route as CR
from tests import _exact_grid as G
from tests import _fc6_route as FR
from tests import _post_grid as PG
from tests import _ws_state as W
from tests._planes import CUR_TOL, head_det_planes, head_rpn_planes, li_constants, li_fp64
from tests._util import SCORE_ATOL, nchw_to_rows, planes_to_dense

pytestmark = pytest.mark.gpu
TOL = 1e-4                                   # outputs against the oracle (tests/test_gpu_exact_grid.py)
ROI_T = 12
B3 = ("bf16x3", "bf16")                      # the precisions whose conv / fc6 report their launch


# ---- the seam ----------------------------------------------------------------------------------------------------------------------------
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
    yield buffers
    for b in buffers:
        b.short_by = 0


# ---- specs: plain dicts (nothing is built at collection time) -----------------------------------------------------------------------------
def rpn(C, T, inp="case", variant="plain", precision="bf16x3", shapes=W.PYRAMID, N=2, feat=None, nhwc=False, entry="rpn_head_forward",
        ws="_WS", in_shapes=None):
    """inp: "case" (the builder's own N(0, 1.7) maps), "silent", "mixed", "full" (tests/_conv_route.py); in_shapes: the maps' pyramid where
    it is not the case's (the weights do not depend on it)"""
    return dict(kind="rpn", entry=entry, ws=ws, variant=variant, C=C, T=T, inp=inp, precision=precision, shapes=shapes, N=N, feat=feat, nhwc=nhwc,
                in_shapes=in_shapes or shapes)


def det(R, C, T, inp="case", variant="plain", precision="bf16x3", feat=None, entry="det_head_forward", ws="_WS"):
    return dict(kind="det", entry=entry, ws=ws, variant=variant, R=R, C=C, T=T, inp=inp, precision=precision, feat=feat)


def roi(variant="plain", feat=None, nhwc=False, entry="det_head_forward_roialign"):
    return dict(kind="roi", entry=entry, ws="_WS", variant=variant, R=38, C=64, T=ROI_T, precision="bf16x3", feat=feat, nhwc=nhwc)


def post(entry, **kw):
    return dict(kind={"batched_nms": "nms", "nms_keep_mask": "nms"}.get(entry, entry), entry=entry, ws="_WS", variant="plain", **kw)


def spec_id(s) -> str:
    parts = [s["entry"]] + ([] if s["ws"] == "_WS" else ["rates_ws"]) + [s["variant"]]
    if s["kind"] == "rpn":
        parts += ["C%d" % s["C"], "T%d" % s["T"], s["inp"]] + ([] if s["in_shapes"] == W.PYRAMID else ["x".join("%d_%d" % hw for hw in s["in_shapes"])])
    elif s["kind"] == "det":
        parts += ["R%d" % s["R"], "C%d" % s["C"], "T%d" % s["T"], s["inp"]]
    elif s["kind"] == "nms":
        parts += ["n%d" % s["n"]]
    if s.get("precision", "bf16x3") != "bf16x3":
        parts.append(s["precision"])
    if s.get("feat"):
        parts.append(s["feat"] + ("_nhwc" if s.get("nhwc") else ""))
    return "-".join(parts)


# ---- cases and their oracles (host; built once, shared by every test that names them) ------------------------------------------------------
def _grid(precision):
    return "narrow" if precision == "bf16" else "wide"          # (the single bf16 plane carries the narrow grid exactly)


@functools.lru_cache(maxsize=None)
def _rpn_case(C, T, shapes, N, grid, feat):
    if feat is not None:
        assert (C, T, shapes, N, grid) == (64, 8, W.PYRAMID, 2, "wide")
        return G.rpn_feat_case(feat)
    if shapes == W.PYRAMID and N == 2:
        return G.rpn_t_case(C, T, grid)
    return G.rpn_case(C, 3, T, shapes, N, C + T, grid)


@functools.lru_cache(maxsize=None)
def _rpn_oracle(C, T, shapes, N, grid, feat, inp, in_shapes):
    """(features, oracle planes [T, P, C], counts [levels, N], logits, bbox) of the case's weights on the named input"""
    case = _rpn_case(C, T, shapes, N, grid, feat)
    if inp == "case":
        assert in_shapes == shapes
        return case["feats"], case["spk"], case["counts"], case["logits"], case["bbox"]
    from oracle import snn_oracle as OR
    feats = {"silent": lambda: CR.silent_maps(C, in_shapes, N), "mixed": lambda: CR.mixed_maps(C, T, in_shapes, N, C + T),
             "full": lambda: CR.full_nibble_maps(C, T, in_shapes, N, C + T)}[inp]()
    counts = []
    with torch.no_grad():
        logits, bbox, traces = OR.rpn_head_forward(feats, case["w_shared"], case["w_cls"], case["w_bbox"], T, li_order=case["li_order"], trace=True,
                                                   counts_out=counts)
    spk = np.concatenate([nchw_to_rows(tr["spk"]) for tr in traces], axis=1)
    return feats, spk, torch.stack(counts).numpy(), logits, bbox


@functools.lru_cache(maxsize=None)
def _det_case(R, C, T, grid, feat):
    if feat is not None:
        assert (R, C, T, grid) == (29, 64, 12, "wide")
        return G.det_feat_case(feat)
    if C == 128:
        assert (R, T) == (37, 12)
        return G.det_mx_case(grid)
    if R == 29 and C == 64:
        return G.det_t_case(T, grid)
    if T == 12:
        return G.det_r_case(R, C)
    return G.det_case(R, C, 128, 9, T, 700 + R + T, grid)


def _det_oracle_on(case, x):
    from oracle import snn_oracle as OR
    counts = []
    with torch.no_grad():
        cls, bbox, tr = OR.det_head_forward(x, case["w6"], case["w7"], case["w_cls"], case["w_bbox"], case["T"], li_order=case["li_order"], trace=True,
                                            counts_out=counts)
    return x, tr["spk6"].numpy(), tr["spk7"].numpy(), [c.numpy() for c in counts], cls, bbox


@functools.lru_cache(maxsize=None)
def _det_oracle(R, C, T, grid, feat, inp):
    """(features [R, C, 7, 7], oracle spk6, spk7 [T, R, Hd], counts (c6, c7), cls, bbox)"""
    case = _det_case(R, C, T, grid, feat)
    if inp == "case":
        tr = case["trace"]
        return case["x"], tr["spk6"].numpy(), tr["spk7"].numpy(), case["counts"], case["cls"], case["bbox"]
    full = G.full_nibble_values((R, C, 7, 7), T, torch.Generator().manual_seed(R + T))
    return _det_oracle_on(case, {"full": full, "silent": FR.silent_like(full), "mixed": FR.mixed_like(full)}[inp])


@functools.lru_cache(maxsize=None)
def _roi_oracle(feat):
    """the RoIAlign feed of tests/_fc6_route.py (two levels, two images, 38 boxes) with the weights of det_t_case(12): the pooled features come
    from the host restatement of roi_align (bit-identical to the fused kernel: tests/test_gpu_roialign.py), the planes from the oracle on them"""
    case = G.det_t_case(ROI_T)
    pool, feats, boxes, shapes = FR.roi_setup(64, 38, 40 + ROI_T)
    if feat is not None:
        feats = {k: v.to({"fp16": torch.float16, "bf16": torch.bfloat16}[feat]) for k, v in feats.items()}
    return (pool, feats, boxes, shapes) + _det_oracle_on(case, FR.roi_pooled(feats, boxes, shapes))[1:]


_HEADS = {}


def _head(kind, key, case, dev, precision):
    """the head module of a case (its packed weights are cached on it)"""
    k = (kind, key, precision, str(dev))
    if k not in _HEADS:
        _HEADS[k] = (CR if kind == "rpn" else FR).head_for(case, dev, precision)
        assert _HEADS[k]._resolve_precision() == precision
    return _HEADS[k]


def _heads_w(case, precision):
    w = torch.cat([case["w_cls"].flatten(1), case["w_bbox"].flatten(1)])
    return w.to(torch.bfloat16).float() if precision == "bf16" else w


def _to_dev(x, dev, feat, nhwc):
    x = x.to(dev)
    if feat is not None:
        x = x.to({"fp16": torch.float16, "bf16": torch.bfloat16}[feat])
    return x.contiguous(memory_format=torch.channels_last) if nhwc else x


class Record(list):
    """the tensors ops allocated during a call (W.poisoned_outputs), and the route_stat the call was handed"""
    stat = None


def _route_kw(variant, dev, key, record=None):
    """-> (keywords of the routed entry, route_stat or None)"""
    if variant in ("plain", "rates"):
        return {}, None
    stat = torch.full((4,), -7, dtype=torch.int32, device=dev)
    if isinstance(record, Record):
        record.stat = stat
    route, cross = {"sparse": ("sparse", None), "dense": ("dense", None), "auto": ("auto", None), "auto_never": ("auto", 2.0),
                    "auto_always": ("auto", -1.0)}[variant]
    return {key + "_route": route, key + "_crossover": cross, "route_stat": stat}, stat


def _stat_list(stat):
    return None if stat is None else stat.tolist()


_COUNTS = {}


def _route_counts(key, count):
    """(hits, blocks) of the numpy restatement, once per input"""
    if key not in _COUNTS:
        _COUNTS[key] = tuple(count())
    return _COUNTS[key]


def _stat_want(variant, sparse_plan, counts, dflt):
    """route_stat as include/snn_hip.h documents it: {hits, blocks, route taken, 0}"""
    if variant in ("plain", "rates"):
        return None
    if not sparse_plan:
        return [0, 0, 1, 0]
    if variant in ("sparse", "dense"):
        return [0, 0, int(variant == "dense"), 0]
    hits, blocks = counts()
    cross = {"auto": dflt, "auto_never": 2.0, "auto_always": -1.0}[variant]
    return [hits, blocks, int(np.float32(hits) > np.float32(cross) * np.float32(blocks)), 0]


# ---- the RPN head ------------------------------------------------------------------------------------------------------------------------
def _rpn_plan(s):
    """the launch the conv reports: 1 sparse, 0 dense, 2 the gated pair; None where nothing reports (f32, mxfp6) or the plan is not pinned"""
    if s["precision"] not in B3 or s["in_shapes"] != s["shapes"]:
        return None
    if not 5 <= s["T"] <= 16:
        return 0
    return {"plain": 1, "rates": 1, "sparse": 1, "dense": 0}.get(s["variant"], 2)


def run_rpn(s, dev, record=None):
    from snn_automotive_object_detection_amd import _lib, ops
    C, T, precision, variant = s["C"], s["T"], s["precision"], s["variant"]
    key = (C, T, s["shapes"], s["N"], _grid(precision), s["feat"])
    case = _rpn_case(*key)
    cpu_feats, spk, counts_e, logits_e, bbox_e = _rpn_oracle(*key, s["inp"], s["in_shapes"])
    if precision == "mxfp6":
        assert G.mx_block_span_bits(case["w_shared"], case["info"]["s"]) <= 27         # (the digit planes carry the grid exactly)
    m = _head("rpn", key, case, dev, precision)
    C_, A, p, w_shared, w_heads = m._pass_args()
    feats = [_to_dev(f, dev, s["feat"], s["nhwc"]) for f in cpu_feats]
    rates = variant == "rates"
    readouts = s["entry"] == "rpn_head_forward_readouts"
    steps = W.READOUT_STEPS if readouts else (T,)
    assert steps[-1] == T
    kw, stat = _route_kw(variant, dev, "conv", record)
    with W.poisoned_outputs(record):
        if readouts:
            out_l, out_b, rows, (counts, sum_l, sum_b, rate_rows) = ops.rpn_head_forward_readouts(feats, C_, A, steps, p, w_shared, w_heads, spike_rates=rates)
        else:
            out_l, out_b, rows, (counts, sum_l, sum_b, rate_rows) = ops.rpn_head_forward(feats, C_, A, T, p, w_shared, w_heads, spike_rates=rates, **kw)
    path = _lib.load().snn_debug_last_conv_path()
    planes = head_rpn_planes(dev, T, C)
    res = dict(snap=W.snapshot(out_l, out_b, counts, sum_l, sum_b, rate_rows, stat, planes), path=path)

    def oracle():
        plan = _rpn_plan(s)
        assert plan is None or path == plan, "%s: the conv reported launch %d, this case is about %d" % (spec_id(s), path, plan)
        got = planes_to_dense(planes, C)
        diff = got != spk
        assert not diff.any(), "hidden planes differ from the oracle's at (step, position, channel) %s ... (%d in all)" % (np.argwhere(diff)[:4].tolist(), int(diff.sum()))
        a, b = li_constants(None)
        last, _ = li_fp64(spk, _heads_w(case, precision), a, b, case["li_order"])
        o = torch.cat([out_l, out_b], dim=-1).double().cpu().numpy().reshape(len(steps), spk.shape[1], 5 * A)
        pos = 0
        for l, (H, Wd) in enumerate(s["in_shapes"]):
            n = s["N"] * H * Wd
            for j, t in enumerate(steps):
                assert np.abs(o[j, pos:pos + n] - last[t - 1, pos:pos + n]).max() <= CUR_TOL
            e = torch.cat([logits_e[l], bbox_e[l]], dim=1).permute(0, 2, 3, 1).reshape(n, 5 * A).numpy()
            assert np.abs(o[-1, pos:pos + n] - e).max() <= TOL
            pos += n
        if rates:
            c = counts.cpu().numpy().reshape(len(steps), len(feats), -1)
            assert np.array_equal(c[-1][:, :s["N"]], counts_e)
            assert all(torch.isfinite(r).all() for r in (rate_rows if readouts else [rate_rows]))
        if plan is not None:                                     # (5 <= T <= 16: the configurations with a sparse plan)
            want = _stat_want(variant, 5 <= T <= 16, lambda: _route_counts(("rpn",) + key + (s["inp"], s["in_shapes"]), lambda: CR.route_counts(cpu_feats, T)), _lib.ROUTE_DEFAULT_CROSSOVER)
            assert _stat_list(stat) == want, "route_stat %s, documented %s" % (_stat_list(stat), want)
        res["stat"] = _stat_list(stat)
    res["oracle"] = oracle
    return res


# ---- the detector head -------------------------------------------------------------------------------------------------------------------
def _det_plan(s):
    if s["precision"] not in B3:
        return None
    if s["C"] % 64:
        return 0                                                 # 49 C / 32 odd: fc6 on the dense tile
    return {"plain": 1, "rates": 1, "sparse": 1, "dense": 0}.get(s["variant"], 2)


def _check_det(s, case, precision, planes6, planes7, out, counts, e6, e7, counts_e, cls_e, bbox_e, steps, rates):
    T, Hd = s["T"], case["Hd"]
    n6 = T if rates else T - 1                                   # (without the counts lif6's spikes of the last step are never read and not formed)
    g6, g7 = planes_to_dense(planes6, Hd), planes_to_dense(planes7, Hd)
    d6, d7 = g6[:n6] != e6[:n6], g7 != e7
    assert not d6.any(), "lif6 planes differ at (step, RoI, unit) %s ... (%d in all)" % (np.argwhere(d6)[:4].tolist(), int(d6.sum()))
    assert not d7.any(), "lif7 planes differ at (step, RoI, unit) %s ... (%d in all)" % (np.argwhere(d7)[:4].tolist(), int(d7.sum()))
    a, b = li_constants(None)
    last, _ = li_fp64(e7, _heads_w(case, precision), a, b, case["li_order"])
    o = torch.cat(out, dim=-1).double().cpu().numpy().reshape(len(steps), e7.shape[1], -1)
    for j, t in enumerate(steps):
        assert np.abs(o[j] - last[t - 1]).max() <= CUR_TOL
    assert np.abs(o[-1] - torch.cat([cls_e, bbox_e], dim=1).numpy()).max() <= TOL
    if rates:
        c6, c7 = [c.cpu().numpy().astype(np.int64).reshape(len(steps), -1)[-1] for c in counts]
        assert np.array_equal(c6, counts_e[0]) and np.array_equal(c7, counts_e[1])


def run_det(s, dev, record=None):
    from snn_automotive_object_detection_amd import _lib, ops
    R, C, T, precision, variant = s["R"], s["C"], s["T"], s["precision"], s["variant"]
    key = (R, C, T, _grid(precision), s["feat"])
    case = _det_case(*key)
    x_cpu, e6, e7, counts_e, cls_e, bbox_e = _det_oracle(*key, s["inp"])
    if precision == "mxfp6":
        assert G.mx_block_span_bits(case["w6"], case["info6"]["s"]) <= 27 and G.mx_block_span_bits(case["w7"], case["info7"]["s"]) <= 27
    d = _head("det", key, case, dev, precision)
    x = _to_dev(x_cpu, dev, s["feat"], False).flatten(1)
    rates = variant == "rates"
    readouts = s["entry"] == "det_head_forward_readouts"
    steps = W.READOUT_STEPS if readouts else (T,)
    assert steps[-1] == T
    args = dict(d._pass_args(x.shape[1], "rows"), spike_rates=rates)
    kw, stat = _route_kw(variant, dev, "fc6", record)
    with W.poisoned_outputs(record):
        if readouts:
            cls, bbox, extras = ops.det_head_forward_readouts(x, steps=steps, **args)
        else:
            cls, bbox, extras = ops.det_head_forward(x, T=T, **args, **kw)
    path = _lib.load().snn_debug_last_fc6_path()
    p6, p7 = head_det_planes(dev, T, case["Hd"], R)
    n6 = T if rates else T - 1
    res = dict(snap=W.snapshot(cls, bbox, extras, stat, p6[:n6], p7), path=path)

    def oracle():
        plan = _det_plan(s)
        assert plan is None or path == plan, "%s: fc6 reported launch %d, this case is about %d" % (spec_id(s), path, plan)
        _check_det(s, case, precision, p6, p7, (cls, bbox), extras[:2], e6, e7, counts_e, cls_e, bbox_e, steps, rates)
        if plan is not None:
            want = _stat_want(variant, C % 64 == 0, lambda: _route_counts(("det",) + key + (s["inp"],), lambda: FR.route_counts(x_cpu.float(), T)), _lib.FC6_ROUTE_DEFAULT_CROSSOVER)
            assert _stat_list(stat) == want, "route_stat %s, documented %s" % (_stat_list(stat), want)
        res["stat"] = _stat_list(stat)
    res["oracle"] = oracle
    return res


def run_roi(s, dev, record=None):
    from snn_automotive_object_detection_amd import _lib, ops
    T, variant = s["T"], s["variant"]
    case = G.det_t_case(T)
    pool, feats, boxes, shapes, e6, e7, counts_e, cls_e, bbox_e = _roi_oracle(s["feat"])
    d = _head("det", ("roi", T), case, dev, "bf16x3")
    dev_feats = {k: _to_dev(v, dev, None, s["nhwc"]) for k, v in feats.items()}
    flist, scales, rois, lvl = pool.assign(dev_feats, [b.to(dev) for b in boxes], shapes)
    assert set(lvl.tolist()) == {0, 1} and int(rois.shape[0]) == s["R"]
    rates = variant == "rates"
    readouts = s["entry"] == "det_head_forward_roialign_readouts"
    steps = W.READOUT_STEPS if readouts else (T,)
    args = dict(d._pass_args(flist[0].shape[1] * 49, "maps"), spike_rates=rates)
    kw, stat = _route_kw(variant, dev, "fc6", record)
    before = dict(ops.feature_calls)
    with W.poisoned_outputs(record):
        if readouts:
            cls, bbox, extras = ops.det_head_forward_roialign_readouts(flist, scales, rois[:, 1:5], rois[:, 0], lvl, steps=steps, **args)
        else:
            cls, bbox, extras = ops.det_head_forward_roialign(flist, scales, rois[:, 1:5], rois[:, 0], lvl, T=T, **args, **kw)
    if s["nhwc"]:
        assert ops.feature_calls["nhwc"] == before["nhwc"] + 1 and ops.feature_calls["no_typed_kernel"] == before["no_typed_kernel"]
    path = _lib.load().snn_debug_last_fc6_path()
    p6, p7 = head_det_planes(dev, T, case["Hd"], s["R"])
    n6 = T if rates else T - 1
    res = dict(snap=W.snapshot(cls, bbox, extras, stat, p6[:n6], p7), path=path)

    def oracle():
        plan = _det_plan(s)
        assert path == plan, "%s: fc6 reported launch %d, this case is about %d" % (spec_id(s), path, plan)
        _check_det(s, case, "bf16x3", p6, p7, (cls, bbox), extras[:2], e6, e7, counts_e, cls_e, bbox_e, steps, rates)
        want = _stat_want(variant, True, lambda: _route_counts(("roi", s["feat"]), lambda: FR.route_counts(FR.roi_pooled(feats, boxes, shapes), T)), _lib.FC6_ROUTE_DEFAULT_CROSSOVER)
        assert _stat_list(stat) == want, "route_stat %s, documented %s" % (_stat_list(stat), want)
    res["oracle"] = oracle
    return res


# ---- post-processing ---------------------------------------------------------------------------------------------------------------------
def _close_scores(got, exp, what):
    got, exp = got.detach().cpu().double(), exp.double()
    assert got.shape == exp.shape, what
    if got.numel():
        assert float((got - exp).abs().max()) <= SCORE_ATOL, "%s: scores differ by %g" % (what, float((got - exp).abs().max()))


def run_nms(s, dev, record=None):
    from oracle import torchvision_restated as TV
    from snn_automotive_object_detection_amd import ops
    c = PG.nms_case(s["n"], 0.5, s["ncat"], s["layout"])
    b, sc, i = c["boxes"].to(dev), c["scores"].to(dev), c["idxs"].to(dev)
    with W.poisoned_outputs(record):
        if s["entry"] == "batched_nms":
            kept = ops.batched_nms(b, sc, i, 0.5)
        else:
            order, mask = ops.nms_keep_mask(b, sc, i, 0.5)
            kept = order[mask]
    res = dict(snap=W.snapshot(kept))

    def oracle():
        assert torch.equal(kept.cpu(), TV.batched_nms(c["boxes"], c["scores"], c["idxs"], 0.5))
    res["oracle"] = oracle
    return res


def run_rpn_proposals(s, dev, record=None):
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd.stock.anchors import AnchorGenerator
    spec = PG.rpn_spec(s["spec"])
    lg, de, hw, strides = PG.rpn_device_inputs(spec, dev)
    ag = AnchorGenerator(spec["geo"]["sizes"], spec["geo"]["ratios"])
    with W.poisoned_outputs(record):
        boxes, scores, counts, pre_b, pre_p = ops.rpn_proposals(lg, de, hw, strides, ag.cell_anchors, spec["image_sizes"], spec["pre"], spec["post"],
                                                                 spec["nms"], spec["score_thresh"], spec["min_size"])
    res = dict(snap=W.snapshot(boxes, scores, counts, pre_b, pre_p))

    def oracle():
        e_b, e_s, e_pre = spec["expected"]
        assert counts.cpu().tolist() == [int(b.shape[0]) for b in e_b]
        for i in range(spec["N"]):
            c = int(e_b[i].shape[0])
            assert torch.equal(boxes[i, :c].cpu(), e_b[i]), "image %d: proposals" % i
            _close_scores(scores[i, :c], e_s[i], "image %d" % i)
            assert not bool(boxes[i, c:].any()) and not bool(scores[i, c:].any()), "image %d: rows behind the count" % i
            assert torch.equal(pre_b[i].cpu(), e_pre[i]["proposals"]), "image %d: pre-NMS boxes" % i
            _close_scores(pre_p[i], e_pre[i]["objectness"], "image %d pre-NMS" % i)
    res["oracle"] = oracle
    return res


def run_det_postprocess(s, dev, record=None):
    from snn_automotive_object_detection_amd import ops
    spec = PG.det_spec(s["spec"])
    K, rois, N = spec["K"], spec["rois"], len(spec["rois"])
    padded = s["entry"] == "det_postprocess_padded"
    with W.poisoned_outputs(record):
        if padded:
            lg, rg, pr, cn, cap = PG.det_padded_inputs(spec, dev)
            boxes, scores, labels, counts, all_s, all_b = ops.det_postprocess_padded(
                lg, rg, pr, cn, list(spec["image_shapes"]), PG.BOX_WEIGHTS, PG.DET_SCORE_THRESH, spec["nms"], spec["det"])
        else:
            boxes, scores, labels, counts, all_s, all_b = ops.det_postprocess(
                spec["logits"].to(dev), spec["reg"].to(dev), torch.cat(spec["props"]).to(dev), rois, list(spec["image_shapes"]), PG.BOX_WEIGHTS,
                PG.DET_SCORE_THRESH, spec["nms"], spec["det"])
    # (the compacted form leaves the rows behind the counts unwritten: they are NaN / 0x5a in every run, which the snapshot pins as well)
    res = dict(snap=W.snapshot(boxes, scores, labels, counts, all_s, all_b))

    def oracle():
        e_b, e_s, e_l, e_as, e_ab = spec["expected"]
        cnt = counts.cpu().tolist()
        cap = max(rois)
        pos = 0
        for i in range(N):
            n_fg, n_all = int((e_l[i] > 0).sum()), int(e_l[i].shape[0])
            assert cnt[i] == [n_fg, n_all - n_fg], "image %d: counts %s" % (i, cnt[i])
            assert torch.equal(labels[i, :n_all].cpu().to(torch.int64), e_l[i]), "image %d: labels" % i
            assert torch.equal(boxes[i, :n_all].cpu(), e_b[i]), "image %d: boxes" % i
            _close_scores(scores[i, :n_all], e_s[i], "image %d" % i)
            ab = all_b.view(N, cap, K, 4)[i, :rois[i]] if padded else all_b[pos:pos + rois[i]]
            asc = all_s.view(N, cap, K)[i, :rois[i]] if padded else all_s[pos:pos + rois[i]]
            assert torch.equal(ab.cpu(), e_ab[i]), "image %d: all_boxes" % i
            _close_scores(asc, e_as[i], "image %d all_scores" % i)
            if padded:
                assert not bool(boxes[i, n_all:].any()) and not bool(scores[i, n_all:].any()) and not bool(labels[i, n_all:].any())
                assert not bool(all_b.view(N, cap, K, 4)[i, rois[i]:].any()) and not bool(all_s.view(N, cap, K)[i, rois[i]:].any())
            pos += rois[i]
    res["oracle"] = oracle
    return res


BUILDERS = {
    ("rpn_head_forward", "_WS"): run_rpn, ("rpn_head_forward", "_WS_RATES"): run_rpn,
    ("rpn_head_forward_readouts", "_WS"): run_rpn, ("rpn_head_forward_readouts", "_WS_RATES"): run_rpn,
    ("det_head_forward", "_WS"): run_det, ("det_head_forward_readouts", "_WS"): run_det,
    ("det_head_forward_roialign", "_WS"): run_roi, ("det_head_forward_roialign_readouts", "_WS"): run_roi,
    ("batched_nms", "_WS"): run_nms, ("nms_keep_mask", "_WS"): run_nms, ("rpn_proposals", "_WS"): run_rpn_proposals,
    ("det_postprocess", "_WS"): run_det_postprocess, ("det_postprocess_padded", "_WS"): run_det_postprocess,
}


def run(s, dev, record=None):
    return BUILDERS[(s["entry"], s["ws"])](s, dev, record)


def call(s, dev):
    """the spec as a call() -> snapshot for the runners of tests/_ws_state.py; the oracle comparison runs inside every call"""
    def go():
        r = run(s, dev)
        r["oracle"]()
        return r["snap"]
    return go


# ---- (b) sequences on one buffer ---------------------------------------------------------------------------------------------------------
RO = dict(entry="rpn_head_forward_readouts")
DRO = dict(entry="det_head_forward_readouts")
SEQUENCES = {
    "large_then_small_rpn": [rpn(128, 16, "full"), rpn(64, 5, "silent", in_shapes=W.ONE_BY_ONE)],
    "large_then_small_det": [det(65, 64, 24), det(1, 64, 6)],
    "product_order": [rpn(64, 8), post("rpn_proposals", spec=W.RPN_POST_SPEC), roi(), post("det_postprocess", spec=W.DET_POST_SPEC),
                      rpn(64, 8, "mixed"), post("rpn_proposals", spec=W.RPN_POST_SPEC)],
    "route_flips_rpn": [rpn(128, 8, "full", "auto"), rpn(128, 8, "silent", "auto"), rpn(128, 8, "mixed", "sparse"), rpn(128, 8, "mixed", "dense"),
                        rpn(128, 8, "mixed", "auto")],
    "route_flips_det": [det(29, 64, 12, "full", "auto"), det(29, 64, 12, "silent", "auto"), det(29, 64, 12, "case", "sparse"),
                        det(29, 64, 12, "case", "dense"), det(29, 64, 12, "case", "auto")],
    "counter_sharing_rpn": [rpn(64, 8, "full", "rates"), rpn(64, 8, "mixed", "auto"), rpn(64, 8, "full", "rates")],
    "counter_sharing_det": [det(29, 64, 12, "full", "rates"), det(29, 64, 12, "mixed", "auto"), det(29, 64, 12, "full", "rates")],
    "plane_form_rpn": [rpn(64, 12, "mixed"), rpn(64, 12, "mixed", "auto"), rpn(64, 12, "mixed", **RO), rpn(64, 12, "mixed")],
    "plane_form_det": [det(29, 64, 12), det(29, 64, 12, "case", "auto"), det(29, 64, 12, **DRO), det(29, 64, 12)],
    "precisions": [rpn(128, 8, "mixed"), rpn(128, 8, "mixed", precision="f32"), rpn(128, 8, "mixed", precision="mxfp6"),
                   rpn(128, 8, "mixed", precision="bf16"), rpn(128, 8, "mixed")],
    "T_rpn": [rpn(64, 16, "mixed"), rpn(64, 5, "mixed"), rpn(64, 8, "mixed"), rpn(64, 4, "mixed")],
    "T_det": [det(29, 64, 24), det(29, 64, 6), det(29, 64, 12)],
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_sequence_on_one_buffer(gpu_device, seam, name):
    """each step returns the bits of the same call alone on freshly armed zeros (and meets its oracle both times); the buffer is armed once,
    with 0x5a, before the first step"""
    specs = SEQUENCES[name]
    W.run_sequence(seam, [call(s, gpu_device) for s in specs], start_fill=0x5a)
    assert seam[0].sizes and len(seam[0].sizes) >= len(specs)


def test_route_flips_take_the_side_the_input_names(gpu_device, seam):
    """the first two steps of the route sequences: `auto` at the header's crossover takes the dense side on full-nibble input and the sparse
    side on silent input (route_stat[2]; run_rpn / run_det compare the whole array with the restated count)"""
    for s, route in [(SEQUENCES["route_flips_rpn"][0], 1), (SEQUENCES["route_flips_rpn"][1], 0), (SEQUENCES["route_flips_det"][0], 1),
                     (SEQUENCES["route_flips_det"][1], 0)]:
        for b in seam:
            b.arm(0x00)
        r = run(s, gpu_device)
        r["oracle"]()
        assert r["path"] == 2 and r["stat"][2] == route and r["stat"][1] > 0 and (r["stat"][0] > 0) == bool(route), (spec_id(s), r["stat"])


# ---- (a) contents and exact size, per entry and fill --------------------------------------------------------------------------------------
def _fill_specs():
    out = []
    # the RPN head: the sparse window's edges, both FAT shapes and the 8-wave shape, on every input
    out += [rpn(C, T, inp) for C in (64, 128) for T in (5, 8, 16) for inp in ("silent", "mixed", "full")]
    out += [rpn(C, T, inp, v) for C, T, inp in ((64, 8, "mixed"), (128, 16, "full")) for v in W.HEAD_VARIANTS[1:]]
    out += [rpn(64, 8, "mixed", "rates", ws="_WS_RATES")]
    out += [rpn(256, 8, inp, v, shapes=W.SPLIT_PYRAMID) for inp, v in (("mixed", "plain"), ("full", "auto_never"), ("case", "rates"))]
    out += [rpn(64, 4, "mixed", v) for v in ("plain", "rates", "auto_always")]                     # the dense plan
    out += [rpn(64, 8, "mixed", precision="f32"), rpn(64, 8, "mixed", precision="bf16"), rpn(128, 8, "mixed", precision="mxfp6")]
    out += [rpn(64, 8, "case", feat="fp16", nhwc=True)]
    out += [rpn(64, 12, "mixed", v, **RO) for v in ("plain", "rates")] + [rpn(64, 12, "mixed", "rates", ws="_WS_RATES", **RO)]
    # the detector head
    out += [det(29, 64, T) for T in (6, 12, 16, 24)]
    out += [det(R, C, 12) for R in (1, 17, 65) for C in (32, 64)]                                    # R = 17: a partly filled RoI group
    out += [det(R, 64, 12, inp, v) for R, inp in ((29, "case"), (17, "case"), (29, "full")) for v in W.HEAD_VARIANTS[1:]]
    out += [det(29, 64, 12, "silent")]
    out += [det(29, 64, 12, precision="f32"), det(29, 64, 12, precision="bf16"), det(37, 128, 12, precision="mxfp6")]
    out += [det(29, 64, 12, feat="fp16")]
    out += [det(29, 64, 12, "case", v, **DRO) for v in ("plain", "rates")]
    out += [roi(v) for v in W.ENTRIES[("det_head_forward_roialign", "_WS")]] + [roi("rates"), roi("plain", feat="fp16", nhwc=True)]
    out += [roi(v, entry="det_head_forward_roialign_readouts") for v in ("plain", "rates")]
    # post-processing
    out += [post(e, n=n, ncat=3, layout=lay) for e in ("batched_nms", "nms_keep_mask") for n, lay in ((65, 3), (129, 5))]
    out += [post("rpn_proposals", spec=W.RPN_POST_SPEC), post("det_postprocess", spec=W.DET_POST_SPEC), post("det_postprocess_padded", spec=W.DET_POST_SPEC)]
    return out


FILL_SPECS = _fill_specs()
_ZERO_SNAPS = {}


def _buffers_of(seam, s):
    return list(seam) if s["kind"] == "rpn" else [seam[0]]


@pytest.mark.parametrize("s,fill", [(s, f) for s in FILL_SPECS for f in W.FILLS], ids=["%s-fill%02x" % (spec_id(s), f) for s in FILL_SPECS for f in W.FILLS])
def test_contents_and_exact_size(gpu_device, seam, s, fill):
    """armed with `fill`, told exactly the queried size: guards and tail intact, the oracle met, the snapshot bit-equal to the 0x00 one"""
    key = spec_id(s)
    if key not in _ZERO_SNAPS:
        _ZERO_SNAPS[key] = W.armed_call(_buffers_of(seam, s), 0x00, call(s, gpu_device))
    if fill != 0x00:
        snap = W.armed_call(_buffers_of(seam, s), fill, call(s, gpu_device))
        assert W.same_bits(snap, _ZERO_SNAPS[key]), "fill 0x%02x against 0x00: %s" % (fill, W.first_difference(snap, _ZERO_SNAPS[key]))
    assert seam[0].sizes and seam[0].high == seam[0].sizes[-1]           # (the region was the query's size, to the byte)


# ---- (c) too small by one byte -----------------------------------------------------------------------------------------------------------
SHORT_SPECS = ([rpn(64, 8, "mixed", v) for v in W.HEAD_VARIANTS] + [rpn(64, 8, "mixed", "rates", ws="_WS_RATES")]
               + [rpn(64, 12, "mixed", v, **RO) for v in ("plain", "rates")] + [rpn(64, 12, "mixed", "rates", ws="_WS_RATES", **RO)]
               + [det(29, 64, 12, "case", v) for v in W.HEAD_VARIANTS] + [det(29, 64, 12, "case", v, **DRO) for v in ("plain", "rates")]
               + [roi(v) for v in W.ENTRIES[("det_head_forward_roialign", "_WS")]]
               + [roi(v, entry="det_head_forward_roialign_readouts") for v in ("plain", "rates")]
               + [post(e, n=65, ncat=3, layout=3) for e in ("batched_nms", "nms_keep_mask")]
               + [post("rpn_proposals", spec=W.RPN_POST_SPEC), post("det_postprocess", spec=W.DET_POST_SPEC),
                  post("det_postprocess_padded", spec=W.DET_POST_SPEC)])


@pytest.mark.parametrize("s", SHORT_SPECS, ids=[spec_id(s) for s in SHORT_SPECS])
def test_one_byte_too_small_is_refused_with_nothing_enqueued(gpu_device, seam, s):
    """the seam hands out need - 1 bytes: the call returns its error (snn_last_error names the workspace) before any device work - every output
    ops allocated for it is still NaN / 0x5a, route_stat still -7, the armed buffer untouched.  (The rates call sits behind a head call that
    runs: there the claim is about the rates buffer and the rate rows.)"""
    from snn_automotive_object_detection_amd import _lib
    main, rates = seam
    target = rates if s["ws"] == "_WS_RATES" else main
    for b in seam:
        b.arm(0x5a)
    target.short_by = 1
    record = Record()
    with pytest.raises(_lib.SnnHipError, match=r"rc=-[12]\b.*workspace"):
        run(s, gpu_device, record)
    torch.cuda.synchronize()
    assert record.stat is None or s["ws"] == "_WS_RATES" or record.stat.tolist() == [-7] * 4
    assert target.sizes and target.size == target.sizes[-1] - 1
    assert target.untouched(), "the refused call wrote to its workspace"
    outs = [t for t in record if t.is_cuda]
    assert outs or s["entry"] == "nms_keep_mask"                      # (its buffers are torch.full / torch.zeros: nothing of it is left unwritten)
    if s["ws"] == "_WS_RATES":
        outs = outs[-1:]                                                # the rate rows (allocated right before the refused call)
    assert all(W.still_poisoned(t) for t in outs), "the refused call wrote to an output"
    for b in seam:
        b.check()


def all_specs():
    """every spec this file runs (tests/test_ws_state_cpu.py asks the size queries about their shapes)"""
    return [s for seq in SEQUENCES.values() for s in seq] + FILL_SPECS + SHORT_SPECS
