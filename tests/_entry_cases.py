"""One set of case builders for the entries of tests/_ws_state.ENTRIES, shared by the workspace seam (tests/test_gpu_ws_state.py) and by graph
capture (tests/test_gpu_graph_capture.py) (test infrastructure).

A spec is a plain dict (rpn / det / roi / post below; nothing is built at collection time).  Each kind has three parts:
  prepare_*(s, dev, inputs) -> ctx   the host case (the smallest of the suite's exact builders: tests/_exact_grid.py, _conv_route.py, _fc6_route.py,
                                     _post_grid.py) and its STATIC device operands, holding input set inputs[0]; `inputs` names further input sets
                                     of the same shapes and weights.  Everything that copies from the host or reads a result back happens here;
  load(ctx, name)                    copies input set `name` into the static operands with copy_ (nothing is reallocated);
  call_*(ctx, record) -> res         ONE ops call on the static operands: no host <-> device copy, so it may sit inside a stream capture.
                                     res["source"]() reads back what a caller can observe (outputs, time sums, spike counts, rate rows, route_stat,
                                     device-side counts and the rows behind them, the hidden planes through the debug accessors) as a
                                     _ws_state.snapshot; res["oracle"](name) makes the zero-flip asserts against the oracle of input set `name` on
                                     what source() read last.
run_*(s, dev, record) = prepare + call + source: the eager runners of tests/test_gpu_ws_state.py."""
import functools

import numpy as np
import torch

from tests import _conv_route as CR
from tests import _exact_grid as G
from tests import _fc6_route as FR
from tests import _post_grid as PG
from tests import _ws_state as W
from tests._planes import CUR_TOL, head_det_planes, head_rpn_planes, li_constants, li_fp64
from tests._util import SCORE_ATOL, nchw_to_rows, planes_to_dense

TOL = 1e-4                                   # outputs against the oracle (tests/test_gpu_exact_grid.py)
ROI_T = 12
B3 = ("bf16x3", "bf16")                      # the precisions whose conv / fc6 report their launch
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


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
    return dict(kind="roi", entry=entry, ws="_WS", variant=variant, R=38, C=64, T=ROI_T, precision="bf16x3", feat=feat, nhwc=nhwc, inp="draw0")


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
    if feat is not None:                                         # (a typed case: the oracle sees the values the typed maps hold)
        feats = [f.to(_DT[feat]).float() for f in feats]
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
    if inp.startswith("decided_"):                               # the inputs tests/_fc6_route.py decides on at the header's crossover
        assert (R, C, T) == (29, 64, 8)
        return _det_oracle_on(case, {n: x for n, x, _ in FR.decided_inputs()}[inp[len("decided_"):]])
    full = G.full_nibble_values((R, C, 7, 7), T, torch.Generator().manual_seed(R + T))
    x = {"full": full, "silent": FR.silent_like(full), "mixed": FR.mixed_like(full)}[inp]
    if feat is not None:
        x = x.to(_DT[feat]).float()
    return _det_oracle_on(case, x)


@functools.lru_cache(maxsize=None)
def _roi_oracle(feat, draw=0):
    """the RoIAlign feed of tests/_fc6_route.py (two levels, two images, 38 boxes) with the weights of det_t_case(12): the pooled features come
    from the host restatement of roi_align (bit-identical to the fused kernel: tests/test_gpu_roialign.py), the planes from the oracle on them.
    draw > 0: another draw of the maps under the boxes of draw 0 (a second input set of the same shapes)"""
    case = G.det_t_case(ROI_T)
    pool, feats, boxes, shapes = FR.roi_setup(64, 38, 40 + ROI_T)
    if draw:
        feats = FR.roi_setup(64, 38, 40 + ROI_T + draw)[1]
    if feat is not None:
        feats = {k: v.to(_DT[feat]) for k, v in feats.items()}
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
        x = x.to(_DT[feat])
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


def _names(s, inputs):
    names = tuple(inputs) if inputs else (s["inp"],)
    assert len(set(names)) == len(names)
    return names


def load(ctx, name) -> None:
    """input set `name` into the static operands (copy_: same buffers, same addresses)"""
    for dst, src in zip(ctx["operands"], ctx["sets"][name]):
        assert dst.shape == src.shape
        dst.copy_(src)
    ctx["loaded"] = name


# ---- the RPN head ------------------------------------------------------------------------------------------------------------------------
def _rpn_plan(s):
    """the launch the conv reports: 1 sparse, 0 dense, 2 the gated pair; None where nothing reports (f32, mxfp6) or the plan is not pinned"""
    if s["precision"] not in B3 or s["in_shapes"] != s["shapes"]:
        return None
    if not 5 <= s["T"] <= 16:
        return 0
    return {"plain": 1, "rates": 1, "sparse": 1, "dense": 0}.get(s["variant"], 2)


def prepare_rpn(s, dev, inputs=None):
    C, T, precision = s["C"], s["T"], s["precision"]
    key = (C, T, s["shapes"], s["N"], _grid(precision), s["feat"])
    case = _rpn_case(*key)
    names = _names(s, inputs)
    host = {n: _rpn_oracle(*key, n, s["in_shapes"]) for n in names}
    if precision == "mxfp6":
        assert G.mx_block_span_bits(case["w_shared"], case["info"]["s"]) <= 27         # (the digit planes carry the grid exactly)
    m = _head("rpn", key, case, dev, precision)
    feats = [_to_dev(f, dev, s["feat"], s["nhwc"]) for f in host[names[0]][0]]
    return dict(s=s, dev=dev, key=key, case=case, host=host, args=m._pass_args(), operands=feats, sets={n: host[n][0] for n in names},
                loaded=names[0], keep=[m])


def call_rpn(ctx, record=None):
    from snn_automotive_object_detection_amd import _lib, ops
    s, dev, key, case, feats = ctx["s"], ctx["dev"], ctx["key"], ctx["case"], ctx["operands"]
    C, T, precision, variant = s["C"], s["T"], s["precision"], s["variant"]
    C_, A, p, w_shared, w_heads = ctx["args"]
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
    res = dict(path=path, tensors=(out_l, out_b, counts, sum_l, sum_b, rate_rows, stat))

    def source():
        res["planes"] = head_rpn_planes(dev, T, C)
        return W.snapshot(out_l, out_b, counts, sum_l, sum_b, rate_rows, stat, res["planes"])

    def oracle(name=None):
        name = ctx["loaded"] if name is None else name
        cpu_feats, spk, counts_e, logits_e, bbox_e = ctx["host"][name]
        planes = res["planes"]
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
            want = _stat_want(variant, 5 <= T <= 16, lambda: _route_counts(("rpn",) + key + (name, s["in_shapes"]), lambda: CR.route_counts(cpu_feats, T)), _lib.ROUTE_DEFAULT_CROSSOVER)
            assert _stat_list(stat) == want, "route_stat %s, documented %s" % (_stat_list(stat), want)
        res["stat"] = _stat_list(stat)
    res["source"], res["oracle"] = source, oracle
    return res


# ---- the detector head -------------------------------------------------------------------------------------------------------------------
def _det_sparse(s):
    """fc6's plan is the sparse launch: 49 C / 32 even, and a window of period planes to compress - T >= 6, or 5 where the spike counts keep
    lif6's last step (tests/test_gpu_every_T.py, tests/test_gpu_exact_grid.py)"""
    return s["C"] % 64 == 0 and s["T"] >= (5 if s["variant"] == "rates" else 6)


def _det_plan(s):
    if s["precision"] not in B3:
        return None
    if not _det_sparse(s):
        return 0                                                 # fc6 on the dense tile
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


def prepare_det(s, dev, inputs=None):
    R, C, T, precision = s["R"], s["C"], s["T"], s["precision"]
    key = (R, C, T, _grid(precision), s["feat"])
    case = _det_case(*key)
    names = _names(s, inputs)
    host = {n: _det_oracle(*key, n) for n in names}
    if precision == "mxfp6":
        assert G.mx_block_span_bits(case["w6"], case["info6"]["s"]) <= 27 and G.mx_block_span_bits(case["w7"], case["info7"]["s"]) <= 27
    d = _head("det", key, case, dev, precision)
    x4 = _to_dev(host[names[0]][0], dev, s["feat"], False)
    x = x4.flatten(1)
    assert x.data_ptr() == x4.data_ptr()
    return dict(s=s, dev=dev, key=key, case=case, host=host, x=x, args=d._pass_args(x.shape[1], "rows"), operands=[x4],
                sets={n: [host[n][0]] for n in names}, loaded=names[0], keep=[d])


def call_det(ctx, record=None):
    from snn_automotive_object_detection_amd import _lib, ops
    s, dev, key, case, x = ctx["s"], ctx["dev"], ctx["key"], ctx["case"], ctx["x"]
    R, C, T, precision, variant = s["R"], s["C"], s["T"], s["precision"], s["variant"]
    rates = variant == "rates"
    readouts = s["entry"] == "det_head_forward_readouts"
    steps = W.READOUT_STEPS if readouts else (T,)
    assert steps[-1] == T
    args = dict(ctx["args"], spike_rates=rates)
    kw, stat = _route_kw(variant, dev, "fc6", record)
    with W.poisoned_outputs(record):
        if readouts:
            cls, bbox, extras = ops.det_head_forward_readouts(x, steps=steps, **args)
        else:
            cls, bbox, extras = ops.det_head_forward(x, T=T, **args, **kw)
    path = _lib.load().snn_debug_last_fc6_path()
    n6 = T if rates else T - 1
    res = dict(path=path, tensors=(cls, bbox, extras, stat))

    def source():
        res["p6"], res["p7"] = head_det_planes(dev, T, case["Hd"], R)
        return W.snapshot(cls, bbox, extras, stat, res["p6"][:n6], res["p7"])

    def oracle(name=None):
        name = ctx["loaded"] if name is None else name
        x_cpu, e6, e7, counts_e, cls_e, bbox_e = ctx["host"][name]
        plan = _det_plan(s)
        assert plan is None or path == plan, "%s: fc6 reported launch %d, this case is about %d" % (spec_id(s), path, plan)
        _check_det(s, case, precision, res["p6"], res["p7"], (cls, bbox), extras[:2], e6, e7, counts_e, cls_e, bbox_e, steps, rates)
        if plan is not None:
            want = _stat_want(variant, _det_sparse(s), lambda: _route_counts(("det",) + key + (name,), lambda: FR.route_counts(x_cpu.float(), T)), _lib.FC6_ROUTE_DEFAULT_CROSSOVER)
            assert _stat_list(stat) == want, "route_stat %s, documented %s" % (_stat_list(stat), want)
        res["stat"] = _stat_list(stat)
    res["source"], res["oracle"] = source, oracle
    return res


def _roi_draw(name) -> int:
    assert name.startswith("draw")
    return int(name[4:])


def prepare_roi(s, dev, inputs=None):
    T = s["T"]
    case = G.det_t_case(T)
    names = _names(s, inputs)
    host = {n: _roi_oracle(s["feat"], _roi_draw(n)) for n in names}
    pool, feats, boxes, shapes = host[names[0]][:4]
    d = _head("det", ("roi", T), case, dev, "bf16x3")
    dev_feats = {k: _to_dev(v, dev, None, s["nhwc"]) for k, v in feats.items()}
    flist, scales, rois, lvl = pool.assign(dev_feats, [b.to(dev) for b in boxes], shapes)
    assert set(lvl.tolist()) == {0, 1} and int(rois.shape[0]) == s["R"]
    assert [f.data_ptr() for f in flist] == [dev_feats[k].data_ptr() for k in ("0", "1")]
    return dict(s=s, dev=dev, case=case, host=host, flist=flist, scales=scales, boxes4=rois[:, 1:5], batch=rois[:, 0], lvl=lvl,
                args=d._pass_args(flist[0].shape[1] * 49, "maps"), operands=list(flist), sets={n: [host[n][1][k] for k in ("0", "1")] for n in names},
                loaded=names[0], keep=[d, rois, dev_feats])


def call_roi(ctx, record=None):
    from snn_automotive_object_detection_amd import _lib, ops
    s, dev, case, flist = ctx["s"], ctx["dev"], ctx["case"], ctx["flist"]
    T, variant = s["T"], s["variant"]
    rates = variant == "rates"
    readouts = s["entry"] == "det_head_forward_roialign_readouts"
    steps = W.READOUT_STEPS if readouts else (T,)
    args = dict(ctx["args"], spike_rates=rates)
    kw, stat = _route_kw(variant, dev, "fc6", record)
    before = dict(ops.feature_calls)
    with W.poisoned_outputs(record):
        if readouts:
            cls, bbox, extras = ops.det_head_forward_roialign_readouts(flist, ctx["scales"], ctx["boxes4"], ctx["batch"], ctx["lvl"], steps=steps, **args)
        else:
            cls, bbox, extras = ops.det_head_forward_roialign(flist, ctx["scales"], ctx["boxes4"], ctx["batch"], ctx["lvl"], T=T, **args, **kw)
    if s["nhwc"]:
        assert ops.feature_calls["nhwc"] == before["nhwc"] + 1 and ops.feature_calls["no_typed_kernel"] == before["no_typed_kernel"]
    path = _lib.load().snn_debug_last_fc6_path()
    n6 = T if rates else T - 1
    res = dict(path=path, tensors=(cls, bbox, extras, stat))

    def source():
        res["p6"], res["p7"] = head_det_planes(dev, T, case["Hd"], s["R"])
        return W.snapshot(cls, bbox, extras, stat, res["p6"][:n6], res["p7"])

    def oracle(name=None):
        name = ctx["loaded"] if name is None else name
        pool, feats, boxes, shapes, e6, e7, counts_e, cls_e, bbox_e = ctx["host"][name]
        plan = _det_plan(s)
        assert path == plan, "%s: fc6 reported launch %d, this case is about %d" % (spec_id(s), path, plan)
        _check_det(s, case, "bf16x3", res["p6"], res["p7"], (cls, bbox), extras[:2], e6, e7, counts_e, cls_e, bbox_e, steps, rates)
        want = _stat_want(variant, True, lambda: _route_counts(("roi", s["feat"], _roi_draw(name)), lambda: FR.route_counts(FR.roi_pooled(feats, boxes, shapes), T)), _lib.FC6_ROUTE_DEFAULT_CROSSOVER)
        assert _stat_list(stat) == want, "route_stat %s, documented %s" % (_stat_list(stat), want)
        res["stat"] = _stat_list(stat)
    res["source"], res["oracle"] = source, oracle
    return res


# ---- post-processing ---------------------------------------------------------------------------------------------------------------------
def _close_scores(got, exp, what):
    got, exp = got.detach().cpu().double(), exp.double()
    assert got.shape == exp.shape, what
    if got.numel():
        assert float((got - exp).abs().max()) <= SCORE_ATOL, "%s: scores differ by %g" % (what, float((got - exp).abs().max()))


def _derived_only(name):
    raise AssertionError("input set %r is derived from the spec's own: its expectation is the eager call, there is no oracle for it" % name)


def prepare_nms(s, dev, inputs=None):
    """further input sets (graph capture): "reversed" = the same boxes with the score order reversed (another greedy order, another kept set);
    "one_box" = every box the same box of one category (one survivor)"""
    c = PG.nms_case(s["n"], 0.5, s["ncat"], s["layout"])
    names = _names(dict(s, inp="spec"), inputs)
    sets = {}
    for n in names:
        if n == "spec":
            sets[n] = [c["boxes"], c["scores"], c["idxs"]]
        elif n == "reversed":
            sets[n] = [c["boxes"], c["scores"].flip(0).contiguous(), c["idxs"]]
        elif n == "one_box":
            sets[n] = [c["boxes"][:1].expand_as(c["boxes"]).contiguous(), c["scores"], torch.zeros_like(c["idxs"])]
        else:
            raise KeyError(n)
    return dict(s=s, dev=dev, c=c, operands=[t.to(dev) for t in sets[names[0]]], sets=sets, loaded=names[0])


def call_nms(ctx, record=None):
    from oracle import torchvision_restated as TV
    from snn_automotive_object_detection_amd import ops
    s, c = ctx["s"], ctx["c"]
    b, sc, i = ctx["operands"]
    with W.poisoned_outputs(record):
        if s["entry"] == "batched_nms":
            kept = ops.batched_nms(b, sc, i, 0.5)
            order = mask = None
        else:
            order, mask = ops.nms_keep_mask(b, sc, i, 0.5)
            kept = None
    res = dict(tensors=(kept, order, mask))

    def source():
        res["kept"] = kept if kept is not None else order[mask]
        return W.snapshot(res["kept"])

    def oracle(name=None):
        name = ctx["loaded"] if name is None else name
        bb, ss, ii = ctx["sets"][name]
        assert torch.equal(res["kept"].cpu(), TV.batched_nms(bb, ss, ii, 0.5))
    res["source"], res["oracle"] = source, oracle
    return res


def _shrink_rows(de, rows):
    """box deltas whose rows `rows` decode to boxes far below min_size (log-size -20)"""
    de = de.clone()
    v = de[rows].view(len(rows), -1, 4)
    v[:, :, 2:] = -20.0
    de[rows] = v.view(len(rows), -1)
    return de


def prepare_rpn_proposals(s, dev, inputs=None):
    """further input sets (graph capture), derived from the spec's by shrinking candidate boxes below min_size so that the COUNTS change:
    "fewer" = image 0 as it is, image 1 left with the candidates of one position of the coarsest level, every later image with none;
    "none" = every box shrunk (all counts zero)"""
    from snn_automotive_object_detection_amd.stock.anchors import AnchorGenerator
    spec = PG.rpn_spec(s["spec"])
    lg, de, hw, strides = PG.rpn_device_inputs(spec, dev)
    ag = AnchorGenerator(spec["geo"]["sizes"], spec["geo"]["ratios"])
    names = _names(dict(s, inp="spec"), inputs)
    N = spec["N"]
    base = [t.cpu() for t in lg] + [t.cpu() for t in de]
    sets = {}
    for n in names:
        if n == "spec":
            sets[n] = base
            continue
        new = []
        for l, d in enumerate(base[len(lg):]):
            per = d.shape[0] // N
            if n == "none":
                rows = list(range(d.shape[0]))
            elif n == "fewer":
                rows = [r for r in range(per, d.shape[0]) if not (l == len(lg) - 1 and r == per)]
            else:
                raise KeyError(n)
            new.append(_shrink_rows(d, rows))
        sets[n] = base[:len(lg)] + new
    return dict(s=s, dev=dev, spec=spec, lg=lg, de=de, hw=hw, strides=strides, anchors=ag.cell_anchors, operands=list(lg) + list(de), sets=sets,
                loaded=names[0], keep=[ag])


def call_rpn_proposals(ctx, record=None):
    from snn_automotive_object_detection_amd import ops
    spec = ctx["spec"]
    with W.poisoned_outputs(record):
        boxes, scores, counts, pre_b, pre_p = ops.rpn_proposals(ctx["lg"], ctx["de"], ctx["hw"], ctx["strides"], ctx["anchors"], spec["image_sizes"], spec["pre"],
                                                                 spec["post"], spec["nms"], spec["score_thresh"], spec["min_size"])
    res = dict(tensors=(boxes, scores, counts, pre_b, pre_p), counts=counts)

    def source():
        return W.snapshot(boxes, scores, counts, pre_b, pre_p)       # (the rows behind the counts are rows of `boxes` / `scores`)

    def oracle(name=None):
        name = ctx["loaded"] if name is None else name
        if name != "spec":
            _derived_only(name)
        e_b, e_s, e_pre = spec["expected"]
        assert counts.cpu().tolist() == [int(b.shape[0]) for b in e_b]
        for i in range(spec["N"]):
            c = int(e_b[i].shape[0])
            assert torch.equal(boxes[i, :c].cpu(), e_b[i]), "image %d: proposals" % i
            _close_scores(scores[i, :c], e_s[i], "image %d" % i)
            assert not bool(boxes[i, c:].any()) and not bool(scores[i, c:].any()), "image %d: rows behind the count" % i
            assert torch.equal(pre_b[i].cpu(), e_pre[i]["proposals"]), "image %d: pre-NMS boxes" % i
            _close_scores(pre_p[i], e_pre[i]["objectness"], "image %d pre-NMS" % i)
    res["source"], res["oracle"] = source, oracle
    return res


def prepare_det_postprocess(s, dev, inputs=None):
    """further input sets (graph capture), derived from the spec's: "fewer" = the background logit of every row but the first two raised by 30
    (their foreground scores fall below the score threshold: fewer detections than detections_per_img); "none" = of every row; for the padded
    entry "counts_a" / "counts_b" / "counts_0" = the spec's rows under the device counts (70, 37, 0)[:N] / (0, 70, 5)[:N] / zeros"""
    spec = PG.det_spec(s["spec"])
    padded = s["entry"] == "det_postprocess_padded"
    names = _names(dict(s, inp="spec"), inputs)
    if padded:
        lg, rg, pr, cn, cap = PG.det_padded_inputs(spec, dev)
    else:
        lg, rg, pr, cn = spec["logits"].to(dev), spec["reg"].to(dev), torch.cat(spec["props"]).to(dev), None
    N = len(spec["rois"])
    base = [lg.cpu(), rg.cpu(), pr.cpu()] + ([cn.cpu()] if padded else [])
    sets = {}
    for n in names:
        new = [t.clone() for t in base]
        if n in ("fewer", "none"):
            new[0][(2 if n == "fewer" else 0):, 0] += 30.0
        elif n in ("counts_a", "counts_b", "counts_0"):
            assert padded
            new[3] = torch.tensor({"counts_a": (70, 37, 0), "counts_b": (0, 70, 5), "counts_0": (0, 0, 0)}[n][:N], dtype=base[3].dtype)
        elif n != "spec":
            raise KeyError(n)
        sets[n] = new
    return dict(s=s, dev=dev, spec=spec, padded=padded, operands=[lg, rg, pr] + ([cn] if padded else []), sets=sets, loaded=names[0])


def call_det_postprocess(ctx, record=None):
    from snn_automotive_object_detection_amd import ops
    spec, padded = ctx["spec"], ctx["padded"]
    K, rois, N = spec["K"], spec["rois"], len(spec["rois"])
    with W.poisoned_outputs(record):
        if padded:
            lg, rg, pr, cn = ctx["operands"]
            boxes, scores, labels, counts, all_s, all_b = ops.det_postprocess_padded(
                lg, rg, pr, cn, list(spec["image_shapes"]), PG.BOX_WEIGHTS, PG.DET_SCORE_THRESH, spec["nms"], spec["det"])
        else:
            lg, rg, pr = ctx["operands"]
            boxes, scores, labels, counts, all_s, all_b = ops.det_postprocess(
                lg, rg, pr, rois, list(spec["image_shapes"]), PG.BOX_WEIGHTS, PG.DET_SCORE_THRESH, spec["nms"], spec["det"])
    res = dict(tensors=(boxes, scores, labels, counts, all_s, all_b), counts=counts)

    def source():
        # (the compacted form leaves the rows behind the counts unwritten: they are NaN / 0x5a in every run, which the snapshot pins as well)
        return W.snapshot(boxes, scores, labels, counts, all_s, all_b)

    def oracle(name=None):
        name = ctx["loaded"] if name is None else name
        if name != "spec":
            _derived_only(name)
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
    res["source"], res["oracle"] = source, oracle
    return res


# ---- the three parts per entry ------------------------------------------------------------------------------------------------------------
_RPN, _DET, _ROI = (prepare_rpn, call_rpn), (prepare_det, call_det), (prepare_roi, call_roi)
_NMS, _DPP = (prepare_nms, call_nms), (prepare_det_postprocess, call_det_postprocess)
PARTS = {
    ("rpn_head_forward", "_WS"): _RPN, ("rpn_head_forward", "_WS_RATES"): _RPN,
    ("rpn_head_forward_readouts", "_WS"): _RPN, ("rpn_head_forward_readouts", "_WS_RATES"): _RPN,
    ("det_head_forward", "_WS"): _DET, ("det_head_forward_readouts", "_WS"): _DET,
    ("det_head_forward_roialign", "_WS"): _ROI, ("det_head_forward_roialign_readouts", "_WS"): _ROI,
    ("batched_nms", "_WS"): _NMS, ("nms_keep_mask", "_WS"): _NMS, ("rpn_proposals", "_WS"): (prepare_rpn_proposals, call_rpn_proposals),
    ("det_postprocess", "_WS"): _DPP, ("det_postprocess_padded", "_WS"): _DPP,
}


def prepare(s, dev, inputs=None):
    return PARTS[(s["entry"], s["ws"])][0](s, dev, inputs)


def call_entry(s, ctx, record=None):
    return PARTS[(s["entry"], s["ws"])][1](ctx, record)


def _runner(key):
    def run_one(s, dev, record=None):
        res = PARTS[key][1](PARTS[key][0](s, dev), record)
        res["snap"] = res["source"]()
        return res
    return run_one


BUILDERS = {key: _runner(key) for key in PARTS}
run_rpn, run_det, run_roi = BUILDERS[("rpn_head_forward", "_WS")], BUILDERS[("det_head_forward", "_WS")], BUILDERS[("det_head_forward_roialign", "_WS")]
run_nms, run_rpn_proposals = BUILDERS[("nms_keep_mask", "_WS")], BUILDERS[("rpn_proposals", "_WS")]
run_det_postprocess = BUILDERS[("det_postprocess", "_WS")]


def run(s, dev, record=None):
    return BUILDERS[(s["entry"], s["ws"])](s, dev, record)


def call(s, dev):
    """the spec as a call() -> snapshot for the runners of tests/_ws_state.py; the oracle comparison runs inside every call"""
    def go():
        r = run(s, dev)
        r["oracle"]()
        return r["snap"]
    return go
