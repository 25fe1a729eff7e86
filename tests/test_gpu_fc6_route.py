"""The fc6 route of the detector head on the GPU (include/snn_hip.h: snn_det_head_forward_routed / _roialign_routed).

Shapes: tests/_exact_grid.py's detector shapes, C = 64, Hd = 128, K = 9 - the smallest at which fc6's sparse launch runs -, R = 17, 29, 33
(a one-row last block, a 13-row one, a full block and a one-row one), T = 6 and 12 (the window of the encoder fold), 16 (beyond it) and 24
(the general LIF epilogue) - all four have a sparse plan -, precisions bf16x3 and bf16; the RoIAlign-fed entry on a two-level pyramid at
T = 12 and 16 with fp32 NCHW and fp16 NHWC maps.

  1. the device count equals the numpy restatement of tests/_fc6_route.py (periods from the oracle's encoder trains);
  2. `sparse` is the plain forward bit for bit;
  3. `dense` on the dyadic grids equals the oracle's planes with zero flips, and a process started with SNN_SPARSE=0 returns the same bits;
  4. `auto` at crossover 2 / -1 is `sparse` / `dense` bit for bit, and at the header's crossover takes the route hits > d * blocks names;
  5. configurations without a sparse plan and spike-rate mode: every route is the plain call, route_stat as documented;
  6. through static.heads_padded without a host synchronisation; SNN_FC6_ROUTE sets the default;
  7. bad arguments return -1 and enqueue nothing."""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _exact_grid as G
from tests import _fc6_route as R
from tests._planes import CUR_TOL, li_constants, li_fp64
from tests._util import planes_to_dense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = [(Rn, T) for Rn in (17, 29, 33) for T in (6, 12, 16, 24)]
PRECISIONS = ["bf16x3", "bf16"]


def _lib():
    from snn_automotive_object_detection_amd import _lib as L
    return L


def _case(Rn, T, precision, full_nibble=False):
    return G.det_case(Rn, 64, 128, 9, T, 600 + Rn + T, "narrow" if precision == "bf16" else "wide", full_nibble=full_nibble)


# ---- 1. the count ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("Rn,T", RT)
def test_device_count_equals_the_restatement(gpu_device, Rn, T, precision):
    case = _case(Rn, T, precision)
    d = R.head_for(case, gpu_device, precision)
    plain = R.forward(d, case["x"].to(gpu_device), None)
    assert plain["path"] == 1 and plain["stat"] is None, "T = %d has a sparse plan: the plain entry must run it" % T
    full = G.full_nibble_values((Rn, 64, 7, 7), T, torch.Generator().manual_seed(Rn + T))
    seen = {}
    for name, x in [("silent", R.silent_like(full)), ("full", full), ("mixed", R.mixed_like(full))]:
        want = R.route_counts(x, T)
        r = R.forward(d, x.to(gpu_device), "auto", 0.5)
        print("%s: device %s, restated %s" % (name, r["stat"], want))
        assert r["path"] == 2, "the gated pair did not run"
        assert tuple(r["stat"][:2]) == want and r["stat"][3] == 0
        assert r["stat"][2] == R.route_of(*want, 0.5)
        seen[name] = want
    # (one full-nibble row already hits nearly every word pair of its block: the mixed rows 15 .. 17 reach blocks 0 and 1, all there are below R = 33)
    assert seen["silent"][0] == 0 and 0 < seen["mixed"][0] <= seen["full"][0] <= seen["full"][1]
    assert seen["mixed"][0] < seen["full"][0] or Rn <= 32


# ---- 2. sparse -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("Rn,T", RT)
def test_sparse_route_is_the_plain_forward(gpu_device, Rn, T, precision):
    from snn_automotive_object_detection_amd import ops
    from tests._planes import head_det_planes
    case = _case(Rn, T, precision)
    d = R.head_for(case, gpu_device, precision)
    x = case["x"].to(gpu_device)
    plain = R.forward(d, x, None)
    assert plain["path"] == 1 and plain["stat"] is None
    # through ops with the route spelled out: snn_det_head_forward_routed(SNN_ROUTE_SPARSE)
    stat = torch.full((4,), -7, dtype=torch.int32, device=gpu_device)
    xr = x.flatten(1)
    cls, bbox, _ = ops.det_head_forward(xr, T=T, **d._pass_args(xr.shape[1], "rows"), fc6_route="sparse", route_stat=stat)
    assert _lib().load().snn_debug_last_fc6_path() == 1
    p6, p7 = head_det_planes(gpu_device, T, 128, Rn)
    assert torch.equal(p6[:T - 1], plain["p6"]) and torch.equal(p7, plain["p7"])
    assert torch.equal(cls, plain["out"][0]) and torch.equal(bbox, plain["out"][1])
    assert stat.tolist() == [0, 0, 0, 0]
    ops.det_head_forward(xr, T=T, **d._pass_args(xr.shape[1], "rows"), fc6_route="sparse")         # (route_stat is optional on this route)


# ---- 3. dense --------------------------------------------------------------------------------------------------------------------------
def _assert_oracle(case, r, precision, what):
    T, Hd = case["T"], case["Hd"]
    e6, e7 = case["trace"]["spk6"].numpy(), case["trace"]["spk7"].numpy()
    g6, g7 = planes_to_dense(r["p6"], Hd), planes_to_dense(r["p7"], Hd)
    d6, d7 = g6 != e6[:T - 1], g7 != e7
    assert not d6.any(), "%s: lif6 planes differ at (step, RoI, unit) %s ... (%d in all)" % (what, np.argwhere(d6)[:4].tolist(), int(d6.sum()))
    assert not d7.any(), "%s: lif7 planes differ at (step, RoI, unit) %s ... (%d in all)" % (what, np.argwhere(d7)[:4].tolist(), int(d7.sum()))
    w = torch.cat([case["w_cls"].flatten(1), case["w_bbox"].flatten(1)])
    if precision == "bf16":
        w = w.to(torch.bfloat16).float()
    a, b = li_constants(None)
    last, _ = li_fp64(e7, w, a, b, case["li_order"])
    o = torch.cat([r["out"][0], r["out"][1]], dim=1).double().cpu().numpy()
    err = np.abs(o - last[T - 1]).max()
    print("%s: |out - fp64| %.3g" % (what, err))
    assert err <= CUR_TOL, what


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("Rn,T", RT)
def test_dense_route_equals_the_oracle_with_zero_flips(gpu_device, Rn, T, precision):
    case = _case(Rn, T, precision)
    d = R.head_for(case, gpu_device, precision)
    r = R.forward(d, case["x"].to(gpu_device), "dense")
    assert r["path"] == 0 and r["stat"] == [0, 0, 1, 0]
    _assert_oracle(case, r, precision, "dense")
    assert case["trace"]["spk6"].any() and case["trace"]["spk7"].any()


CHILD_CASES = [("R29_T12_bf16x3", 29, 12, "bf16x3"), ("R17_T6_bf16", 17, 6, "bf16"), ("R33_T16_bf16x3", 33, 16, "bf16x3"),
               ("R29_T24_bf16", 29, 24, "bf16"), ("full_R29_T12", 29, 12, "bf16x3")]


def _child(env_extra, mode, cases):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("SNN_SPARSE", "SNN_FC6_ROUTE", "SNN_CONV_ROUTE"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fc6_route.py"), mode, json.dumps(cases)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dense_route_equals_a_process_started_with_SNN_SPARSE_0(gpu_device):
    child = _child({"SNN_SPARSE": "0"}, "plain", CHILD_CASES)
    for name, Rn, T, precision in CHILD_CASES:
        case = _case(Rn, T, precision, full_nibble=name.startswith("full"))
        d = R.head_for(case, gpu_device, precision)
        mine = R.forward(d, case["x"].to(gpu_device), "dense")
        assert child[name]["path"] == 0, "the child did not run the dense plan"
        assert mine["path"] == 0 and child[name]["digest"] == R.digest(mine), name


# ---- 4. auto ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("Rn,T", RT)
def test_auto_is_one_side_or_the_other_bit_for_bit(gpu_device, Rn, T, precision):
    case = _case(Rn, T, precision)
    d = R.head_for(case, gpu_device, precision)
    x = case["x"].to(gpu_device)
    sparse, dense = R.forward(d, x, "sparse"), R.forward(d, x, "dense")
    never, always = R.forward(d, x, "auto", 2.0), R.forward(d, x, "auto", -1.0)
    assert sparse["path"] == 1 and dense["path"] == 0 and never["path"] == always["path"] == 2
    assert never["stat"][2] == 0 and R.same_bits(never, sparse)
    assert always["stat"][2] == 1 and R.same_bits(always, dense)
    assert never["stat"][:2] == always["stat"][:2] == list(R.route_counts(case["x"], T))
    _assert_oracle(case, never, precision, "auto / sparse side")
    _assert_oracle(case, always, precision, "auto / dense side")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_header_crossover_takes_the_route_the_restatement_names(gpu_device, precision):
    """T = 8, the inputs of tests/_fc6_route.decided_inputs: full-nibble and N(0, 1) features take the dense side, silent and N(0, 4) features
    the sparse side; tests/test_fc6_route_cpu.py checks that each lies at least 0.05 from the header's crossover"""
    dflt = _lib().FC6_ROUTE_DEFAULT_CROSSOVER
    case = G.det_case(29, 64, 128, 9, 8, 208, "narrow" if precision == "bf16" else "wide")
    d = R.head_for(case, gpu_device, precision)
    for name, x, expected in R.decided_inputs():
        want = R.route_counts(x, 8)
        xg = x.to(gpu_device)
        r = R.forward(d, xg, "auto")                                   # (fc6_crossover None: the header's)
        print("%s: %s, restated %s, crossover %g" % (name, r["stat"], want, dflt))
        assert r["path"] == 2 and tuple(r["stat"][:2]) == want
        assert r["stat"][2] == R.route_of(*want, dflt)
        assert dflt >= 1.0 or r["stat"][2] == expected, name
        assert R.same_bits(r, R.forward(d, xg, "dense" if r["stat"][2] else "sparse"))


# ---- the RoIAlign-fed entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,nhwc", [(torch.float32, False), (torch.float16, True)], ids=["fp32", "fp16_nhwc"])
@pytest.mark.parametrize("T", [12, 16])
def test_roialign_fed_entry(gpu_device, T, dtype, nhwc):
    from snn_automotive_object_detection_amd import ops
    case = _case(33, T, "bf16x3")                                       # (its weights; the features come from the pyramid)
    d = R.head_for(case, gpu_device, "bf16x3")
    pool, feats, boxes, shapes = R.roi_setup(64, 33, 40 + T)
    feats = {k: v.to(dtype) for k, v in feats.items()}
    want = R.route_counts(R.roi_pooled(feats, boxes, shapes), T)
    dev_feats = {k: v.to(gpu_device) for k, v in feats.items()}
    if nhwc:
        dev_feats = {k: v.contiguous(memory_format=torch.channels_last) for k, v in dev_feats.items()}
    roi = pool.assign(dev_feats, [b.to(gpu_device) for b in boxes], shapes)
    assert set(roi[3].tolist()) == {0, 1} and int(roi[2].shape[0]) == 33
    before = dict(ops.feature_calls)
    plain = R.forward(d, None, None, roi=roi)
    assert plain["path"] == 1
    sparse, dense = R.forward(d, None, "sparse", roi=roi), R.forward(d, None, "dense", roi=roi)
    never, always = R.forward(d, None, "auto", 2.0, roi=roi), R.forward(d, None, "auto", -1.0, roi=roi)
    if nhwc:
        assert ops.feature_calls["nhwc"] == before["nhwc"] + 6 and ops.feature_calls["no_typed_kernel"] == before["no_typed_kernel"]
    print("device %s, restated %s" % (never["stat"], want))
    assert sparse["path"] == 1 and sparse["stat"] == [0, 0, 0, 0] and R.same_bits(sparse, plain)
    assert dense["path"] == 0 and dense["stat"] == [0, 0, 1, 0]
    assert never["path"] == always["path"] == 2
    assert never["stat"] == list(want) + [0, 0] and always["stat"] == list(want) + [1, 0] and want[0] > 0
    assert R.same_bits(never, sparse) and R.same_bits(always, dense)
    assert float(plain["out"][0].abs().max()) > 0 and bool(plain["p6"].any())


# ---- 5. configurations without a sparse plan, spike-rate mode --------------------------------------------------------------------------
def _every_route_is_plain(d, x, want_stat):
    plain = R.forward(d, x, None)
    for route in ("sparse", "dense", "auto"):
        r = R.forward(d, x, route, -1.0)
        assert r["path"] == plain["path"] and R.same_bits(r, plain), route
        assert r["stat"] == want_stat, (route, r["stat"])
    return plain


@pytest.mark.parametrize("name", ["f32", "mxfp6", "C32"])
def test_every_route_is_the_plain_call_where_the_plan_is_dense(gpu_device, name):
    case, precision = {"f32": (G.det_t_case(12), "f32"), "mxfp6": (G.det_mx_case(), "mxfp6"), "C32": (G.det_r_case(17, 32), "bf16x3")}[name]
    d = R.head_for(case, gpu_device, precision)
    plain = _every_route_is_plain(d, case["x"].to(gpu_device), [0, 0, 1, 0])
    assert d._resolve_precision() == precision
    assert plain["path"] == 0 or name != "C32"                         # (only the fused bf16x3 layers report their fc6 launch)


def test_flatten_order_weights_decide_nothing(gpu_device, monkeypatch):
    """w6_inner != 49 (SNN_FC6_PERM=0: fc6 packed in the reference's order): `auto` and `sparse` run the plain plan, `dense` the dense launch;
    route_stat[2] names the launch that ran, nothing is counted"""
    monkeypatch.setenv("SNN_FC6_PERM", "0")
    case = G.det_t_case(12)
    d = R.head_for(case, gpu_device, "bf16x3")
    assert d.fc6_inner() == 0
    x = case["x"].to(gpu_device)
    plain = R.forward(d, x, None)
    print("flatten order: the plain entry's fc6 path is %d" % plain["path"])
    for route in ("sparse", "auto"):
        r = R.forward(d, x, route, -1.0)
        assert r["path"] == plain["path"] and R.same_bits(r, plain) and r["stat"] == [0, 0, 1 - plain["path"], 0], (route, r["stat"])
    r = R.forward(d, x, "dense")
    assert r["path"] == 0 and r["stat"] == [0, 0, 1, 0]
    _assert_oracle(case, r, "bf16x3", "flatten order, dense")


@pytest.mark.parametrize("Rn,T", [(17, 6), (33, 16)])
def test_spike_rate_mode_runs_the_plain_plan_on_every_route(gpu_device, Rn, T):
    case = _case(Rn, T, "bf16x3")
    d = R.head_for(case, gpu_device, "bf16x3")
    d.spike_rates = True
    x = case["x"].to(gpu_device)
    plain = R.forward(d, x, None)
    counts = [c.clone() for c in d.last_spike_counts]
    assert plain["path"] == 1 and len(plain["out"]) == 4
    for route in ("sparse", "dense", "auto"):
        r = R.forward(d, x, route, -1.0)
        assert r["path"] == 1 and R.same_bits(r, plain) and all(torch.equal(a, b) for a, b in zip(d.last_spike_counts, counts)), route
        assert r["stat"] == [0, 0, 0, 0], route
    assert np.array_equal(counts[0].cpu().numpy().astype(np.int64), case["counts"][0])


# ---- 6. module level -------------------------------------------------------------------------------------------------------------------
LEVELS = [(32, 64), (16, 32), (8, 16), (4, 8), (2, 4)]
NAMES = ["0", "1", "2", "3", "pool"]


@pytest.fixture(scope="module")
def detector(gpu_device):
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(1234)
    model = S.create_model("cityscapes", 9, True, True, 0, False, False, num_steps_rpn=8, num_steps_detector=12).eval()
    model.rpn.to(gpu_device)
    model.roi_heads.to(gpu_device)
    with torch.no_grad():
        model.rpn.head.shared_conv.weight.mul_(5.0)
    model.roi_heads.score_thresh = 0.05
    model.rpn._post_nms_top_n = dict(training=40, testing=40)
    return model


def _pyramid(dev, dtype, nhwc):
    g = torch.Generator().manual_seed(21)
    out = OrderedDict()
    for n, (h, w) in zip(NAMES, LEVELS):
        f = (2 * torch.randn((2, 256, h, w), generator=g)).to(dev).to(dtype)
        out[n] = f.contiguous(memory_format=torch.channels_last) if nhwc else f
    return out


@pytest.mark.parametrize("dtype,nhwc", [(torch.float32, False), (torch.float16, True)], ids=["fp32", "fp16_nhwc"])
def test_heads_padded_auto_equals_sparse_without_a_host_synchronisation(gpu_device, detector, dtype, nhwc):
    from snn_automotive_object_detection_amd import static
    from snn_automotive_object_detection_amd.stock.anchors import ImageList
    images = ImageList(torch.empty((2, 0, 128, 256)), [(128, 256)] * 2)
    feats = _pyramid(gpu_device, dtype, nhwc)
    head = detector.roi_heads.box_head_and_predictor
    try:
        head.fc6_route = "sparse"
        want = static.heads_padded(detector, feats, images)
        assert _lib().load().snn_debug_last_fc6_path() == 1 and head.route_stat is None
        head.fc6_route, head.fc6_crossover = "auto", 2.0
        static.heads_padded(detector, feats, images)             # (first call: sizes the workspaces)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = static.heads_padded(detector, feats, images)
            stat = head.route_stat
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert _lib().load().snn_debug_last_fc6_path() == 2
    finally:
        head.fc6_route, head.fc6_crossover = None, None
    hits, blocks, route, _ = stat.tolist()
    print("randn pyramid: %d hits of %d blocks" % (hits, blocks))
    assert blocks == 5 * 196 * 8 and hits > 0 and route == 0          # 2 x 40 padded rows, 256 x 49 / 64 word pairs, planes e_3 .. e_10
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert int(want["roi_counts"].sum()) == 80 and float(want["class_logits"].abs().max()) > 0


def test_SNN_FC6_ROUTE_sets_the_default_route(gpu_device):
    cases = [CHILD_CASES[0]]
    child = _child({"SNN_FC6_ROUTE": "auto"}, "default", cases)[cases[0][0]]
    name, Rn, T, precision = cases[0]
    want = R.route_counts(_case(Rn, T, precision)["x"], T)
    assert child["path"] == 2 and child["stat"] == list(want) + [R.route_of(*want, _lib().FC6_ROUTE_DEFAULT_CROSSOVER), 0]


# ---- 7. bad arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_minus_one_and_enqueue_nothing(gpu_device):
    lib = _lib().load()
    case = _case(29, 12, "bf16x3")
    d = R.head_for(case, gpu_device, "bf16x3")
    x = case["x"].to(gpu_device)
    shape = (29, 64 * 49, 128, 9, 36, 12)
    need = lib.snn_det_head_workspace_bytes_routed(*shape, 1, 2)
    assert need == lib.snn_det_head_workspace_bytes_routed(*shape, 1, 0) >= lib.snn_det_head_workspace_bytes(*shape, 1) > 0
    assert lib.snn_det_head_workspace_bytes_routed(*shape, 1, 5) == 0
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device=gpu_device)
    stat = torch.full((4,), -7, dtype=torch.int32, device=gpu_device)
    for what, kw in [("route", dict(route=3, stat=stat)), ("route", dict(route=-1, stat=stat)), ("route_stat", dict(route=2, stat=None)),
                     ("workspace", dict(route=2, stat=stat, ws_bytes=need - 1)), ("workspace", dict(route=1, stat=stat, ws_bytes=need - 1))]:
        rc, out_c, out_b = R.raw_call(lib, d, x, kw["route"], 0.5, kw["stat"], ws, kw.get("ws_bytes"))
        assert rc == -1 and what.encode() in lib.snn_last_error(), (what, rc, lib.snn_last_error())
        torch.cuda.synchronize()
        assert stat.tolist() == [-7] * 4 and bool((ws == 0x5a).all()) and not out_c.any() and not out_b.any(), what
    rc, out_c, out_b = R.raw_call(lib, d, x, 2, 0.5, stat, ws)
    assert rc == 0 and stat.tolist()[1] > 0 and out_c.any()
    from snn_automotive_object_detection_amd import ops
    xr = x.flatten(1)
    for bad in (dict(fc6_route="fast"), dict(fc6_route="auto", route_stat=torch.zeros(4, dtype=torch.int32)),
                dict(fc6_route="auto", route_stat=torch.zeros(4, dtype=torch.int64, device=gpu_device))):
        with pytest.raises(_lib().SnnHipError):
            ops.det_head_forward(xr, T=12, **d._pass_args(xr.shape[1], "rows"), **bad)
