"""The conv route of the RPN head on the GPU (include/snn_hip.h: snn_rpn_head_forward_routed).

Shapes: N = 2, A = 3, the pyramid of tests/_exact_grid.py ((13, 17), (6, 7), (2, 1)) - the smallest at which the sparse launch runs -, C = 64
(one word pair) and 128 (two, spike planes in blocks of four words), T = 5, 8, 16 (the edges of the sparse window, both FAT tile shapes
and the 8-wave one), precisions bf16x3 and bf16.

  1. the device count equals the numpy restatement of tests/_conv_route.py (periods from the oracle's encoder trains);
  2. `sparse` is snn_rpn_head_forward bit for bit;
  3. `dense` on the dyadic grids equals the oracle's planes with zero flips, and a process started with SNN_SPARSE=0 returns the same bits;
  4. `auto` at crossover 2 / -1 is `sparse` / `dense` bit for bit, and at the default crossover takes the dense side on the full-nibble case
     and the sparse side on a silent and on a randn map;
  5. configurations without a sparse plan and spike-rate mode: every route is today's call, route_stat as documented;
  6. through static.heads_padded, fp32 and fp16 NHWC features, without a host synchronisation; SNN_CONV_ROUTE sets the default;
  7. bad arguments return -1 and enqueue nothing."""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import _conv_route as R
from tests import _exact_grid as G
from tests._planes import CUR_TOL, li_constants, li_fp64
from tests._util import planes_to_dense

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CT = [(C, T) for C in (64, 128) for T in (5, 8, 16)]
PRECISIONS = ["bf16x3", "bf16"]


def _grid(precision):
    return "narrow" if precision == "bf16" else "wide"          # (the single bf16 plane carries the narrow grid exactly)


def _case(C, T, precision):
    return G.rpn_t_case(C, T, _grid(precision))


def _dev(feats, dev):
    return [f.to(dev) for f in feats]


# ---- 1. the count ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,T", CT)
def test_device_count_equals_the_restatement(gpu_device, C, T, precision):
    m = R.head_for(_case(C, T, precision), gpu_device, precision)
    inputs = [("silent", R.silent_maps(C, G.PYRAMID, 2)), ("full", R.full_nibble_maps(C, T, G.PYRAMID, 2, C + T)),
              ("mixed", R.mixed_maps(C, T, G.PYRAMID, 2, C + T))]
    seen = {}
    for name, feats in inputs:
        want = R.route_counts(feats, T)
        r = R.forward(m, _dev(feats, gpu_device), "auto")
        print("%s: device %s, restated %s" % (name, r["stat"], want))
        assert r["path"] == 2, "the gated pair did not run"
        assert tuple(r["stat"][:2]) == want and r["stat"][3] == 0
        seen[name] = want
    assert seen["silent"][0] == 0 and 0 < seen["mixed"][0] < seen["full"][0] <= seen["full"][1]


# ---- 2. sparse -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,T", CT)
def test_sparse_route_is_the_plain_forward(gpu_device, C, T, precision):
    case = _case(C, T, precision)
    m = R.head_for(case, gpu_device, precision)
    feats = _dev(case["feats"], gpu_device)
    plain = R.forward(m, feats, None)
    assert plain["path"] == 1 and plain["stat"] is None
    # through ops with the route spelled out: snn_rpn_head_forward_routed(SNN_ROUTE_SPARSE)
    from snn_automotive_object_detection_amd import _lib, ops
    from tests._planes import head_rpn_planes
    Cc, A, p, w_shared, w_heads = m._pass_args()
    stat = torch.full((4,), -7, dtype=torch.int32, device=gpu_device)
    out_l, out_b, rows, _ = ops.rpn_head_forward(feats, Cc, A, T, p, w_shared, w_heads, conv_route="sparse", route_stat=stat)
    assert _lib.load().snn_debug_last_conv_path() == 1
    assert torch.equal(head_rpn_planes(gpu_device, T, C), plain["planes"])
    assert stat.tolist() == [0, 0, 0, 0]
    pos = 0
    for l, n in enumerate(rows):
        N, H, W = case["N"], *case["shapes"][l]
        assert torch.equal(out_l[pos:pos + n].view(N, H, W, A).permute(0, 3, 1, 2), plain["out"][l])
        assert torch.equal(out_b[pos:pos + n].view(N, H, W, 4 * A).permute(0, 3, 1, 2), plain["out"][len(rows) + l])
        pos += n
    ops.rpn_head_forward(feats, Cc, A, T, p, w_shared, w_heads, conv_route="sparse")          # (route_stat is optional on this route)


# ---- 3. dense --------------------------------------------------------------------------------------------------------------------------
def _assert_oracle(case, r, precision, what):
    C, A, T, N = case["C"], case["A"], case["T"], case["N"]
    got = planes_to_dense(r["planes"], C)
    diff = got != case["spk"]
    assert not diff.any(), "%s: hidden planes differ from the oracle's at %s ... (%d in all)" % (what, np.argwhere(diff)[:4].tolist(), int(diff.sum()))
    w = torch.cat([case["w_cls"].flatten(1), case["w_bbox"].flatten(1)])
    if precision == "bf16":
        w = w.to(torch.bfloat16).float()
    a, b = li_constants(None)
    last, _ = li_fp64(case["spk"], w, a, b, case["li_order"])
    pos = 0
    L = len(case["shapes"])
    for l, (H, W) in enumerate(case["shapes"]):
        o = torch.cat([r["out"][l], r["out"][L + l]], dim=1).permute(0, 2, 3, 1).reshape(N * H * W, 5 * A).double().cpu().numpy()
        assert np.abs(o - last[T - 1, pos:pos + N * H * W]).max() <= CUR_TOL, what
        pos += N * H * W


def _dense_cases():
    out = [("C%d_T%d_%s" % (C, T, pr), C, T, pr) for pr in PRECISIONS for C, T in CT]
    return out + [("full_nibble", 256, 8, "bf16x3")]


def _dense_case(name, C, T, precision):
    return G.rpn_full_nibble_case() if name == "full_nibble" else _case(C, T, precision)


@pytest.mark.parametrize("name,C,T,precision", _dense_cases(), ids=[c[0] for c in _dense_cases()])
def test_dense_route_equals_the_oracle_with_zero_flips(gpu_device, name, C, T, precision):
    case = _dense_case(name, C, T, precision)
    m = R.head_for(case, gpu_device, precision)
    r = R.forward(m, _dev(case["feats"], gpu_device), "dense")
    assert r["path"] == 0 and r["stat"] == [0, 0, 1, 0]
    _assert_oracle(case, r, precision, "dense")
    assert case["spk"].any()


CHILD_CASES = [("C64_T8_bf16x3", 64, 8, "bf16x3"), ("C128_T16_bf16", 128, 16, "bf16"), ("C128_T5_bf16x3", 128, 5, "bf16x3"),
               ("full_nibble", 256, 8, "bf16x3")]


def test_dense_route_equals_a_process_started_with_SNN_SPARSE_0(gpu_device):
    env = dict(os.environ, SNN_SPARSE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("SNN_CONV_ROUTE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conv_route_child.py"), "plain", json.dumps(CHILD_CASES)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    for name, C, T, precision in CHILD_CASES:
        case = _dense_case(name, C, T, precision)
        m = R.head_for(case, gpu_device, precision)
        mine = R.forward(m, _dev(case["feats"], gpu_device), "dense")
        assert child[name]["path"] == 0, "the child did not run the dense plan"
        assert child[name]["digest"] == R.digest(mine), name


# ---- 4. auto ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,T", CT)
def test_auto_is_one_side_or_the_other_bit_for_bit(gpu_device, C, T, precision):
    case = _case(C, T, precision)
    m = R.head_for(case, gpu_device, precision)
    feats = _dev(case["feats"], gpu_device)
    sparse, dense = R.forward(m, feats, "sparse"), R.forward(m, feats, "dense")
    never, always = R.forward(m, feats, "auto", 2.0), R.forward(m, feats, "auto", -1.0)
    assert never["path"] == always["path"] == 2
    assert never["stat"][2] == 0 and R.same_bits(never, sparse)
    assert always["stat"][2] == 1 and R.same_bits(always, dense)
    assert never["stat"][:2] == always["stat"][:2] == list(R.route_counts(case["feats"], T))
    _assert_oracle(case, never, precision, "auto / sparse side")
    _assert_oracle(case, always, precision, "auto / dense side")


def test_auto_full_nibble_case_both_sides(gpu_device):
    from snn_automotive_object_detection_amd import _lib
    case = G.rpn_full_nibble_case()
    m = R.head_for(case, gpu_device, "bf16x3")
    feats = _dev(case["feats"], gpu_device)
    sparse, dense = R.forward(m, feats, "sparse"), R.forward(m, feats, "dense")
    never, always, default = R.forward(m, feats, "auto", 2.0), R.forward(m, feats, "auto", -1.0), R.forward(m, feats, "auto")
    assert R.same_bits(never, sparse) and never["stat"][2] == 0
    assert R.same_bits(always, dense) and always["stat"][2] == 1
    hits, blocks = default["stat"][:2]
    print("full-nibble case: %d hits of %d blocks" % (hits, blocks))
    assert (hits, blocks) == R.route_counts(case["feats"], 8)
    assert np.float32(hits) > np.float32(_lib.ROUTE_DEFAULT_CROSSOVER) * np.float32(blocks)
    assert default["stat"][2] == 1 and R.same_bits(default, dense)
    for r in (sparse, dense):
        _assert_oracle(case, r, "bf16x3", "full nibble")


@pytest.mark.parametrize("C,T", [(64, 8), (128, 16)])
def test_default_crossover_takes_the_sparse_side_on_sparse_inputs(gpu_device, C, T):
    from snn_automotive_object_detection_amd import _lib
    case = _case(C, T, "bf16x3")
    m = R.head_for(case, gpu_device, "bf16x3")
    for feats in (case["feats"], R.silent_maps(C, G.PYRAMID, 2)):               # N(0, 1.7) maps; silent maps
        feats = _dev(feats, gpu_device)
        r = R.forward(m, feats, "auto")
        hits, blocks, route, _ = r["stat"]
        print("hits %d of %d blocks" % (hits, blocks))
        assert (hits, blocks) == R.route_counts([f.cpu() for f in feats], T) and route == 0
        assert not np.float32(hits) > np.float32(_lib.ROUTE_DEFAULT_CROSSOVER) * np.float32(blocks)
        assert R.same_bits(r, R.forward(m, feats, "sparse"))


# ---- 5. configurations without a sparse plan, spike-rate mode --------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,precision", [(64, 8, "f32"), (64, 4, "bf16x3"), (192, 8, "bf16x3")], ids=["f32", "T4", "C192"])
def test_every_route_is_todays_call_where_the_plan_is_dense(gpu_device, C, T, precision):
    case = G.rpn_t_case(C, T)
    m = R.head_for(case, gpu_device, precision)
    feats = _dev(case["feats"], gpu_device)
    plain = R.forward(m, feats, None)
    assert plain["path"] == 0 or precision == "f32"
    for route in ("sparse", "dense", "auto"):
        r = R.forward(m, feats, route)
        assert R.same_bits(r, plain), route
        assert r["stat"] == [0, 0, 1, 0], route


def test_one_hundred_channels_pad_to_two_word_pairs_and_do_have_a_sparse_plan(gpu_device):
    """C = 100 pads to 128 channels = two word pairs: today's plan IS the sparse one (tests/test_gpu_exact_grid.py pins that), so the routes are
    real there.  On the dyadic grid both sides give the oracle's planes, hence all routes equal today's call bit for bit all the same"""
    case = G.rpn_t_case(100, 8)
    m = R.head_for(case, gpu_device, "bf16x3")
    feats = _dev(case["feats"], gpu_device)
    plain = R.forward(m, feats, None)
    assert plain["path"] == 1
    want = {"sparse": (1, [0, 0, 0, 0]), "dense": (0, [0, 0, 1, 0]), "auto": (2, list(R.route_counts(case["feats"], 8)) + [0, 0])}
    for route, (path, stat) in want.items():
        r = R.forward(m, feats, route)
        assert R.same_bits(r, plain) and r["path"] == path and r["stat"] == stat, route
    _assert_oracle(case, plain, "bf16x3", "C = 100")


@pytest.mark.parametrize("C,T", [(64, 8), (128, 16)])
def test_spike_rate_mode_runs_todays_plan_on_every_route(gpu_device, C, T):
    case = _case(C, T, "bf16x3")
    m = R.head_for(case, gpu_device, "bf16x3")
    m.spike_rates = True
    feats = _dev(case["feats"], gpu_device)
    plain = R.forward(m, feats, None)
    counts = m.last_spike_counts.clone()
    assert plain["path"] == 1 and len(plain["out"]) > 2 * len(feats)
    for route in ("sparse", "dense", "auto"):
        r = R.forward(m, feats, route, -1.0)
        assert r["path"] == 1 and R.same_bits(r, plain) and torch.equal(m.last_spike_counts, counts), route
        assert r["stat"] == [0, 0, 0, 0], route
    assert np.array_equal(counts[:, :case["N"]].cpu().numpy(), case["counts"])


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
    from snn_automotive_object_detection_amd import _lib, static
    from snn_automotive_object_detection_amd.stock.anchors import ImageList
    images = ImageList(torch.empty((2, 0, 128, 256)), [(128, 256)] * 2)
    feats = _pyramid(gpu_device, dtype, nhwc)
    head = detector.rpn.head
    try:
        head.conv_route = "sparse"
        want = static.heads_padded(detector, feats, images)
        assert _lib.load().snn_debug_last_conv_path() == 1
        head.conv_route = "auto"
        static.heads_padded(detector, feats, images)             # (first call: sizes the workspaces)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = static.heads_padded(detector, feats, images)
            stat = head.route_stat
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert _lib.load().snn_debug_last_conv_path() == 2
    finally:
        head.conv_route = None
    hits, blocks, route, _ = stat.tolist()
    print("randn pyramid: %d hits of %d blocks" % (hits, blocks))
    assert blocks > 0 and route == 0
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert int(want["roi_counts"].sum()) == 80 and float(want["objectness"].abs().max()) > 0


def test_SNN_CONV_ROUTE_sets_the_default_route(gpu_device):
    env = dict(os.environ, SNN_CONV_ROUTE="auto", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("SNN_SPARSE", None)
    cases = [CHILD_CASES[0]]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conv_route_child.py"), "default", json.dumps(cases)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])[cases[0][0]]
    assert child["path"] == 2 and child["stat"] is not None and child["stat"][1] > 0 and child["stat"][2] == 0


# ---- 7. bad arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_minus_one_and_enqueue_nothing(gpu_device):
    from snn_automotive_object_detection_amd import _lib, ops
    lib = _lib.load()
    case = _case(64, 8, "bf16x3")
    m = R.head_for(case, gpu_device, "bf16x3")
    feats = _dev(case["feats"], gpu_device)
    C, A, p, w_shared, w_heads = m._pass_args()
    need = lib.snn_rpn_head_workspace_bytes_routed(ops._rpn_table(feats), len(feats), C, A, 8, p.precision, 2)
    assert need == lib.snn_rpn_head_workspace_bytes_routed(ops._rpn_table(feats), len(feats), C, A, 8, p.precision, 0) > 0
    assert lib.snn_rpn_head_workspace_bytes_routed(ops._rpn_table(feats), len(feats), C, A, 8, p.precision, 5) == 0
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device=gpu_device)
    stat = torch.full((4,), -7, dtype=torch.int32, device=gpu_device)
    for what, kw in [("route", dict(route=3, stat=stat)), ("route", dict(route=-1, stat=stat)), ("route_stat", dict(route=2, stat=None)),
                     ("workspace", dict(route=2, stat=stat, ws_bytes=need - 1)), ("workspace", dict(route=1, stat=stat, ws_bytes=need - 1))]:
        rc, out_l, out_b = R.raw_call(lib, feats, C, A, 8, p, w_shared, w_heads, kw["route"], 0.5, kw["stat"], ws, kw.get("ws_bytes"))
        assert rc == -1 and what.encode() in lib.snn_last_error(), (what, rc, lib.snn_last_error())
        torch.cuda.synchronize()
        assert stat.tolist() == [-7] * 4 and bool((ws == 0x5a).all()) and not out_l.any() and not out_b.any(), what
    rc, out_l, out_b = R.raw_call(lib, feats, C, A, 8, p, w_shared, w_heads, 2, 0.5, stat, ws)
    assert rc == 0 and stat.tolist()[1] > 0 and out_l.any()
