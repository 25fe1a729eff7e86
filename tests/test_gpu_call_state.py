"""A head pass leaves nothing behind for the next call of the thread: not its route, not a half-made plan, not its weight-plane count.

One thread, one library handle, the smallest shapes of the route tests that have a sparse plan: the RPN head at C = 64, T = 5 on the
pyramid of tests/_exact_grid.py (tests/test_gpu_conv_route.py), the detector head at R = 17, C = 64, Hd = 128, K = 9, T = 6
(tests/test_gpu_fc6_route.py), row-fed and RoIAlign-fed.  Every output goes into a NaN-filled buffer (tests/_ws_state.poisoned_outputs) and
is compared with torch.equal, the hidden planes with it.

  1. plain call (path 1) -> `dense` call (path 0) -> plain call: path 1 and the first call's bits;
  2. an `auto` call that returns behind the point where its plan was made, without finishing -> plain call: path 1, the recorded bits ->
     `auto` at crossover 2: the gated pair (path 2), route_stat[2] == 0, the recorded bits.  Such a return exists on the RoIAlign feed
     alone - rois = NULL: fp32 NCHW maps are refused by the encoder (-1), channels-last maps answered with SNN_STATUS_NO_TYPED_KERNEL; behind
     the plan of the RPN head and of the row-fed detector only a failed launch returns, which no test may provoke;
  3. a head pass at precision bf16 (one weight plane) -> the stage-level fc + LIF on three-plane weights returns what it returned before
     that pass -> a bf16x3 head pass: its earlier bits.

Every call is well-formed or refused on the host."""
import ctypes as Ct
import functools

import pytest
import torch

from tests import _conv_route as CR
from tests import _exact_grid as G
from tests import _fc6_route as FR
from tests._ws_state import poisoned_outputs, still_poisoned

pytestmark = pytest.mark.gpu
RPN_C, RPN_T = 64, 5
DET_R, DET_T = 17, 6


def _lib():
    from snn_automotive_object_detection_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def _rpn_case():
    return G.rpn_t_case(RPN_C, RPN_T, "wide")


@functools.lru_cache(maxsize=None)
def _det_case():
    return G.det_case(DET_R, 64, 128, 9, DET_T, 600 + DET_R + DET_T, "wide")


def _stat(dev):
    return torch.full((4,), -7, dtype=torch.int32, device=dev)


def _rpn_call(m, feats, route=None, crossover=None):
    """one RPN head pass through ops -> (outputs + hidden planes, the conv's reported launch, route_stat)"""
    from snn_automotive_object_detection_amd import ops
    from tests._planes import head_rpn_planes
    C_, A, p, w_shared, w_heads = m._pass_args()
    stat = None if route is None else _stat(feats[0].device)
    with poisoned_outputs():
        out_l, out_b, _, _ = ops.rpn_head_forward(feats, C_, A, RPN_T, p, w_shared, w_heads, conv_route=route, conv_crossover=crossover,
                                                  route_stat=stat)
    path = _lib().load().snn_debug_last_conv_path()
    return [out_l, out_b, head_rpn_planes(feats[0].device, RPN_T, C_).clone()], path, None if stat is None else stat.tolist()


def _det_call(d, x, roi, route=None, crossover=None):
    """one detector head pass through ops, fed by rows `x` or by roi = (maps, scales, rois [R, 5], levels) -> as _rpn_call, fc6's launch"""
    from snn_automotive_object_detection_amd import ops
    from tests._planes import head_det_planes
    dev = x.device if roi is None else roi[2].device
    stat = None if route is None else _stat(dev)
    kw = dict(T=DET_T, fc6_route=route, fc6_crossover=crossover, route_stat=stat)
    with poisoned_outputs():
        if roi is None:
            xr = x.flatten(1)
            cls, bbox, _ = ops.det_head_forward(xr, **kw, **d._pass_args(xr.shape[1], "rows"))
        else:
            flist, scales, rois, lvl = roi
            cls, bbox, _ = ops.det_head_forward_roialign(flist, scales, rois[:, 1:5], rois[:, 0], lvl, **kw,
                                                         **d._pass_args(flist[0].shape[1] * 49, "maps"))
    path = _lib().load().snn_debug_last_fc6_path()
    p6, p7 = head_det_planes(dev, DET_T, d.representation_size, DET_R)
    return [cls, bbox, p6[:DET_T - 1].clone(), p7.clone()], path, None if stat is None else stat.tolist()


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _written(out):
    return not any(bool(torch.isnan(t).any()) for t in out if t.is_floating_point())


def _roi(dev, nhwc=False):
    pool, feats, boxes, shapes = FR.roi_setup(64, DET_R, 40 + DET_T)
    dev_feats = {k: v.to(dev) for k, v in feats.items()}
    if nhwc:
        dev_feats = {k: v.contiguous(memory_format=torch.channels_last) for k, v in dev_feats.items()}
    roi = pool.assign(dev_feats, [b.to(dev) for b in boxes], shapes)
    assert int(roi[2].shape[0]) == DET_R
    return roi


def _heads(gpu_device, which, precision="bf16x3"):
    """-> call(route=None, crossover=None) of the RPN head, the row-fed or the RoIAlign-fed detector head on fixed inputs"""
    if which == "rpn":
        case = _rpn_case()
        m = CR.head_for(case, gpu_device, precision)
        feats = [f.to(gpu_device) for f in case["feats"]]
        return lambda route=None, crossover=None: _rpn_call(m, feats, route, crossover)
    case = _det_case()
    d = FR.head_for(case, gpu_device, precision)
    x = case["x"].to(gpu_device)
    roi = _roi(gpu_device) if which == "det_roialign" else None
    return lambda route=None, crossover=None: _det_call(d, x, roi, route, crossover)


# ---- 1. a routed call does not move the next plain call --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rpn", "det_rows", "det_roialign"])
def test_plain_call_after_a_dense_call_is_the_plain_call(gpu_device, which):
    call = _heads(gpu_device, which)
    first, path, stat = call()
    assert path == 1 and stat is None and _written(first), "the shape has a sparse plan: the plain entry must run it"
    dense, path, stat = call("dense")
    assert path == 0 and stat == [0, 0, 1, 0] and _written(dense)
    again, path, stat = call()
    assert path == 1 and stat is None and _same(again, first)


# ---- 2. a call that returns behind its plan leaves nothing of the plan ----------------------------------------------------------------
def _raw_roialign_auto(lib, d, roi, with_rois, stat):
    """snn_det_head_forward_roialign_routed on `auto` at crossover 2 with every argument spelled out, rois = NULL unless with_rois
    -> (return code, the NaN-filled outputs, the maps' SNN_FEAT_* code)"""
    from snn_automotive_object_detection_amd import ops
    flist, scales, rois, lvl = roi
    table, keep, fdt, Cc, boxes, roi_batch, roi_level = ops._roi_feed(flist, scales, rois[:, 1:5], rois[:, 0], lvl)
    a = d._pass_args(Cc * 49, "maps")
    dev = boxes.device
    out_c = torch.full((DET_R, a["K"]), float("nan"), dtype=torch.float32, device=dev)
    out_b = torch.full((DET_R, a["K4"]), float("nan"), dtype=torch.float32, device=dev)
    ws = ops._WS.get(dev, lib.snn_det_head_workspace_bytes_routed(DET_R, Cc * 49, a["Hd"], a["K"], a["K4"], DET_T, a["p"].precision, 2))
    rc = lib.snn_det_head_forward_roialign_routed(table(keep), fdt, len(keep), Cc, ops._ptr(boxes) if with_rois else None, ops._ptr(roi_batch),
                                                  ops._ptr(roi_level), DET_R, a["Hd"], a["K"], a["K4"], DET_T, Ct.byref(a["p"]),
                                                  ops._ptr(a["w6_packed"]), a["w6_inner"], ops._ptr(a["w7_packed"]), ops._ptr(a["w_heads_packed"]),
                                                  ops._ptr(out_c), ops._ptr(out_b), None, None, None, None, ops._ptr(ws), ws.numel(), 2, 2.0,
                                                  ops._ptr(stat), ops._stream())
    return rc, [out_c, out_b], fdt


@pytest.mark.parametrize("nhwc", [False, True], ids=["refused_by_the_encoder", "no_typed_kernel"])
def test_auto_call_that_returns_behind_its_plan_leaves_no_plan(gpu_device, nhwc):
    L = _lib()
    lib = L.load()
    d = FR.head_for(_det_case(), gpu_device, "bf16x3")
    roi = _roi(gpu_device)
    call = lambda route=None, crossover=None: _det_call(d, None, roi, route, crossover)
    first, path, _ = call()
    assert path == 1 and _written(first)
    assert d.fc6_inner() == 49, "the gated plan needs fc6 in bin-major order"
    stat = _stat(gpu_device)
    rc, out, fdt = _raw_roialign_auto(lib, d, _roi(gpu_device, nhwc=True) if nhwc else roi, False, stat)
    assert fdt == (L.FEAT_NHWC if nhwc else 0)
    assert rc == (L.NO_TYPED_KERNEL if nhwc else -1), (rc, lib.snn_last_error())
    assert nhwc or b"snn_roi_align_encode: bad argument" in lib.snn_last_error()
    torch.cuda.synchronize()
    assert stat.tolist() == [-7] * 4 and all(still_poisoned(t) for t in out), "the refused call enqueued something"
    again, path, _ = call()
    assert path == 1 and _same(again, first)
    never, path, stat = call("auto", 2.0)
    assert path == 2 and stat[2] == 0 and stat[1] > 0 and _same(never, first)
    rc, out, _ = _raw_roialign_auto(lib, d, roi, True, _stat(gpu_device))          # (the raw call itself, well-formed: the gated pair runs)
    assert rc == 0 and lib.snn_debug_last_fc6_path() == 2 and _same(out, first[:2])


# ---- 3. the weight-plane count of a pass is that pass's alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rpn", "det_rows"])
def test_stage_call_after_a_one_plane_pass_runs_three_planes(gpu_device, which):
    from snn_automotive_object_detection_amd import ops
    g = torch.Generator().manual_seed(77)
    T, R, K, N = 6, 50, 128, 96
    planes = torch.randint(-2 ** 31, 2 ** 31 - 1, (T, R, K // 32), dtype=torch.int64, generator=g).to(torch.int32).to(gpu_device)
    w = ops.pack_linear_bf16x3((torch.randn(N, K, generator=g) * 0.05).to(gpu_device))
    p = FR.head_for(_det_case(), gpu_device, "bf16x3")._params("bf16x3")
    with poisoned_outputs():
        stage = ops.spike_gemm_lif_bf16x3(planes, K, N, p, w)
    assert bool(stage.any())
    three = _heads(gpu_device, which, "bf16x3")
    first, path, _ = three()
    assert path == 1 and _written(first)
    one, path, _ = _heads(gpu_device, which, "bf16")()
    assert path == 1 and _written(one)
    with poisoned_outputs():
        assert torch.equal(ops.spike_gemm_lif_bf16x3(planes, K, N, p, w), stage)
    again, path, _ = three()
    assert path == 1 and _same(again, first)
