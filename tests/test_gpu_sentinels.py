"""Sentinel neurons (tests/_sentinels.py) through the public modules: every head output is a sentinel whose value is known on the host,
so the production kernels' bf16x3 / fp32 arithmetic is pinned without a flip budget or a tie margin.

 * hidden spike trains (shared conv + LIF, fc6 + LIF, fc7 + LIF) are predicted bit for bit; boundary pairs (adjacent floats whose trains
   differ) make one ulp of a sentinel current visible as a whole spike;
 * LI head outputs are within head_tolerance (the bound derived in tests/_sentinels.py: (2n + 2) 2^-24 sum_j kappa_j |u| for n spikes,
   <= 4 ulps for one) of the fp64 LI recursion; where no spike reached a head the output is exactly 0;
 * the all-sentinel RPN configuration makes the spike-rate mode's integer counts exact.
tests/test_sentinels_cpu.py proves on the oracle that every weight mutant a kernel bug could cause fails these assertions.
The largest observed ulp error per test is recorded (tests/_util.record_parity)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _sentinels as S
from tests._util import record_parity

pytestmark = pytest.mark.gpu

PYRAMID = [(37, 53), (7, 9), (1, 1), (1, 3)]
BASELINE_PYRAMID = [(192, 384), (96, 192), (48, 96), (24, 48), (12, 24)]       # 768 x 1536 images, strides 4 .. 64


@functools.lru_cache(maxsize=None)
def _rpn_case(C, A, T, shapes, N, seed, li_order="jump_first", all_sentinel=False):
    return S.rpn_case(C, A, T, list(shapes), N=N, seed=seed, li_order=li_order, all_sentinel=all_sentinel)


@functools.lru_cache(maxsize=None)
def _det_case(C, Hd, K, T, R, seed, li_order="jump_first"):
    return S.det_case(C, Hd, K, T, R, seed=seed, li_order=li_order)


def _rpn_module(case, dev, precision):
    import snn_automotive_object_detection_amd as pkg
    m = pkg.RPNHeadSNN(case["C"], case["A"], case["T"]).to(dev)
    m.precision = precision
    m.li_order = case["li_order"]
    m.load_state_dict({"shared_conv.weight": case["w_shared"].view(case["C"], case["C"], 3, 3), "conv_cls.weight": case["w_cls"],
                       "conv_bbox.weight": case["w_bbox"]})
    return m


def _det_module(case, dev, precision):
    import snn_automotive_object_detection_amd as pkg
    m = pkg.FastRCNNPredictorSNNFull(case["C"] * 49, case["Hd"], case["K"], case["T"]).to(dev)
    m.precision = precision
    m.li_order = case["li_order"]
    m.load_state_dict({"fc6.weight": case["w6"], "fc7.weight": case["w7"], "cls_score.weight": case["w_cls"],
                       "bbox_pred.weight": case["w_bbox"]})
    return m


def _run_rpn(case, dev, precision="bf16x3", sparse=None, what=""):
    from snn_automotive_object_detection_amd import _lib
    m = _rpn_module(case, dev, precision)
    lg, bb = m([f.to(dev) for f in case["feats"]])
    if sparse is not None:
        assert _lib.load().snn_debug_last_conv_path() == int(sparse)
    bad, mx = S.check_levels(S.rpn_outputs(lg, bb), case)
    record_parity("sentinels_rpn" + what, T=case["T"], precision=precision, max_ulps=round(mx, 3), bad=bad)
    assert bad == 0, "%d sentinel outputs off their bound (largest error %.1f ulps)" % (bad, mx)
    return mx


def _run_det(case, dev, precision="bf16x3", fc6_sparse=None, what="", x=None):
    from snn_automotive_object_detection_amd import _lib
    m = _det_module(case, dev, precision)
    cls, bbox = m((case["x"] if x is None else x).to(dev))
    if fc6_sparse is not None:
        assert _lib.load().snn_debug_last_fc6_path() == int(fc6_sparse)
    got = S.det_outputs(cls, bbox)
    bad, mx = S.check(got, case["exp"], case["tol"])
    record_parity("sentinels_det" + what, T=case["T"], R=case["R"], precision=precision, max_ulps=round(mx, 3), bad=bad)
    assert bad == 0, "%d sentinel outputs off their bound (largest error %.1f ulps)" % (bad, mx)
    return mx


# ---- RPN head ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 8, 12, 16])
def test_rpn_sentinels(gpu_device, T):
    """the default sparse conv + LIF (T = 5: 8-wave; 8 / 12 / 16: the FAT shapes) and the default LI heads"""
    _run_rpn(_rpn_case(256, 3, T, tuple(PYRAMID), 2, T), gpu_device, sparse=True)


@pytest.mark.parametrize("knob,value,sparse", [("SNN_SPARSE", "0", False), ("SNN_PLANES", "rm", None),
                                               ("SNN_LI_HEADS", "valu", True), ("SNN_LI_HEADS", "mfma", True),
                                               ("SNN_LI_HEADS", "ksplit", True)])
def test_rpn_sentinels_under_knobs(gpu_device, monkeypatch, knob, value, sparse):
    monkeypatch.setenv(knob, value)
    _run_rpn(_rpn_case(256, 3, 8, tuple(PYRAMID), 2, 8), gpu_device, sparse=sparse, what="_%s_%s" % (knob, value))


@pytest.mark.parametrize("precision", ["f32", "f32_strict"])
def test_rpn_sentinels_fp32_precisions(gpu_device, precision):
    _run_rpn(_rpn_case(256, 3, 8, tuple(PYRAMID), 2, 8), gpu_device, precision)


def test_rpn_sentinels_voltage_first(gpu_device):
    _run_rpn(_rpn_case(256, 3, 12, tuple(PYRAMID), 2, 21, "voltage_first"), gpu_device, sparse=True, what="_voltage_first")


@pytest.mark.parametrize("T", [8, 16])
def test_rpn_all_sentinel_spike_counts_are_exact(gpu_device, T):
    """every weight row one-hot: the spike-rate mode's integer counts and the rate column derived from them equal the host's exactly"""
    case = _rpn_case(256, 3, T, tuple(PYRAMID), 2, 30 + T, all_sentinel=True)
    _run_rpn(case, gpu_device, what="_all")
    m = _rpn_module(case, gpu_device, "bf16x3")
    m.spike_rates = True
    lg, bb, rates = m([f.to(gpu_device) for f in case["feats"]])
    bad, _ = S.check_levels(S.rpn_outputs(lg, bb), case)
    assert bad == 0
    cnt = m.last_spike_counts[:, :case["N"]].cpu().numpy()
    assert np.array_equal(cnt, case["counts"]), (cnt, case["counts"])
    for l, (H, W) in enumerate(case["shapes"]):
        exp_rate = (case["counts"][l].astype(np.float64) / (T * case["C"] * H * W)).astype(np.float32)
        assert np.array_equal(rates[3 * l][:, 0].cpu().numpy(), exp_rate)


@pytest.mark.sweep
@pytest.mark.parametrize("T", [5, 8, 12, 16])
@pytest.mark.parametrize("precision", ["bf16x3", "f32", "f32_strict"])
@pytest.mark.parametrize("knob", [None, ("SNN_SPARSE", "0"), ("SNN_PLANES", "rm"), ("SNN_LI_HEADS", "valu"), ("SNN_LI_HEADS", "mfma"),
                                  ("SNN_LI_HEADS", "ksplit")])
@pytest.mark.parametrize("li_order", ["jump_first", "voltage_first"])
def test_rpn_sentinels_grid(gpu_device, monkeypatch, T, precision, knob, li_order):
    if knob is not None:
        monkeypatch.setenv(*knob)
    _run_rpn(_rpn_case(256, 3, T, tuple(PYRAMID), 2, 40 + T, li_order), gpu_device, precision, what="_grid")


@pytest.mark.sweep
def test_rpn_sentinels_baseline_size(gpu_device):
    """the bench's pyramid: 768 x 1536 images, b = 2, T = 8"""
    _run_rpn(_rpn_case(256, 3, 8, tuple(BASELINE_PYRAMID), 2, 99), gpu_device, sparse=True, what="_baseline")


# ---- detector head -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,R", [(8, 17), (12, 300), (24, 1)])
def test_det_sentinels(gpu_device, T, R):
    """default path: fc6 on the structured-sparse instruction (FAT shape; T = 24: sp_lif_general), fc7 bf16x3 GEMM + LIF, LI heads"""
    _run_det(_det_case(64, 256, 9, T, R, T), gpu_device, fc6_sparse=True)


@pytest.mark.parametrize("knob,value,fc6_sparse", [("SNN_SPARSE_FAT", "0", True), ("SNN_SPARSE", "0", False)])
def test_det_sentinels_under_knobs(gpu_device, monkeypatch, knob, value, fc6_sparse):
    monkeypatch.setenv(knob, value)
    _run_det(_det_case(64, 256, 9, 12, 300, 12), gpu_device, fc6_sparse=fc6_sparse, what="_%s_%s" % (knob, value))


@pytest.mark.parametrize("precision", ["f32", "f32_strict"])
def test_det_sentinels_fp32_precisions(gpu_device, precision):
    _run_det(_det_case(64, 256, 9, 12, 300, 12), gpu_device, precision)


def test_det_sentinels_voltage_first(gpu_device):
    _run_det(_det_case(64, 256, 9, 12, 17, 5, "voltage_first"), gpu_device, what="_voltage_first")


def _roi_inputs(case, dev, n_img=2, per_img=None, seed=0):
    """FPN maps whose sentinel feature channels are constant (RoIAlign of a constant is that constant up to an ulp, which a mid-interval
    input absorbs) and RoIs inside the images"""
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    g = torch.Generator().manual_seed(seed)
    C = case["C"]
    chans = {}
    for d, v in case["feature_values"].items():
        chans[d // 49] = v
    feats = {}
    for i, (h, w) in enumerate([(96, 160), (48, 80), (24, 40), (12, 20)]):
        f = torch.randn((n_img, C, h, w), generator=g) * 1.7
        for c, v in chans.items():
            f[:, c] = v
        feats[str(i)] = f.to(dev)
    R = case["R"]
    per_img = per_img or [R - R // 2, R // 2]
    boxes = []
    for n in range(n_img):
        k = per_img[n]
        xy = torch.rand((k, 2), generator=g) * torch.tensor([500.0, 300.0])
        wh = torch.exp(torch.rand((k, 2), generator=g) * 4.0 + 1.0)
        b = torch.cat([xy, torch.minimum(xy + wh, torch.tensor([639.0, 383.0]))], dim=1)
        boxes.append(b.to(dev))
    pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    return pool, feats, boxes, [(384, 640)] * n_img


@pytest.mark.parametrize("T", [12, 24])
def test_det_sentinels_roialign_fused(gpu_device, T):
    """forward_roialign: T <= 12 folds the compression into the RoIAlign encoder (k_roi_align_encode_perm), T = 24 takes the table
    kernel and a separate compression"""
    case = _det_case(64, 256, 9, T, 300, 60 + T)
    pool, feats, boxes, shapes = _roi_inputs(case, gpu_device, seed=T)
    flist, scales, rois, lvl = pool.assign(feats, boxes, shapes)
    m = _det_module(case, gpu_device, "bf16x3")
    cls, bbox = m.forward_roialign(flist, scales, rois, lvl)
    got = S.det_outputs(cls, bbox)
    bad, mx = S.check(got, case["exp"], case["tol"])
    record_parity("sentinels_det_roialign", T=T, R=case["R"], max_ulps=round(mx, 3), bad=bad)
    assert bad == 0, (bad, mx)


@pytest.mark.sweep
@pytest.mark.parametrize("T", [8, 12, 24])
@pytest.mark.parametrize("R", [1, 17, 300])
@pytest.mark.parametrize("precision", ["bf16x3", "f32", "f32_strict"])
@pytest.mark.parametrize("knob", [None, ("SNN_SPARSE_FAT", "0"), ("SNN_SPARSE", "0"), ("SNN_LI_HEADS", "valu"), ("SNN_LI_HEADS", "ksplit")])
@pytest.mark.parametrize("li_order", ["jump_first", "voltage_first"])
def test_det_sentinels_grid(gpu_device, monkeypatch, T, R, precision, knob, li_order):
    if knob is not None:
        monkeypatch.setenv(*knob)
    _run_det(_det_case(64, 256, 9, T, R, 70 + T, li_order), gpu_device, precision, what="_grid")


@pytest.mark.sweep
def test_det_sentinels_baseline_size(gpu_device):
    """production shapes: 256 x 49 features, 1024 hidden units, 9 classes, 2000 RoIs at T = 12, direct and RoIAlign-fused"""
    case = _det_case(256, 1024, 9, 12, 2000, 98)
    _run_det(case, gpu_device, fc6_sparse=True, what="_baseline")
    pool, feats, boxes, shapes = _roi_inputs(case, gpu_device, seed=98)
    flist, scales, rois, lvl = pool.assign(feats, boxes, shapes)
    cls, bbox = _det_module(case, gpu_device, "bf16x3").forward_roialign(flist, scales, rois, lvl)
    bad, mx = S.check(S.det_outputs(cls, bbox), case["exp"], case["tol"])
    record_parity("sentinels_det_roialign_baseline", T=12, R=2000, max_ulps=round(mx, 3), bad=bad)
    assert bad == 0, (bad, mx)
