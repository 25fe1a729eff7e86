"""fp16 / bf16 feature maps straight into both spiking heads (include/snn_hip.h: the *_typed entry points).

A half element means its exact fp32 value, so the yardstick of every check is the EXISTING fp32 path on x.float() - which the rest of the
suite pins to the oracle - and the comparison is torch.equal: outputs, hidden spike planes, counts and rates.  The typed path is never
its own yardstick.  One test ties the half path to the oracle directly, with the suite's tolerance and flip budgets."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._planes import head_det_planes, head_rpn_planes
from tests._util import flip_budget, planes_to_dense

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


def _params():
    from snn_automotive_object_detection_amd import ops
    return ops.make_params(ops.LIFParameters(v_th=torch.tensor(0.25)), ops.LIFParameters(alpha=100, v_th=torch.tensor(0.1)))


def _calls():
    from snn_automotive_object_detection_amd import ops
    return dict(ops.feature_calls)


def _typed_ran(before, dtype, n=1):
    """the typed entry was reached n times since `before` and never answered "no typed kernel\""""
    now, key = _calls(), "f16" if dtype == torch.float16 else "bf16"
    assert now[key] - before[key] == n and now["no_typed_kernel"] == before["no_typed_kernel"], (before, now)


def _same(a, b):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert a.dtype == b.dtype and torch.equal(a, b), float((a.float() - b.float()).abs().max())


# ---- 1. encoder planes, stage level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [4, 8, 16])
@pytest.mark.parametrize("shape", [(2, 64, 13, 19), (1, 48, 7, 10), (2, 256, 5, 3)])      # odd H W; C = 48: per-channel predicate; H W < 64
def test_typed_encode_nchw_planes_equal_the_fp32_call_on_widened_input(gpu_device, dtype, T, shape):
    from snn_automotive_object_detection_amd import ops
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape) + T)) * 1.5).to(gpu_device).to(dtype)
    before = _calls()
    got = ops.encode_nchw(x, T, _params())
    _typed_ran(before, dtype)
    ref = ops.encode_nchw(x.float(), T, _params())
    assert int((ref != 0).sum()) > 0
    _same(got, ref)


# ---- 2. RPN head -----------------------------------------------------------------------------------------------------------------------
def _rpn(dev, C_, T, seed=0):
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(seed)
    m = S.RPNHeadSNN(C_, 3, T).to(dev)
    with torch.no_grad():
        m.shared_conv.weight.mul_(4.0)                       # (so that the shared LIF fires)
    g = torch.Generator().manual_seed(seed + 1)
    feats = [(torch.randn((2, C_, h, w), generator=g) * 1.5).to(dev) for h, w in ((13, 19), (7, 10))]
    return m, feats


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C_,T", [(256, 8), (256, 4), (64, 12)])      # fold + compressed planes + FAT conv; dense conv, no fold; narrow head
def test_rpn_head_on_half_features_equals_the_fp32_path(gpu_device, dtype, C_, T):
    m, feats = _rpn(gpu_device, C_, T)
    half = [f.to(dtype) for f in feats]
    wide = [h.float() for h in half]
    for rates in (False, True):
        m.spike_rates = rates
        before = _calls()
        got = m(half)
        _typed_ran(before, dtype)
        got_planes = head_rpn_planes(gpu_device, T, C_)
        got_counts = m.last_spike_counts.clone() if rates else None
        ref = m(wide)
        ref_planes = head_rpn_planes(gpu_device, T, C_)
        assert all(o.dtype == torch.float32 for o in got[0])
        _same(got, ref)
        _same(got_planes, ref_planes)
        assert int((ref_planes != 0).sum()) > 0
        if rates:
            _same(got_counts, m.last_spike_counts)
    m.spike_rates = False
    before = _calls()
    got = m.forward_readouts(half, (3, 5, 8))
    _typed_ran(before, dtype)
    ref = m.forward_readouts(wide, (3, 5, 8))
    for t in (3, 5, 8):
        _same(got[t], ref[t])


# ---- 3. detector head, pooled rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", [37, 130])
@pytest.mark.parametrize("K,T,rates", [(9, 12, False), (11, 16, True)])
def test_det_head_on_half_pooled_rows_equals_the_fp32_path(gpu_device, dtype, R, K, T, rates):
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(R + K)
    Hd = 128
    head = S.FastRCNNPredictorSNNFull(256 * 49, Hd, K, T).to(gpu_device)
    with torch.no_grad():
        head.fc6.weight.mul_(4.0)
        head.fc7.weight.mul_(4.0)
    head.spike_rates = rates
    x = (torch.randn((R, 256, 7, 7), generator=torch.Generator().manual_seed(R)) * 1.5).to(gpu_device).to(dtype)
    before = _calls()
    got = head(x)
    _typed_ran(before, dtype)
    got_planes = head_det_planes(gpu_device, T, Hd, R)
    got_counts = [c.clone() for c in head.last_spike_counts] if rates else []
    ref = head(x.float())
    ref_planes = head_det_planes(gpu_device, T, Hd, R)
    _same(got, ref)
    _same(got_planes, ref_planes)
    assert int((ref_planes[0] != 0).sum()) > 0
    if rates:
        _same(got_counts, list(head.last_spike_counts))
    got = head.forward_readouts(x, (3, 5, 8))
    ref = head.forward_readouts(x.float(), (3, 5, 8))
    for t in (3, 5, 8):
        _same(got[t], ref[t])


def _det_pair(dev, dtype, C_, R, T, rates, Hd=128, K=5):
    """(head outputs, lif6 / lif7 planes, counts) of a row-fed detector on half rows and on the fp32 tensor they mean; the typed call ran"""
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(R + C_)
    head = S.FastRCNNPredictorSNNFull(C_ * 49, Hd, K, T).to(dev)
    with torch.no_grad():
        head.fc6.weight.mul_(4.0)
        head.fc7.weight.mul_(4.0)
    head.spike_rates = rates
    x = (torch.randn((R, C_, 7, 7), generator=torch.Generator().manual_seed(R)) * 1.5).to(dev).to(dtype)
    out = []
    for feat in (x, x.float()):
        before = _calls()
        o = head(feat)
        if feat is x:
            _typed_ran(before, dtype)
        out.append((o, head_det_planes(dev, T, Hd, R), [c.clone() for c in head.last_spike_counts] if rates else []))
    assert int((out[1][1][0] != 0).sum()) > 0
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", [37, 130])
@pytest.mark.parametrize("knob", [None, "SNN_ENC_QUANT=0", "SNN_ENC_GENERIC=1"])     # the three encoder modes of k_encode_rows_wm_h
def test_det_head_rows_that_take_the_word_major_row_encoder(gpu_device, monkeypatch, dtype, R, knob):
    """C = 96 (C % 64 != 0: the folded encoder does not apply) routes half rows to k_encode_rows_wm_h, whose load phase - 16-byte pieces of
    eight halves, widened on the way into LDS - is its own text: R not a multiple of 32, D = 4704 = 147 words (a ragged last group of 8)"""
    if knob:
        monkeypatch.setenv(*knob.split("="))
    for rates in (False, True):
        got, ref = _det_pair(gpu_device, dtype, 96, R, 12, rates)
        _same(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rb,nw", [("16", "4"), ("8", "8"), ("16", "8"), ("8", "4")])
def test_folded_row_encoder_block_shapes(gpu_device, monkeypatch, dtype, rb, nw):
    """every instantiation of k_encode_rows_perm_h (SNN_ENCP_RB RoIs per block x SNN_ENCP_NW waves)"""
    monkeypatch.setenv("SNN_ENCP_RB", rb)
    monkeypatch.setenv("SNN_ENCP_NW", nw)
    got, ref = _det_pair(gpu_device, dtype, 256, 37, 12, True)
    _same(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("knob", ["SNN_STAGE_PERIODS=1", "SNN_ENC_GENERIC=1", "SNN_ENC_QUANT=0"])
def test_other_encoder_modes_of_the_nchw_and_level_kernels(gpu_device, monkeypatch, dtype, knob):
    """the threshold (period-plane) and op-for-op instantiations of k_encode_nchw_h, and the recurrence / op-for-op ones of k_encode_levels_h"""
    from snn_automotive_object_detection_amd import ops
    monkeypatch.setenv(*knob.split("="))
    x = (torch.randn((2, 48, 7, 10), generator=torch.Generator().manual_seed(3)) * 1.5).to(gpu_device).to(dtype)
    before = _calls()
    got = ops.encode_nchw(x, 8, _params())
    _typed_ran(before, dtype)
    ref = ops.encode_nchw(x.float(), 8, _params())
    assert int((ref != 0).sum()) > 0
    _same(got, ref)
    if knob != "SNN_STAGE_PERIODS=1":
        m, feats = _rpn(gpu_device, 64, 8)
        half = [f.to(dtype) for f in feats]
        before = _calls()
        got = m(half)
        _typed_ran(before, dtype)
        got_planes = head_rpn_planes(gpu_device, 8, 64)
        _same(got, m([h.float() for h in half]))
        _same(got_planes, head_rpn_planes(gpu_device, 8, 64))


# ---- 4. fused RoIAlign ------------------------------------------------------------------------------------------------------------------
def _border_geometry(dev, C_, dtype):
    """the border / tiny-map geometry of the table kernel's own test (tests/test_gpu_roialign.py), with an odd-W level: a 2-pixel-wide level,
    boxes clamped at the far edge, partly and wholly outside the map, degenerate boxes; R = 37"""
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    g = torch.Generator().manual_seed(9)
    sizes = [(16, 15), (8, 7), (4, 4), (2, 2)]                 # W = 15, 7: odd (and narrower than the image: samples beyond the last column); W = 2
    feats = {str(i): (torch.randn((1, C_, h, w), generator=g) * 1.5).to(dev).to(dtype) for i, (h, w) in enumerate(sizes)}
    b = torch.tensor([[0.0, 0.0, 64.0, 64.0], [60.0, 60.0, 64.0, 64.0], [63.5, 0.0, 64.0, 64.0], [-30.0, -30.0, 10.0, 10.0],
                      [0.0, 62.0, 64.0, 66.0], [10.0, 10.0, 500.0, 500.0], [63.9, 63.9, 64.0, 64.0], [0.0, 0.0, 3.0, 3.0]])
    # (the level of a box follows its size: 112 .. 224 px -> level 1, 224 .. 448 px -> level 2; such boxes reach beyond the 64-px image)
    big = torch.tensor([[-50.0, -50.0, 100.0, 100.0], [0.0, 0.0, 130.0, 120.0], [-100.0, -90.0, 150.0, 160.0], [0.0, 0.0, 300.0, 250.0]])
    boxes = [torch.cat([b, big, torch.rand((25, 4), generator=g) * 32 + torch.tensor([0.0, 0.0, 32.0, 32.0])]).to(dev)]
    pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    flist, scales, rois, lvl = pool.assign(feats, boxes, [(64, 64)])
    assert rois.shape[0] == 37 and set(lvl.tolist()) == {0, 1, 2, 3} and all(f.dtype == dtype for f in flist)     # assign hands half maps through
    return flist, scales, rois, lvl


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [12, 16])                    # the fused head: perm kernel (window <= 12 planes); table kernel, then permute + compress
def test_roialign_on_half_maps_equals_the_fp32_path(gpu_device, monkeypatch, dtype, T):
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import _lib, ops
    flist, scales, rois, lvl = _border_geometry(gpu_device, 64, dtype)
    wide = [f.float() for f in flist]
    # stage level: the table kernel's planes (word-major, as the fused head takes them) and pooled values
    monkeypatch.setenv("SNN_STAGE_PLANES", "wm")
    before = _calls()
    got = ops.roi_align_encode(flist, scales, rois[:, 1:5], rois[:, 0], lvl, T, _params(), want_pooled=True)
    _typed_ran(before, dtype)
    ref = ops.roi_align_encode(wide, scales, rois[:, 1:5], rois[:, 0], lvl, T, _params(), want_pooled=True)
    _same(got, ref)
    assert int((ref[0] != 0).sum()) > 0 and float(ref[1].abs().max()) > 0
    monkeypatch.delenv("SNN_STAGE_PLANES")
    # the fused head
    torch.manual_seed(2)
    head = S.FastRCNNPredictorSNNFull(64 * 49, 128, 5, T).to(gpu_device)
    with torch.no_grad():
        head.fc6.weight.mul_(4.0)
        head.fc7.weight.mul_(4.0)
    assert head.fc6_inner() == 49
    for rates in (False, True):
        head.spike_rates = rates
        before = _calls()
        got = head.forward_roialign(flist, scales, rois, lvl)
        _typed_ran(before, dtype)
        got_planes = head_det_planes(gpu_device, T, 128, 37)
        got_counts = [c.clone() for c in head.last_spike_counts] if rates else []
        ref = head.forward_roialign(wide, scales, rois, lvl)
        assert _lib.load().snn_debug_last_fc6_path() == 1
        _same(got, ref)
        _same(got_planes, head_det_planes(gpu_device, T, 128, 37))
        if rates:
            _same(got_counts, list(head.last_spike_counts))
            assert any(int(c.sum()) > 0 for c in got_counts)
    head.spike_rates = False
    got = head.forward_roialign_readouts(flist, scales, rois, lvl, (3, 5, 8))
    ref = head.forward_roialign_readouts(wide, scales, rois, lvl, (3, 5, 8))
    for t in (3, 5, 8):
        _same(got[t], ref[t])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_subnormal_half_values_are_kept_by_the_widening(gpu_device, monkeypatch, dtype):
    """maps of half-precision SUBNORMALS (no encoder threshold can tell them from zero): the pooled values of the typed RoIAlign kernel are those
    of the fp32 path on the widened maps, and they are not zero - a conversion that flushed subnormals would pool zeros"""
    from snn_automotive_object_detection_amd import ops
    flist, scales, rois, lvl = _border_geometry(gpu_device, 64, dtype)
    g = torch.Generator().manual_seed(11)
    top = 0x3FF if dtype == torch.float16 else 0x7F                            # mantissa bits only: exponent field 0
    sub = [(torch.randint(1, top + 1, f.shape, generator=g, dtype=torch.int16) | (torch.randint(0, 2, f.shape, generator=g, dtype=torch.int16) << 15))
           .view(dtype).to(gpu_device) for f in flist]
    assert all(float(f.float().abs().max()) < float(torch.finfo(dtype).tiny) for f in sub)
    monkeypatch.setenv("SNN_STAGE_PLANES", "wm")
    before = _calls()
    _, got = ops.roi_align_encode(sub, scales, rois[:, 1:5], rois[:, 0], lvl, 6, _params(), want_pooled=True)
    _typed_ran(before, dtype)
    _, ref = ops.roi_align_encode([f.float() for f in sub], scales, rois[:, 1:5], rois[:, 0], lvl, 6, _params(), want_pooled=True)
    _same(got, ref)
    assert float(ref.abs().max()) > 0 and int((got != 0).sum()) > got.numel() // 2


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_roi_heads_forward_on_a_half_feature_dict(gpu_device, dtype):
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(0)
    m = S.create_model("cityscapes", 9, True, True, 0, False, False, num_steps_rpn=4, num_steps_detector=6)
    rh = m.roi_heads.to(gpu_device).eval()
    assert rh.fuse_roi_align
    g = torch.Generator().manual_seed(4)
    fm = {str(i): (torch.randn((1, 256, 16 >> i, 32 >> i), generator=g) * 1.5).to(gpu_device).to(dtype) for i in range(4)}
    fm["pool"] = torch.randn((1, 256, 1, 2), generator=g).to(gpu_device).to(dtype)
    xy = torch.rand((50, 2), generator=g) * torch.tensor([100.0, 40.0])
    props = [torch.cat([xy, xy + torch.rand((50, 2), generator=g) * 60 + 2], dim=1).to(gpu_device)]
    before = _calls()
    with torch.no_grad():
        a, _ = rh(fm, props, [(64, 128)])
        _typed_ran(before, dtype)
        b, _ = rh({k: v.float() for k, v in fm.items()}, props, [(64, 128)])
    for k in ("boxes", "scores", "labels", "all_scores", "all_boxes"):
        _same(a[0][k], b[0][k])
    assert a[0]["all_scores"].dtype == torch.float32


# ---- 5. sentinels -----------------------------------------------------------------------------------------------------------------------
def _neighbours(th, dtype):
    """(largest half value <= th, smallest half value > th) for th > 0"""
    t = torch.tensor([float(th)], dtype=torch.float32)
    h = t.to(dtype)
    bits = h.view(torch.int16)
    if float(h.float()) > float(t):
        lo, hi = (bits - 1).view(dtype), h
    else:
        lo, hi = h, (bits + 1).view(dtype)
    assert float(lo.float()) <= float(t) < float(hi.float())
    return lo, hi


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sentinels_at_every_encoder_threshold_and_special_values(gpu_device, dtype):
    from snn_automotive_object_detection_amd import _lib, ops
    T, p = 16, _params()
    th = (C.c_float * 32)()
    assert _lib.load().snn_debug_encoder_thresholds(C.byref(p), th) == 1
    th = np.array(list(th), dtype=np.float32)
    vals = []
    for t in range(T):
        lo, hi = _neighbours(th[t], dtype)
        vals += [lo, hi, -lo, -hi]
    n_finite = len(vals) + 6
    fi = torch.finfo(dtype)
    smallest_sub = torch.tensor([1], dtype=torch.int16).view(dtype)              # fp16: 2^-24
    assert dtype != torch.float16 or float(smallest_sub.float()) == 2.0 ** -24
    vals += [torch.tensor([0.0], dtype=dtype), torch.tensor([-0.0], dtype=dtype), smallest_sub, -smallest_sub,
             torch.tensor([fi.max], dtype=dtype), torch.tensor([-fi.max], dtype=dtype)]
    vals += [torch.tensor([v], dtype=dtype) for v in (float("inf"), float("-inf"), float("nan"))]
    flat = torch.zeros(64 * 15, dtype=dtype)
    slots = [7 * k + 3 for k in range(len(vals))]                                 # slot s -> (channel s // 15, position s % 15)
    for s, v in zip(slots, vals):
        flat[s] = v[0]
    x = flat.view(1, 64, 3, 5).to(gpu_device)
    before = _calls()
    got = ops.encode_nchw(x, T, p)
    _typed_ran(before, dtype)
    ref = ops.encode_nchw(x.float(), T, p)
    _same(got, ref)
    dense = planes_to_dense(got, 64)                                               # [T, 15, 64]
    for k, (s, v) in enumerate(zip(slots, vals)):
        if k >= n_finite:
            continue                                                              # (+-inf, NaN: equal to the fp32 path, divergence as documented)
        f = np.float32(float(v.float()))
        fired = np.nonzero(f >= th[:T])[0]
        n = int(fired[0]) + 1 if fired.size else 0                                 # period: first spike at step n - 1
        want = np.array([1.0 if n and (t + 1) % n == 0 else 0.0 for t in range(T)], dtype=np.float32)
        assert np.array_equal(dense[:, s % 15, s // 15], want), (k, float(f), n, dense[:, s % 15, s // 15])
    assert dense.sum() > 0


# ---- 6. one oracle tie-in ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_half_path_against_the_oracle_on_the_widened_tensors(gpu_device, dtype):
    import snn_automotive_object_detection_amd as S
    from tests._oracle_heads import OracleDetHead, OracleRPNHead
    C_, T = 64, 12
    m, feats = _rpn(gpu_device, C_, T)
    half = [f.to(dtype) for f in feats]
    got_l, got_b = m(half)
    exp_l, exp_b = OracleRPNHead(m)([h.float() for h in half])
    bad, mx, pos = 0, 0.0, 0
    for gl, gb, el, eb in zip(got_l, got_b, exp_l, exp_b):
        d = torch.maximum((gl.cpu() - el).abs().amax(1), (gb.cpu() - eb).abs().amax(1))
        bad += int((d > 1e-4).sum())
        mx = max(mx, float(d.max()))
        pos += d.numel()
    assert bad <= flip_budget(pos, C_, T, "rpn_randn") and mx < 0.05, (bad, mx)
    R, Hd, Td = 37, 128, 12
    torch.manual_seed(5)
    head = S.FastRCNNPredictorSNNFull(256 * 49, Hd, 9, Td).to(gpu_device)
    x = (torch.randn((R, 256, 7, 7), generator=torch.Generator().manual_seed(R)) * 1.5).to(gpu_device).to(dtype)
    cls, reg = head(x)
    e_cls, e_reg = OracleDetHead(head)(x.float().flatten(1))
    off = ((cls.cpu() - e_cls).abs().amax(1) > 1e-4) | ((reg.cpu() - e_reg).abs().amax(1) > 1e-4)
    assert int(off.sum()) <= flip_budget(R, 2 * Hd, Td, "det") and float((cls.cpu() - e_cls).abs().max()) < 0.05, int(off.sum())


# ---- 7. no widening happened ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_half_features_are_not_widened_on_the_way_in(gpu_device, dtype):
    m, feats = _rpn(gpu_device, 256, 8)
    half = [f.to(dtype) for f in feats]
    m([h.float() for h in half])                                                 # (sizes the cached workspace)
    fp32_bytes = sum(h.numel() for h in half) * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu_device)
    base = torch.cuda.memory_allocated(gpu_device)
    before = _calls()
    m(half)
    _typed_ran(before, dtype)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(gpu_device) - base
    assert grown < fp32_bytes, (grown, fp32_bytes)


# ---- 8. a launch plan without a typed kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", IDS)
def test_plan_without_a_typed_kernel_widens_and_gives_the_fp32_results(gpu_device, dtype):
    """fresh process: the knobs freeze at first use.  SNN_ROI_TAB=0 selects the per-element RoIAlign kernels, which have no typed form"""
    env = dict(os.environ, SNN_ROI_TAB="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_half_features_child.py"), dtype], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "no_typed_kernel=1 equal=True" in r.stdout, r.stdout[-2000:]


# ---- 9. mixed dtypes across levels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mixed_dtypes_across_levels_raise(gpu_device, dtype):
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd._lib import SnnHipError
    m, feats = _rpn(gpu_device, 64, 4)
    with pytest.raises(SnnHipError, match="share a dtype"):
        m([feats[0].to(dtype), feats[1]])
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    with pytest.raises(SnnHipError, match="share a dtype"):
        m([feats[0].to(dtype), feats[1].to(other)])
    flist, scales, rois, lvl = _border_geometry(gpu_device, 64, dtype)
    with pytest.raises(SnnHipError, match="share a dtype"):
        ops.roi_align_encode([flist[0].float()] + flist[1:], scales, rois[:, 1:5], rois[:, 0], lvl, 6, _params())
