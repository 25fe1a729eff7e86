"""Any-time readouts on the GPU: one head pass at T = steps[-1] with a readout per T' (include/snn_hip.h, snn_*_readouts).

* the readout kernels against the single-readout heads at T' on the same planes, bit for bit (mfma / ksplit / column blocks /
  the fp32 VALU kernel);
* the readout at T' = T against the plain forward at T, bit for bit (outputs, counts, rates);
* every readout against the oracle at T' within the smoke budgets;
* timestep_sweep against standalone models at every pair of a 2 x 2 grid."""
import numpy as np
import pytest
import torch

import snn_automotive_object_detection_amd as S
from snn_automotive_object_detection_amd import ops
from snn_automotive_object_detection_amd.sweep import timestep_sweep
from oracle import fixtures as FX
from oracle import snn_oracle as OR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _params(prec):
    m = S.RPNHeadSNN(64, 3, 8)
    return m, ops.make_params(m.p_enc, m.p_lif, m.dt, m.li_order, prec)


@pytest.mark.parametrize("K,NA,NB,T,M,prec", [
    (256, 3, 12, 12, 1000, "bf16x3"),      # k_li_heads_mfma_ro, NT = 1
    (256, 5, 20, 16, 777, "bf16x3"),       # NT = 2
    (1024, 9, 36, 16, 333, "bf16x3"),      # k_li_heads_ksplit_ro, NT = 3
    (1024, 91, 364, 12, 130, "bf16x3"),    # ksplit, column blocks of 64
    (1024, 9, 36, 24, 45, "bf16x3"),       # ksplit, two time groups
    (256, 3, 12, 12, 500, "f32_strict"),   # fp32 VALU kernel, one launch per readout
])
@pytest.mark.parametrize("sums", [False, True])
def test_readout_kernels_equal_single_readout_heads(K, NA, NB, T, M, prec, sums):
    g = torch.Generator().manual_seed(K + NA + T + M)
    planes = torch.randint(-2 ** 31, 2 ** 31, (T, M, K // 32), generator=g, dtype=torch.int64).to(torch.int32)
    planes &= torch.randint(-2 ** 31, 2 ** 31, planes.shape, generator=g, dtype=torch.int64).to(torch.int32)   # ~25 % density
    planes = planes.to(DEV)
    wa = (torch.randn(NA, K, generator=g) * 0.02).to(DEV)
    wb = (torch.randn(NB, K, generator=g) * 0.02).to(DEV)
    wp = ops.pack_heads(wa, wb)
    _, p = _params(prec)
    for steps in (tuple(range(1, T + 1)), tuple(t for t in range(4, 13) if t <= T)):
        got = ops.li_heads_readouts(planes, K, wp, NA, NB, p, steps, want_sums=sums)
        for j, Tp in enumerate(steps):
            exp = ops.li_heads(planes[:Tp].contiguous(), K, wp, NA, NB, p, want_sums=sums)
            for a, b in zip(got, exp):
                assert torch.equal(a[j], b), (steps, Tp)


@pytest.mark.parametrize("form,K,NA,NB,T,M", [
    ("mfma", 1024, 9, 36, 12, 45),         # k_li_heads_mfma_ro with W streamed (288 KB of planes), NT = 3
    ("ksplit", 256, 3, 12, 24, 45),        # k_li_heads_ksplit_ro by force, NT = 1: groups of 16 steps, two of them
    ("ksplit", 128, 5, 20, 5, 17),         # four words per row: one chunk per wave; last group of 4 accumulator steps, tn odd
])
@pytest.mark.parametrize("sums", [False, True])
def test_readout_kernels_forced_forms_equal_single_readout_heads(monkeypatch, form, K, NA, NB, T, M, sums):
    """the readout kernels where only SNN_LI_HEADS takes them (the streamed matrix-core loop, the reduction-split form on shapes whose W
    fits LDS): every readout against the single-readout heads of the same forced form on the first T' planes, bit for bit"""
    monkeypatch.setenv("SNN_LI_HEADS", form)
    g = torch.Generator().manual_seed(K + NA + T + M)
    planes = torch.randint(-2 ** 31, 2 ** 31, (T, M, K // 32), generator=g, dtype=torch.int64).to(torch.int32)
    planes &= torch.randint(-2 ** 31, 2 ** 31, planes.shape, generator=g, dtype=torch.int64).to(torch.int32)   # ~25 % density
    planes = planes.to(DEV)
    wa = (torch.randn(NA, K, generator=g) * 0.02).to(DEV)
    wb = (torch.randn(NB, K, generator=g) * 0.02).to(DEV)
    wp = ops.pack_heads(wa, wb)
    _, p = _params("bf16x3")
    steps = tuple(range(1, T + 1))
    got = ops.li_heads_readouts(planes, K, wp, NA, NB, p, steps, want_sums=sums)
    for j, Tp in enumerate(steps):
        exp = ops.li_heads(planes[:Tp].contiguous(), K, wp, NA, NB, p, want_sums=sums)
        for a, b in zip(got, exp):
            assert torch.equal(a[j], b), Tp
    for a in got:                                                   # not vacuous: no readout is all zero, and the readouts differ
        assert all(bool(a[j].any()) for j in range(T))
        assert any(not torch.equal(a[0], a[j]) for j in range(1, T))


def _rpn_module(spec, prec):
    feats, w_s, w_c, w_b = FX.rpn_inputs(spec)
    m = S.RPNHeadSNN(spec["C"], spec["A"], spec["T"]).to(DEV)
    m.load_state_dict({"shared_conv.weight": w_s, "conv_cls.weight": w_c, "conv_bbox.weight": w_b})
    m.precision = prec
    return m, feats, (w_s, w_c, w_b)


@pytest.mark.parametrize("name,Tmax", [("rpn_c256_T8_odd", 8), ("rpn_c256_T12", 12), ("rpn_c64_A5_T8", 16)])
@pytest.mark.parametrize("prec", ["bf16x3", "f32", "f32_strict"])
def test_rpn_readouts(name, Tmax, prec):
    spec = FX.RPN_SPECS[name]
    m, feats, (w_s, w_c, w_b) = _rpn_module(spec, prec)
    x = [f.to(DEV) for f in feats]
    steps = tuple(range(1, Tmax + 1))
    out = m.forward_readouts(x, steps)
    assert m.num_steps == spec["T"]
    m.num_steps = Tmax
    plain = m(x)                                                    # contract 2: T' = T is the plain forward
    for a, b in zip(out[Tmax][0] + out[Tmax][1], plain[0] + plain[1]):
        assert torch.equal(a, b)
    for Tp in (1, 2, 4, 5, Tmax // 2 + 1, Tmax):                    # contract 3: the oracle at T'
        o_l, o_b = OR.rpn_head_forward(feats, w_s, w_c, w_b, Tp)
        bad = 0
        for a, b in zip(out[Tp][0] + out[Tp][1], list(o_l) + list(o_b)):
            d = (a.cpu() - b).abs()
            bad += int((d > 1e-4).sum())
            assert float(d.max()) < 0.05, Tp
        assert bad <= 6, (Tp, bad)


@pytest.mark.parametrize("name,Tmax", [("det_K9_T12", 12), ("det_K11_T8_R37", 16), ("det_K9_T12_R130", 24)])
def test_det_readouts(name, Tmax):
    spec = FX.DET_SPECS[name]
    x, w6, w7, wc, wb = FX.det_inputs(spec)
    d = S.FastRCNNPredictorSNNFull(spec["C"] * 49, spec["Hd"], spec["K"], spec["T"]).to(DEV)
    d.load_state_dict({"fc6.weight": w6, "fc7.weight": w7, "cls_score.weight": wc, "bbox_pred.weight": wb})
    steps = (4, 5, 8, 11, Tmax)
    out = d.forward_readouts(x.to(DEV), steps)
    d.num_steps = Tmax
    c, b = d(x.to(DEV))
    assert torch.equal(out[Tmax][0], c) and torch.equal(out[Tmax][1], b)
    for Tp in steps:
        o_c, o_d = OR.det_head_forward(x, w6, w7, wc, wb, Tp)
        rows_bad = int((((out[Tp][0].cpu() - o_c).abs() > 1e-4).any(1) | ((out[Tp][1].cpu() - o_d).abs() > 1e-4).any(1)).sum())
        assert rows_bad <= 1, (Tp, rows_bad)


def test_spike_rate_readouts_at_T_equal_the_plain_forward():
    spec = FX.RPN_SPECS["rpn_c256_T8_odd"]
    m, feats, _ = _rpn_module(spec, "bf16x3")
    m.spike_rates = True
    x = [f.to(DEV) for f in feats]
    out = m.forward_readouts(x, (3, 5, 8))
    m.num_steps = 8
    plain = m(x)
    for a, b in zip(out[8][2], plain[2]):
        assert torch.equal(a, b)
    for Tp in (3, 5):                                              # a standalone spike-rate forward at T' (up to threshold ties)
        m.num_steps = Tp
        ref = m(x)[2]
        for a, b in zip(out[Tp][2], ref):
            assert torch.allclose(a, b, rtol=1e-3, atol=1e-4), Tp
    spec = FX.DET_SPECS["det_K9_T12"]
    xd, w6, w7, wc, wb = FX.det_inputs(spec)
    d = S.FastRCNNPredictorSNNFull(spec["C"] * 49, spec["Hd"], spec["K"], 12).to(DEV)
    d.load_state_dict({"fc6.weight": w6, "fc7.weight": w7, "cls_score.weight": wc, "bbox_pred.weight": wb})
    d.spike_rates = True
    out = d.forward_readouts(xd.to(DEV), (6, 12))
    plain = d(xd.to(DEV))
    for a, b in zip(out[12], plain):
        assert torch.equal(a, b)


class _FirstFeatures(torch.nn.Module):
    """the backbone's features of its first call, returned for every later call: the stock fp32 backbone (MIOpen convolutions) need
    not give the same bits twice, and the sweep is compared with the standalone models on the same features"""

    def __init__(self, backbone):
        super().__init__()
        self.backbone, self.out = backbone, None

    def forward(self, x):
        if self.out is None:
            self.out = self.backbone(x)
        return self.out


def test_timestep_sweep_equals_standalone_models():
    torch.manual_seed(0)
    imgs = [torch.rand(3, 96, 160, device=DEV), torch.rand(3, 80, 128, device=DEV)]
    base = S.create_model("cityscapes", 9).to(DEV).eval()
    base.transform.min_size, base.transform.max_size = 96, 160
    weights = base.state_dict()
    base.backbone = _FirstFeatures(base.backbone)
    grid = timestep_sweep(base, imgs, [6, 12], [8, 16])
    assert base.rpn.head.num_steps == 12 and base.roi_heads.box_head_and_predictor.num_steps == 16
    diffs = []
    for (tr, td), dets in grid.items():
        m = S.create_model("cityscapes", 9, num_steps_rpn=tr, num_steps_detector=td).to(DEV).eval()
        m.load_state_dict(weights)
        m.backbone = base.backbone
        m.transform.min_size, m.transform.max_size = 96, 160
        ref = m(imgs)
        for a, b in zip(dets, ref):
            for k in ("boxes", "scores", "labels"):
                if not torch.equal(a[k], b[k]):
                    diffs.append((tr, td, k))
    assert not diffs, diffs
