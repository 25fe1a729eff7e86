"""Spike taps on the GPU (include/snn_hip.h: snn_*_planes_view, snn_planes_counts, snn_planes_raster_*).  Every tap
output is an integer or a boolean, so every comparison is exact: against an independent numpy reading of the same planes
(tests/_planes.py), against the pass's own counts, against the oracle's spike trains on dyadic grids, against the any-time readouts,
across workspace fills and inside a captured graph."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _exact_grid as G
from tests import _taps as TP
from tests._planes import head_det_planes, head_rpn_planes

pytestmark = pytest.mark.gpu

RPN_PYRAMIDS = ((2, ((5, 7), (3, 4))), (1, ((1, 1),)))              # (N, level shapes): odd W, P = 94 (no multiple of 16); one position
RPN_C = (40, 96, 128, 256)                                           # padding bits, an odd word count, blocks of four words
RPN_T = (2, 8, 17)
DET_R, DET_HD, DET_T = (1, 17, 50), (72, 128, 1024), (4, 12, 24)
DET_C = 64                                                           # RoI input 64 x 7 x 7


def _pkg():
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import _lib, ops, taps
    return S, _lib, ops, taps


def _rpn_head(C_, T, dev, seed=0, precision="bf16x3"):
    S, _, _, _ = _pkg()
    torch.manual_seed(1000 + seed + C_)
    m = S.RPNHeadSNN(C_, 3, T).to(dev)
    with torch.no_grad():
        m.shared_conv.weight.mul_(4.0)                               # spikes must reach the shared LIF
    m.precision = precision
    return m


def _rpn_feats(N, shapes, C_, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(N, C_, h, w, generator=g) * 1.7).to(dev) for h, w in shapes]


def _det_head(Hd, T, dev, seed=0, precision="bf16x3", C_=DET_C):
    S, _, _, _ = _pkg()
    torch.manual_seed(2000 + seed + Hd)
    d = S.FastRCNNPredictorSNNFull(C_ * 49, Hd, 9, T).to(dev)
    with torch.no_grad():
        d.fc7.weight.mul_(3.0)
    d.precision = precision
    return d


def _det_x(R, dev, seed=0, C_=DET_C):
    return (torch.randn(R, C_, 7, 7, generator=torch.Generator().manual_seed(seed)) * 2).to(dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.int64)


def _check_rpn_taps(taps, spk, N, shapes, C_, T, raster):
    """taps of one pass against the dense spike train bool [T, P, C] of all levels"""
    pos = 0
    for l, (h, w) in enumerate(shapes):
        s = spk[:, pos:pos + N * h * w]
        per_step, per_col, per_row = TP.expected_counts(s, [h * w] * N)
        t = taps["shared_lif"][l]
        assert t["per_step"].shape == (N, T) and t["per_step"].dtype == torch.int64
        assert t["per_channel"].shape == (N, C_) and t["per_position"].shape == (N, h, w)
        assert np.array_equal(_np(t["per_step"]), per_step.T), "per_step, level %d" % l
        assert np.array_equal(_np(t["per_channel"]), per_col), "per_channel, level %d" % l
        assert np.array_equal(_np(t["per_position"]).reshape(-1), per_row), "per_position, level %d" % l
        if raster:
            r = t["raster"]
            assert r.dtype == torch.bool and r.shape == (T, N, C_, h, w)
            want = torch.from_numpy(s.reshape(T, N, h, w, C_)).permute(0, 1, 4, 2, 3)
            assert torch.equal(r.cpu(), want), "raster, level %d" % l
        else:
            assert "raster" not in t
        pos += N * h * w


def _check_det_taps(taps, s6, s7, groups, Hd, T, raster):
    for name, s in (("lif6", s6), ("lif7", s7)):
        per_step, per_col, per_row = TP.expected_counts(s, groups)
        t = taps[name]
        assert t["per_step"].shape == (len(groups), T) and t["per_step"].dtype == torch.int64 and t["per_channel"].shape == (len(groups), Hd)
        assert np.array_equal(_np(t["per_step"]), per_step.T), name
        assert np.array_equal(_np(t["per_channel"]), per_col), name
        assert np.array_equal(_np(t["per_roi"]), per_row), name
        if raster:
            assert t["raster"].dtype == torch.bool and torch.equal(t["raster"].cpu(), torch.from_numpy(s)), name


# ---- 1 + 2: the taps equal an independent reading of the same planes, and the pass's own counts ---------------------------------------------
def test_rpn_taps_equal_the_planes_and_the_pass_counts(gpu_device):
    _, _lib, ops, taps_mod = _pkg()
    layouts = set()
    for C_ in RPN_C:
        m = _rpn_head(C_, 8, gpu_device)
        for T in RPN_T:
            m.num_steps = T
            for N, shapes in RPN_PYRAMIDS:
                feats = _rpn_feats(N, shapes, C_, gpu_device, seed=T)
                m.spike_rates = True
                want = m(feats)                                              # the spike-rate-mode pass ...
                planes = head_rpn_planes(gpu_device, T, C_)                  # ... and its planes through the debug accessor, unpacked in numpy
                counts_want = m.last_spike_counts.clone()
                m.spike_rates = False
                logits, bbox, taps = m.forward_tapped(feats, raster=True)
                assert m.spike_rates is False and m.num_steps == T
                spk = TP.dense(planes.cpu().numpy().view(np.uint32), C_)
                assert spk.any() or T < 8, "no spikes: the case says nothing"          # (T = 2: the shared LIF cannot have fired yet)
                _check_rpn_taps(taps, spk, N, shapes, C_, T, raster=True)
                # a tapped pass IS the spike-rate pass: outputs, counts, sums bit for bit
                for a, b in zip(list(logits) + list(bbox), list(want[0]) + list(want[1])):
                    assert torch.equal(a, b)
                assert torch.equal(taps["pass"]["spike_counts"], counts_want)
                for got, ref in zip(taps_mod.rpn_rate_list(taps), want[2]):
                    assert torch.equal(got, ref)
                # 2: the per-group sums agree with the pass's own counters and with each other
                for l in range(len(shapes)):
                    t = taps["shared_lif"][l]
                    total = t["per_step"].sum(1)
                    assert torch.equal(total, counts_want[l, :N])
                    assert torch.equal(t["per_channel"].sum(1, dtype=torch.int64), total) and torch.equal(t["per_position"].sum((1, 2), dtype=torch.int64), total)
                v = taps_mod.rpn_planes_view([(N, h, w) for h, w in shapes], C_, 3, T, m._params())
                layouts.add(int(v.layout))
                assert int(v.layout) == (TP.SPLIT4 if _split_flag() else TP.ROWS)        # what the pass itself reported
    assert layouts == {TP.ROWS, TP.SPLIT4}, "the grid must reach plain rows and blocks of four words, saw %s" % sorted(layouts)


def _split_flag():
    _, _lib, _, _ = _pkg()
    off3 = (C.c_uint64 * 3)()
    _lib.load().snn_debug_last_rpn_planes(off3)
    return int(off3[1])


def test_rpn_raster_only_for_the_levels_asked_for(gpu_device):
    """... and a level whose H W is a multiple of 16 (sixteen positions per store) beside one that is not"""
    shapes = ((4, 8), (3, 4))
    m = _rpn_head(96, 8, gpu_device)
    feats = _rpn_feats(2, shapes, 96, gpu_device)
    _, _, both = m.forward_tapped(feats, raster=True)
    spk = TP.dense(head_rpn_planes(gpu_device, 8, 96).cpu().numpy().view(np.uint32), 96)
    _check_rpn_taps(both, spk, 2, shapes, 96, 8, raster=True)
    _, _, taps = m.forward_tapped(feats, raster=True, levels=[1])
    assert "raster" not in taps["shared_lif"][0] and taps["shared_lif"][1]["raster"].shape == (8, 2, 96, 3, 4)
    _, _, none = m.forward_tapped(feats)
    assert all("raster" not in t for t in none["shared_lif"])
    assert torch.equal(none["shared_lif"][1]["per_step"], taps["shared_lif"][1]["per_step"])


def _det_splits(R):
    return [[R]] + ([[R - 1, 1]] if R > 1 else [])


def _run_det_grid(dev, cases, layouts):
    _, _lib, ops, taps_mod = _pkg()
    heads = {}
    for Hd, T, R, precision in cases:
        if (Hd, precision) not in heads:
            heads[(Hd, precision)] = _det_head(Hd, T, dev, precision=precision)
        d = heads[(Hd, precision)]
        d.num_steps = T
        x = _det_x(R, dev, seed=R + T)
        d.spike_rates = True
        rates_want = d(x)
        p6, p7 = head_det_planes(dev, T, Hd, R)
        s6, s7 = TP.dense(p6.cpu().numpy().view(np.uint32), Hd), TP.dense(p7.cpu().numpy().view(np.uint32), Hd)
        c6_want, c7_want = [c.clone() for c in d.last_spike_counts]
        d.spike_rates = False
        cls_plain, bbox_plain = d(x)
        assert (s6.any() and s7.any()) or T < 12, "no spikes: the case says nothing"      # (T = 4: lif7 has hardly had the time to fire)
        for groups in _det_splits(R):
            cls, bbox, taps = d.forward_tapped(x, raster=True, rois_per_image=groups)
            assert d.spike_rates is False
            _check_det_taps(taps, s6, s7, groups, Hd, T, raster=True)
            assert torch.equal(taps["pass"]["spk6_count"], c6_want) and torch.equal(taps["pass"]["spk7_count"], c7_want)
            assert torch.equal(taps["lif6"]["per_roi"], c6_want) and torch.equal(taps["lif7"]["per_roi"], c7_want)        # 2
            for got, ref in zip(taps_mod.det_rate_list(taps), rates_want):
                assert torch.equal(got, ref)
            assert cls.shape == cls_plain.shape and bbox.shape == bbox_plain.shape
            for name in ("lif6", "lif7"):
                t = taps[name]
                assert int(t["per_step"].sum()) == int(t["per_channel"].sum()) == int(t["per_roi"].sum())
        v6, v7 = taps_mod.det_planes_views(R, DET_C * 49, Hd, 9, 36, T, d._params(), d.fc6_inner())
        assert int(v7.layout) == TP.ROWS
        layouts.add(int(v6.layout))


@pytest.mark.parametrize("Hd", DET_HD)
def test_det_taps_equal_the_planes_and_the_pass_counts(gpu_device, Hd):
    layouts = set()
    _run_det_grid(gpu_device, [(Hd, T, R, "bf16x3") for T in DET_T for R in DET_R], layouts)
    assert layouts == {TP.WORD_MAJOR}


def test_det_lif6_layouts_rows_and_word_major(gpu_device):
    """the grid above keeps lif6 word-major (the fused bf16x3 layers); tests/_entry_cases.py's det(29, 64, 12, precision="f32") keeps rows"""
    layouts = set()
    _run_det_grid(gpu_device, [(128, 12, 29, "f32"), (128, 12, 29, "bf16x3")], layouts)
    assert layouts == {TP.ROWS, TP.WORD_MAJOR}, "lif6 must be seen as rows and word-major, saw %s" % sorted(layouts)


# ---- 3: the raster equals the oracle's spike train on dyadic grids ---------------------------------------------------------------------
def test_rpn_raster_equals_the_oracle_trace(gpu_device):
    S, _, _, _ = _pkg()
    case = G.rpn_t_case(64, 8)
    m = S.RPNHeadSNN(case["C"], case["A"], case["T"]).to(gpu_device)
    m.load_state_dict({"shared_conv.weight": case["w_shared"], "conv_cls.weight": case["w_cls"], "conv_bbox.weight": case["w_bbox"]})
    _, _, taps = m.forward_tapped([f.to(gpu_device) for f in case["feats"]], raster=True)
    for l, tr in enumerate(case["traces"]):
        want = tr["spk"].bool()
        got = taps["shared_lif"][l]["raster"].cpu()
        assert got.shape == want.shape and torch.equal(got, want), "level %d: %d spikes differ" % (l, int((got != want).sum()))
        assert np.array_equal(_np(taps["shared_lif"][l]["per_step"]).sum(1), case["counts"][l])


def test_det_raster_equals_the_oracle_trace(gpu_device):
    S, _, _, _ = _pkg()
    case = G.det_t_case(12)
    d = S.FastRCNNPredictorSNNFull(case["C"] * 49, case["Hd"], case["K"], case["T"]).to(gpu_device)
    d.load_state_dict({"fc6.weight": case["w6"], "fc7.weight": case["w7"], "cls_score.weight": case["w_cls"], "bbox_pred.weight": case["w_bbox"]})
    _, _, taps = d.forward_tapped(case["x"].to(gpu_device), raster=True)
    for name, key in (("lif6", "spk6"), ("lif7", "spk7")):
        want = case["trace"][key].bool()
        got = taps[name]["raster"].cpu()
        assert got.shape == want.shape and torch.equal(got, want), "%s: %d spikes differ" % (name, int((got != want).sum()))
    assert np.array_equal(_np(taps["lif6"]["per_roi"]), case["counts"][0]) and np.array_equal(_np(taps["lif7"]["per_roi"]), case["counts"][1])


# ---- 4: any-time ------------------------------------------------------------------------------------------------------------------------
def test_cumulative_per_step_equals_the_readout_counts(gpu_device):
    _, _, ops, _ = _pkg()
    steps = [3, 5, 8]
    N, shapes = RPN_PYRAMIDS[0]
    m = _rpn_head(128, 8, gpu_device)
    feats = _rpn_feats(N, shapes, 128, gpu_device, seed=3)
    C_, A, p, w_shared, w_heads = m._pass_args()
    _, _, _, (counts, _, _, _) = ops.rpn_head_forward_readouts(feats, C_, A, steps, p, w_shared, w_heads, spike_rates=True)
    _, _, taps = m.forward_tapped(feats)
    for l in range(len(shapes)):
        cum = taps["shared_lif"][l]["per_step"].cumsum(1)                    # [N, T]
        for j, T_ in enumerate(steps):
            assert torch.equal(cum[:, T_ - 1], counts[j, l, :N]), (l, T_)
    d = _det_head(128, 8, gpu_device)
    x = _det_x(17, gpu_device, seed=4)
    args = d._pass_args(x.flatten(1).shape[1], "")
    args["spike_rates"] = True
    _, _, (c6, c7, _, _) = ops.det_head_forward_readouts(x, steps=steps, **args)
    _, _, taps = d.forward_tapped(x, raster=True)
    for name, c in (("lif6", c6), ("lif7", c7)):
        cum = taps[name]["raster"].sum(2, dtype=torch.int64).cumsum(0)       # [T, R]: spikes of RoI r in the steps <= t
        for j, T_ in enumerate(steps):
            assert torch.equal(cum[T_ - 1], c[j].to(torch.int64)), (name, T_)
        assert torch.equal(taps[name]["per_step"][0].cumsum(0)[[t - 1 for t in steps]], c.to(torch.int64).sum(1))


# ---- 5: steps_formed ---------------------------------------------------------------------------------------------------------------------
def test_a_plain_pass_leaves_lif6_last_step_unformed(gpu_device):
    _, _lib, ops, taps_mod = _pkg()
    lib = _lib.load()
    Hd, T, R = 128, 12, 17
    d = _det_head(Hd, T, gpu_device)
    x = _det_x(R, gpu_device, seed=5)
    _, _, tapped = d.forward_tapped(x, raster=True)
    path_rates = lib.snn_debug_last_fc6_path()
    d(x)                                                                     # a plain forward: lif6's plane of step T - 1 reaches nothing
    path_plain = lib.snn_debug_last_fc6_path()
    v6, _ = taps_mod.det_planes_views(R, DET_C * 49, Hd, 9, 36, T, d._params(), d.fc6_inner(), spike_rates=False)
    assert v6.steps_formed == T - 1
    ws = ops._WS.get(gpu_device, 1)
    out = torch.empty((T, R, Hd), dtype=torch.uint8, device=gpu_device)
    rc = lib.snn_planes_raster_rows(ops._ptr(ws), C.byref(v6), Hd, T, ops._ptr(out), ops._stream())
    assert rc == -1 and b"forms 11" in lib.snn_last_error()
    rc = lib.snn_planes_counts(ops._ptr(ws), C.byref(v6), (C.c_int64 * 2)(0, R), 1, Hd, T, None, None, None, ops._stream())
    assert rc == -1
    got = taps_mod.planes_raster_rows(ws, v6, Hd, T - 1)
    if path_plain != path_rates:
        pytest.skip("fc6 took launch %d in the plain pass and %d in spike-rate mode: their planes may differ at threshold ties" % (path_plain, path_rates))
    assert torch.equal(got, tapped["lif6"]["raster"][:T - 1])


# ---- 6: model level ------------------------------------------------------------------------------------------------------------------------
def test_model_forward_tapped_gives_detections_and_the_energy_rates(gpu_device):
    from collections import OrderedDict

    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import energy
    from snn_automotive_object_detection_amd.stock.transform import GeneralizedRCNNTransform
    from tests.test_gpu_static import LEVELS, NAMES
    torch.manual_seed(1234)
    model = S.create_model("cityscapes", 9, True, True, 0, False, False, num_steps_rpn=8, num_steps_detector=12).eval()
    model.rpn.to(gpu_device)
    model.roi_heads.to(gpu_device)
    with torch.no_grad():
        model.rpn.head.shared_conv.weight.mul_(5.0)
    model.roi_heads.score_thresh = 0.05
    model.rpn._post_nms_top_n = dict(training=40, testing=40)
    model.transform = GeneralizedRCNNTransform(128, 256, model.transform.image_mean, model.transform.image_std)
    g = torch.Generator().manual_seed(21)
    feats = OrderedDict((n, (2 * torch.randn((2, 256, h, w), generator=g)).to(gpu_device)) for n, (h, w) in zip(NAMES, LEVELS))

    class Computed(torch.nn.Module):                                          # the small pyramid of tests/test_gpu_static.py in place of the backbone
        def forward(self, x):
            return OrderedDict(feats)
    model.backbone = Computed()
    imgs = [torch.rand((3, 128, 256), generator=g).to(gpu_device) for _ in range(2)]
    want = model(imgs)
    dets, taps = model.forward_tapped(imgs)
    assert model.rpn.head.spike_rates is False and model.roi_heads.box_head_and_predictor.spike_rates is False
    assert len(dets) == len(want) == 2 and sum(int(w_["boxes"].shape[0]) for w_ in want) > 0
    for g_, w_ in zip(dets, want):
        assert list(g_) == list(w_)
        for k in w_:
            assert g_[k].dtype == w_[k].dtype and g_[k].shape == w_[k].shape, k
    ref = energy.extract_spike_rates(model, [imgs])
    got = energy.rates_from_taps(taps)
    assert sorted(got) == sorted(ref) == list(range(19))
    for k in ref:
        assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), k
    assert energy.energy_report(got, 8, 12) == energy.energy_report(ref, 8, 12)
    assert len(taps["rpn"]["shared_lif"]) == 5 and taps["det"]["lif6"]["per_step"].shape[0] == 2


# ---- 7: scratch independence -----------------------------------------------------------------------------------------------------------------
def _fill_outside(ws, views, T, byte=0xff):
    """every workspace byte outside the views' T steps <- byte"""
    keep = torch.zeros(ws.numel(), dtype=torch.bool, device=ws.device)
    for v in views:
        f = TP.view_fields(v)
        keep[f["offset"]: f["offset"] + T * f["stride"] * 4] = True
    ws[~keep] = byte


def test_taps_do_not_depend_on_scratch_or_output_contents(gpu_device, monkeypatch):
    _, _, ops, taps_mod = _pkg()
    N, shapes, C_, T = 2, RPN_PYRAMIDS[0][1], 256, 8
    m = _rpn_head(C_, T, gpu_device)
    feats = _rpn_feats(N, shapes, C_, gpu_device, seed=7)
    _, _, taps = m.forward_tapped(feats, raster=True)
    ws = ops._WS.get(gpu_device, 1)
    v = taps_mod.rpn_planes_view([(N, h, w) for h, w in shapes], C_, 3, T, m._params())
    _fill_outside(ws, [v], T)
    real_empty = torch.empty

    def ones(*a, **k):
        t = real_empty(*a, **k)
        t.view(torch.uint8).fill_(0xff) if t.numel() else None
        return t
    groups = [h * w for h, w in shapes for _ in range(N)]
    with monkeypatch.context() as mp:
        mp.setattr(torch, "empty", ones)
        per_step, per_col, per_row = taps_mod.planes_counts(ws, v, groups, C_, T)
        r0 = taps_mod.planes_raster_nchw(ws, v, 0, N, C_, 5, 7, T)
    assert torch.equal(per_step[:, :N].t(), taps["shared_lif"][0]["per_step"]) and torch.equal(per_col[N:], taps["shared_lif"][1]["per_channel"])
    assert torch.equal(per_row[:N * 35].view(N, 5, 7), taps["shared_lif"][0]["per_position"]) and torch.equal(r0, taps["shared_lif"][0]["raster"])

    d = _det_head(72, 12, gpu_device)
    x = _det_x(17, gpu_device, seed=8)
    _, _, taps = d.forward_tapped(x, raster=True, rois_per_image=[16, 1])
    ws = ops._WS.get(gpu_device, 1)
    v6, v7 = taps_mod.det_planes_views(17, DET_C * 49, 72, 9, 36, 12, d._params(), d.fc6_inner())
    _fill_outside(ws, [v6, v7], 12)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "empty", ones)
        got = {n: (taps_mod.planes_counts(ws, v_, [16, 1], 72, 12), taps_mod.planes_raster_rows(ws, v_, 72, 12)) for n, v_ in (("lif6", v6), ("lif7", v7))}
    for n, ((per_step, per_col, per_row), raster) in got.items():
        assert torch.equal(per_step.t(), taps[n]["per_step"]) and torch.equal(per_col, taps[n]["per_channel"])
        assert torch.equal(per_row, taps[n]["per_roi"]) and torch.equal(raster, taps[n]["raster"])


# ---- 8: capture ------------------------------------------------------------------------------------------------------------------------------
def test_counts_and_raster_replay_in_a_graph_on_new_planes(gpu_device):
    """snn_planes_counts and both raster calls in ONE single-stream torch.cuda.graph over hand-made plane sets (all three layouts): every
    replay equals the eager call on the same contents"""
    _, _lib, ops, taps_mod = _pkg()
    lib = _lib.load()
    T, rows, words, n_cols = 5, 94, 8, 250
    N, H, W = 2, 5, 7                                                        # rows 0 .. 69 as one level of the NCHW raster
    rng = np.random.default_rng(11)
    sets = [torch.from_numpy(rng.integers(0, 2 ** 32, size=8 + T * (rows * words + 2), dtype=np.uint64).astype(np.uint32).view(np.int32)) for _ in range(2)]
    for layout in TP.LAYOUTS:
        v = _lib.snn_planes_view(32, rows * words + 2, rows, words, layout, T, 0)
        ws = torch.zeros((T * (rows * words + 2) + 8 + 64) * 4, dtype=torch.uint8, device=gpu_device)
        per_step = torch.empty((T, 3), dtype=torch.int64, device=gpu_device)
        per_col = torch.empty((3, n_cols), dtype=torch.int32, device=gpu_device)
        per_row = torch.empty((rows,), dtype=torch.int32, device=gpu_device)
        r_rows = torch.empty((T, rows, n_cols), dtype=torch.uint8, device=gpu_device)
        r_nchw = torch.empty((T, N, n_cols, H, W), dtype=torch.uint8, device=gpu_device)
        starts = (C.c_int64 * 4)(0, 35, 70, 94)

        def enqueue():
            s = torch.cuda.current_stream().cuda_stream
            assert lib.snn_planes_counts(ops._ptr(ws), C.byref(v), starts, 3, n_cols, T, ops._ptr(per_step), ops._ptr(per_col), ops._ptr(per_row), s) == 0
            assert lib.snn_planes_raster_rows(ops._ptr(ws), C.byref(v), n_cols, T, ops._ptr(r_rows), s) == 0
            assert lib.snn_planes_raster_nchw(ops._ptr(ws), C.byref(v), 0, N, n_cols, H, W, T, ops._ptr(r_nchw), s) == 0

        def load(words_cpu):
            ws.view(torch.int32)[:words_cpu.numel()].copy_(words_cpu)

        outs = (per_step, per_col, per_row, r_rows, r_nchw)
        load(sets[0])
        enqueue()                                                            # eager once before the capture (the capture contract)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                enqueue()
        torch.cuda.current_stream().wait_stream(side)
        for words_cpu in (sets[1], sets[0]):
            load(words_cpu)
            for o in outs:
                o.view(torch.uint8).fill_(0xff)
            graph.replay()
            torch.cuda.synchronize()
            replayed = [o.clone() for o in outs]
            for o in outs:
                o.view(torch.uint8).fill_(0xff)
            enqueue()
            torch.cuda.synchronize()
            for a, b in zip(replayed, outs):
                assert torch.equal(a, b)
            # ... and both equal the numpy reading of what was loaded
            spk = TP.dense(TP.rows_from_layout(words_cpu.numpy().view(np.uint32)[8:], T, rows, words, layout, rows * words + 2), n_cols)
            e_step, e_col, e_row = TP.expected_counts(spk, [35, 35, 24])
            assert np.array_equal(_np(per_step), e_step) and np.array_equal(_np(per_col), e_col) and np.array_equal(_np(per_row), e_row)
            assert np.array_equal(r_rows.cpu().numpy().astype(bool), spk)
            assert np.array_equal(r_nchw.cpu().numpy().astype(bool), spk[:, :70].reshape(T, N, H, W, n_cols).transpose(0, 1, 4, 2, 3))
        del graph
