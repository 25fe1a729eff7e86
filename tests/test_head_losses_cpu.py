"""Target matching and head losses without a GPU: argument validation and limits of snn_match_targets, snn_rpn_loss_grad and
snn_det_loss_grad (return codes and snn_last_error, before any device work), monotone size queries, the sampler's properties, the Python
shape errors, and the restatements of tests/_head_losses.py against the fixtures of the reference's own bodies."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _head_losses as HL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    from snn_automotive_object_detection_amd import _lib
    return _lib, _lib.load()


def _err(lib):
    return lib.snn_last_error().decode()


P = C.c_void_p(4096)                             # a non-null, aligned address nothing ever reads: every call below fails before device work
ODD = C.c_void_p(4100)


def _match(lib, bs, gs, N, high=0.7, low=0.3, lq=1, boxes=P, gt=P, w=True, scratch=P, nbytes=1 << 30):
    return lib.snn_match_targets(boxes, (C.c_int64 * len(bs))(*bs) if bs is not None else None, gt, None, (C.c_int64 * len(gs))(*gs) if gs is not None else None,
                                 N, high, low, lq, (C.c_float * 4)(1, 1, 1, 1) if w else None, P, P, P, scratch, nbytes, None)


def test_match_targets_arguments_and_limits():
    _, lib = _lib()
    assert _match(lib, None, [0, 1], 1) == -1 and "null" in _err(lib)
    assert _match(lib, [0, 5], [0, 1], 1, w=False) == -1
    assert _match(lib, [0, 5], [0, 1], 0) == -1 and "N = 0" in _err(lib)
    assert _match(lib, [0] * 66, [0] * 66, 65) == -4 and "65 images" in _err(lib)
    assert _match(lib, [0, 5], [0, 257], 1) == -4 and "257 ground-truth boxes" in _err(lib)
    assert _match(lib, [0, 5, 9], [0, 256, 513], 2) == -4 and "image 1" in _err(lib)
    assert _match(lib, [0, 5, 3], [0, 1, 2], 2) == -1 and "decrease" in _err(lib)
    assert _match(lib, [1, 5], [0, 1], 1) == -1 and "must be 0" in _err(lib)
    assert _match(lib, [0, 1 << 31], [0, 1], 1) == -4 and "2^31" in _err(lib)
    assert _match(lib, [0, 5], [0, 1], 1, lq=2) == -1 and "allow_low_quality" in _err(lib)
    assert _match(lib, [0, 5], [0, 1], 1, boxes=None) == -1
    assert _match(lib, [0, 5], [0, 1], 1, gt=None) == -1
    assert _match(lib, [0, 5], [0, 1], 1, boxes=ODD) == -1 and "aligned" in _err(lib)
    assert _match(lib, [0, 5], [0, 1], 1, scratch=None) == -1 and "scratch" in _err(lib)
    assert _match(lib, [0, 5], [0, 1], 1, nbytes=16) == -1 and "scratch" in _err(lib)
    assert _match(lib, [0, 0], [0, 0], 1, boxes=None, gt=None, scratch=None, nbytes=0) == 0          # no boxes: nothing to do


def _rpn(lib, levels, A, N, n_levels=None, deltas=P, scratch=P, nbytes=1 << 30, logits=P):
    from snn_automotive_object_detection_amd._lib import snn_rpn_level
    lv = (snn_rpn_level * max(1, len(levels)))(*[snn_rpn_level(None, n, h, w, 0) for n, h, w in levels])
    return lib.snn_rpn_loss_grad(lv, len(levels) if n_levels is None else n_levels, A, N, logits, deltas, P, P, P, P, P, P, scratch, nbytes, None)


def test_rpn_loss_grad_arguments_and_limits():
    _, lib = _lib()
    lv = [(2, 5, 7), (2, 3, 4)]
    assert _rpn(lib, lv, 3, 2, logits=None) == -1 and "null" in _err(lib)
    assert _rpn(lib, lv, 0, 2) == -1 and _rpn(lib, lv, 3, 0) == -1 and _rpn(lib, lv, 3, 2, n_levels=0) == -1
    assert _rpn(lib, [(2, 1, 1)] * 9, 3, 2) == -4 and "9 levels" in _err(lib)
    assert _rpn(lib, lv, 65, 2) == -4 and "A = 65" in _err(lib)
    assert _rpn(lib, [(2, 5, 7), (1, 3, 4)], 3, 2) == -1 and "level 1" in _err(lib)
    assert _rpn(lib, [(2, 0, 7)], 3, 2) == -1
    assert _rpn(lib, [(2, 32768, 32768)], 3, 2) == -4 and "2^31" in _err(lib)
    assert _rpn(lib, lv, 3, 2, deltas=ODD) == -1 and "aligned" in _err(lib)
    assert _rpn(lib, lv, 3, 2, scratch=None) == -1 and _rpn(lib, lv, 3, 2, nbytes=64) == -1 and "scratch" in _err(lib)


def _det(lib, R, K, K4=None, logits=P, scratch=P, nbytes=1 << 30):
    return lib.snn_det_loss_grad(logits, P, P, P, R, K, 4 * K if K4 is None else K4, P, P, P, scratch, nbytes, None)


def test_det_loss_grad_arguments_and_limits():
    _, lib = _lib()
    assert _det(lib, 5, 9, logits=None) == -1 and "null" in _err(lib)
    assert _det(lib, 0, 9) == -1 and _det(lib, 5, 1) == -1
    assert _det(lib, 5, 9, K4=4) == -1 and "K4 = 4" in _err(lib)                                    # (an only_one_bbox head)
    assert _det(lib, 5, 257) == -4 and "K = 257" in _err(lib)
    assert _det(lib, 1 << 22, 256) == -4 and "2^31" in _err(lib)
    assert _det(lib, 5, 9, logits=ODD) == -1 and "aligned" in _err(lib)
    assert _det(lib, 5, 9, scratch=None) == -1 and _det(lib, 5, 9, nbytes=64) == -1 and "scratch" in _err(lib)


def test_size_queries_are_monotone_and_zero_outside_the_limits():
    _, lib = _lib()
    m, r, d = lib.snn_match_targets_workspace_bytes, lib.snn_rpn_loss_grad_workspace_bytes, lib.snn_det_loss_grad_workspace_bytes
    assert m(0, 0) == 0 and m(10, 65) == 0 and m(-1, 1) == 0 and m(1 << 31, 1) == 0 and m(0, 1) > 0
    totals, Ns = [0, 1, 255, 256, 257, 1031, 294624, 2 * 294624, (1 << 31) - 1], [1, 2, 3, 64]
    for N in Ns:
        sizes = [m(t, N) for t in totals]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for t in totals:
        sizes = [m(t, N) for N in Ns]
        assert sizes == sorted(sizes)
    # the scratch holds a maximum per ground-truth box of every work-group and of every image
    assert m(2 * 294624, 2) >= ((2 * 294624 + 255) // 256 + 2 + 2) * 256 * 4 - 2 * 1024
    assert r(0) == 0 and r(1 << 31) == 0
    sizes = [r(a) for a in [1, 255, 256, 257, 294, 589248, (1 << 31) - 1]]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert d(0, 9) == 0 and d(5, 1) == 0 and d(5, 257) == 0 and d(1 << 22, 256) == 0
    for K in (2, 9, 91, 256):
        sizes = [d(R, K) for R in (1, 15, 16, 17, 513, 1024, 100000)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for R in (1, 513):
        sizes = [d(R, K) for K in (2, 9, 91, 256)]
        assert sizes == sorted(sizes)


def test_every_new_symbol_is_bound():
    L, lib = _lib()
    for name in ("snn_match_targets", "snn_rpn_loss_grad", "snn_det_loss_grad"):
        assert name in L.SYMBOLS and name + "_workspace_bytes" in L.SYMBOLS and hasattr(lib, name)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,frac", [(8, 0.25), (64, 0.5), (7, 0.5), (512, 0.25)])
def test_sampler_properties(batch, frac):
    from snn_automotive_object_detection_amd import losses
    g = torch.Generator().manual_seed(batch)
    labels = [torch.randint(-1, 4, (n,), generator=g) for n in (300, 5, 40)] + [torch.full((20,), -1), torch.zeros(30, dtype=torch.int64)]
    s = losses.BalancedPositiveNegativeSampler(batch, frac)
    pos, neg = s(labels, torch.Generator().manual_seed(3))
    pos2, neg2 = s(labels, torch.Generator().manual_seed(3))
    pos3, _ = s(labels, torch.Generator().manual_seed(4))
    for lab, p, n, p2, n2 in zip(labels, pos, neg, pos2, neg2):
        assert p.dtype == torch.uint8 and p.shape == lab.shape and torch.equal(p, p2) and torch.equal(n, n2)
        assert bool((lab[p.bool()] >= 1).all()) and bool((lab[n.bool()] == 0).all()) and not bool((p & n).any())
        n_pos, n_neg = int(p.sum()), int(n.sum())
        want_pos = min(int((lab >= 1).sum()), int(batch * frac))
        assert n_pos == want_pos and n_neg == min(int((lab == 0).sum()), batch - want_pos) and n_pos + n_neg <= batch
    assert not torch.equal(pos[0], pos3[0]), "another generator, another sample"
    float_pos, _ = s([labels[0].float()], torch.Generator().manual_seed(3))                          # (the RPN's labels are float32)
    assert torch.equal(float_pos[0], pos[0])


# ---- Python shape errors -------------------------------------------------------------------------------------------------------------------------
def test_python_shape_errors():
    from snn_automotive_object_detection_amd import losses
    b, g = torch.zeros((5, 4)), torch.zeros((2, 4))
    with pytest.raises(ValueError, match="n, 4"):
        losses.match_targets([torch.zeros((5, 3))], [g], None, 0.7, 0.3, True)
    with pytest.raises(ValueError, match="per image"):
        losses.match_targets([b, b], [g], None, 0.7, 0.3, True)
    with pytest.raises(ValueError, match="per image"):
        losses.match_targets([b], [g], [torch.zeros(2, dtype=torch.int64)] * 2, 0.5, 0.5, False)
    assert losses.match_targets([], [], None, 0.7, 0.3, True) == ([], [], [])
    obj, dl = [torch.zeros((2, 3, 4, 5))], [torch.zeros((2, 12, 4, 5))]
    lab, tg, sm = torch.zeros(120), torch.zeros((120, 4)), torch.zeros(120, dtype=torch.uint8)
    with pytest.raises(ValueError, match="per level"):
        losses.rpn_loss(obj, dl + dl, lab, tg, sm)
    with pytest.raises(ValueError, match="a level is"):
        losses.rpn_loss(obj, [torch.zeros((2, 8, 4, 5))], lab, tg, sm)
    with pytest.raises(ValueError, match="120 anchors"):
        losses.rpn_loss(obj, dl, lab[:100], tg, sm)
    with pytest.raises(ValueError, match="R, K"):
        losses.fastrcnn_loss(torch.zeros((5, 9)), torch.zeros((4, 36)), torch.zeros(5), torch.zeros((5, 4)))
    with pytest.raises(ValueError, match="5 rows"):
        losses.fastrcnn_loss(torch.zeros((5, 9)), torch.zeros((5, 36)), torch.zeros(4), torch.zeros((5, 4)))
    from snn_automotive_object_detection_amd._lib import SnnHipError
    with pytest.raises(SnnHipError, match="GPU"):                                                      # (no CPU fallback)
        losses.fastrcnn_loss(torch.zeros((5, 9)), torch.zeros((5, 36)), torch.zeros(5), torch.zeros((5, 4)))


def test_readout_losses_refusals_and_target_checks():
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd.model import _default_anchorgen
    rpn = S.RegionProposalNetwork(_default_anchorgen(), S.RPNHeadSNN(32, 3, 4), 0.7, 0.3, 256, 0.5, dict(training=20, testing=10),
                                  dict(training=30, testing=15), 0.7).eval()
    roi = S.RoIHeadsSNN(None, S.FastRCNNPredictorSNNFull(32 * 49, 64, 5, 4), 0.5, 0.5, 512, 0.25, None, 0.05, 0.5, 10).eval()
    assert (rpn.fg_iou_thresh, rpn.bg_iou_thresh, rpn.batch_size_per_image, rpn.positive_fraction) == (0.7, 0.3, 256, 0.5)
    assert (roi.fg_iou_thresh, roi.bg_iou_thresh, roi.batch_size_per_image, roi.positive_fraction) == (0.5, 0.5, 512, 0.25)
    assert tuple(roi.box_coder.weights) == (10.0, 10.0, 5.0, 5.0) and tuple(rpn.box_coder.weights) == (1.0, 1.0, 1.0, 1.0)
    assert rpn._top_n("training") == (20, 30) and rpn._top_n("testing") == (10, 15) and rpn._top_n() == (10, 15) and rpn._top_n((3, 4)) == (3, 4)
    model = S.GeneralizedRCNN(torch.nn.Identity(), rpn, roi, torch.nn.Identity()).eval()
    images = [torch.zeros((3, 8, 8))]
    good = [{"boxes": torch.zeros((1, 4)), "labels": torch.zeros(1, dtype=torch.int64)}]
    with pytest.raises(ValueError, match="None"):
        model.readout_losses(images, None)
    with pytest.raises(ValueError, match="labels key"):
        model.readout_losses(images, [{"boxes": torch.zeros((1, 4))}])
    with pytest.raises(TypeError, match="float"):
        model.readout_losses(images, [{"boxes": torch.zeros((1, 4), dtype=torch.int64), "labels": good[0]["labels"]}])
    with pytest.raises(TypeError, match="int64"):
        model.readout_losses(images, [{"boxes": torch.zeros((1, 4)), "labels": torch.zeros(1, dtype=torch.int32)}])
    with pytest.raises(ValueError, match=r"\[N, 4\]"):
        model.readout_losses(images, [{"boxes": torch.zeros((4,)), "labels": good[0]["labels"]}])
    model.train()
    with pytest.raises(NotImplementedError):
        model.readout_losses(images, good)
    with pytest.raises(NotImplementedError):
        model(images)
    with pytest.raises(NotImplementedError):
        rpn.head_losses(None, {}, good)
    with pytest.raises(NotImplementedError):
        roi.head_losses({}, [], [], good)


# ---- the restatements against the reference's own bodies ----------------------------------------------------------------------------------------
def _npz(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def test_grid_facts_hold_in_fp32():
    assert all(HL.grid_facts())
    b, g, _ = HL.grid_image()
    iou = HL.box_iou(g, b)
    assert iou[0, 0] == np.float32(0.7) and iou[0, 1] == np.float32(0.3) and iou[0, 2] == 0.5 and iou[2, 4] == 0.5 and not bool(iou[3].any())
    assert torch.equal(iou[0], iou[1]) and not bool(torch.isnan(iou).any())


@pytest.mark.parametrize("name", ["pyr_a3", "one_level"])
def test_rpn_restatements_equal_the_reference_fixture(name):
    from snn_automotive_object_detection_amd import losses
    z = _npz("loss_rpn_%s.npz" % name)
    N, A, shapes = int(z["N"]), int(z["A"]), [tuple(s) for s in z["shapes"].tolist()]
    per = z["anchors"].shape[0]
    for n, g in enumerate(z["gt_boxes"].split(z["gt_counts"].tolist())):
        idx, lab = HL.match(z["anchors"], g, None, 0.7, 0.3, True)
        assert torch.equal(lab.float(), z["labels"][n * per:(n + 1) * per]), "the restated labels are not assign_targets_to_anchors'"
        i2, l2, t2 = losses._match_stock(z["anchors"], g, None, 0.7, 0.3, True, (1.0, 1.0, 1.0, 1.0))      # (the package's stock path)
        assert torch.equal(i2, idx) and torch.equal(l2, lab) and torch.equal(t2, z["targets32"][n * per:(n + 1) * per])
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        o = HL.head_rows_to_ref(z["logits"].to(dt), shapes, N, 1).reshape(-1)
        d = HL.head_rows_to_ref(z["deltas"].to(dt), shapes, N, 4)
        (l0, l1), (g_o, g_d), _ = HL.with_grads(HL.rpn_loss, o, d, z["labels"].to(dt), z["targets" + tag].to(dt), z["sampled"].bool())
        assert torch.equal(torch.stack((l0, l1)), z["loss" + tag]), "the restated loss is not compute_loss'"
        assert torch.equal(HL.ref_to_head_rows(g_o.reshape(-1, 1), shapes, N, A, 1), z["g_logits" + tag])
        assert torch.equal(HL.ref_to_head_rows(g_d, shapes, N, A, 4), z["g_deltas" + tag])


@pytest.mark.parametrize("name", ["k9", "k11_bg"])
def test_det_restatements_equal_the_reference_fixture(name):
    z = _npz("loss_det_%s.npz" % name)
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        (l0, l1), (g_l, g_b), _ = HL.with_grads(HL.det_loss, z["logits"].to(dt), z["box"].to(dt), z["labels"], z["targets" + tag].to(dt))
        assert torch.equal(torch.stack((l0, l1)), z["loss" + tag]) and torch.equal(g_l, z["g_logits" + tag]) and torch.equal(g_b, z["g_box" + tag])
    bc, gc = z["box_counts"].tolist(), z["gt_counts"].tolist()
    for p, g, gl, want in zip(z["proposals"].split(bc), z["gt_boxes"].split(gc), z["gt_labels"].split(gc), z["labels_all"].split(bc)):
        assert torch.equal(HL.match(p, g, gl, 0.5, 0.5, False)[1], want), "the restated labels are not assign_targets_to_proposals'"
