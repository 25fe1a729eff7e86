"""The post-processing kernels (csrc/snn_post.h: radix top-k, box decode, NMS bit-matrix and walk, rank merges, detection lists) on the
exactly decodable grids of tests/_post_grid.py.  Every decoded box is exact in fp32 and every pair of scores that meets anywhere is
equal by construction or 1e-4 apart, so the expectation (the oracle restatement, stable top-k) is matched with ZERO tolerance on the
row count, the order, every box, every label and the zero rows behind the counts; SCORE_ATOL covers the VALUE of a score alone (device
expf against torch's exp).  tests/test_post_grid_cpu.py proves on the host that each planted decision (IoU equal to the threshold, a
tie across lists, a cut inside a tie group) changes these expectations when it is taken the wrong way."""
import numpy as np
import pytest
import torch

from oracle import torchvision_restated as TV
from tests import _post_grid as G
from tests._util import SCORE_ATOL
from tests.test_post_golden import StoredHead

pytestmark = pytest.mark.gpu


def _close_scores(got, exp, what):
    got, exp = got.detach().cpu().double(), exp.double()
    assert got.shape == exp.shape, what
    if got.numel():
        assert float((got - exp).abs().max()) <= SCORE_ATOL, "%s: scores differ by %g" % (what, float((got - exp).abs().max()))


# ---- NMS, called directly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", G.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", G.NMS_SIZES)
def test_hip_nms_on_planted_threshold_pairs(gpu_device, n, thr):
    """integer boxes with pairs whose IoU is exactly the threshold (and the nearest ratios on either side), suppressor and victim on
    bits 0 / 31 / 32 / 63 of one mask word and of adjacent words, 1 and 3 categories: the kept indices are torchvision's"""
    from snn_automotive_object_detection_amd import ops
    for ncat in (1, 3):
        for layout in range(G.NMS_LAYOUTS):
            c = G.nms_case(n, thr, ncat, layout)
            what = "n=%d thr=%g ncat=%d layout=%d" % (n, thr, ncat, layout)
            exp = TV.batched_nms(c["boxes"], c["scores"], c["idxs"], thr)
            b, s, i = c["boxes"].to(gpu_device), c["scores"].to(gpu_device), c["idxs"].to(gpu_device)
            assert torch.equal(ops.batched_nms(b, s, i, thr).cpu(), exp), what
            if ncat == 1:
                assert torch.equal(ops.batched_nms(b, s, None, thr).cpu(), TV.nms(c["boxes"], c["scores"], thr)), what
            order, kept = ops.nms_keep_mask(b, s, i, thr)
            assert torch.equal(order[kept].cpu(), exp), what + " (keep mask)"
            for mk in (1, 64, 65):
                assert torch.equal(ops.batched_nms(b, s, i, thr, max_keep=mk).cpu(), exp[:mk]), what + " max_keep=%d" % mk


# ---- RPN -----------------------------------------------------------------------------------------------------------------------------
def _rpn_direct(spec, dev):
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd.stock.anchors import AnchorGenerator
    lg, de, hw, strides = G.rpn_device_inputs(spec, dev)
    ag = AnchorGenerator(spec["geo"]["sizes"], spec["geo"]["ratios"])
    return ops.rpn_proposals(lg, de, hw, strides, ag.cell_anchors, spec["image_sizes"], spec["pre"], spec["post"], spec["nms"],
                             spec["score_thresh"], spec["min_size"])


@pytest.mark.parametrize("name", sorted(G.RPN_SPECS))
def test_hip_rpn_proposals_on_exact_grids(gpu_device, name):
    """ops.rpn_proposals == the oracle with the stable top-k: counts, proposals bit for bit in exact order, zero rows behind the counts,
    the pre-NMS report bit for bit; score values within SCORE_ATOL"""
    spec = G.rpn_spec(name)
    e_b, e_s, e_pre = spec["expected"]
    boxes, scores, counts, pre_b, pre_p = _rpn_direct(spec, gpu_device)
    assert boxes.shape == (spec["N"], spec["post"], 4) and scores.shape == (spec["N"], spec["post"])
    assert counts.cpu().tolist() == [int(b.shape[0]) for b in e_b]
    for i in range(spec["N"]):
        c = int(e_b[i].shape[0])
        assert torch.equal(boxes[i, :c].cpu(), e_b[i]), "%s image %d: proposals" % (name, i)
        _close_scores(scores[i, :c], e_s[i], "%s image %d" % (name, i))
        assert not bool(boxes[i, c:].any()) and not bool(scores[i, c:].any()), "%s image %d: rows behind the count" % (name, i)
        assert torch.equal(pre_b[i].cpu(), e_pre[i]["proposals"]), "%s image %d: pre-NMS boxes" % (name, i)
        _close_scores(pre_p[i], e_pre[i]["objectness"], "%s image %d pre-NMS" % (name, i))


def test_hip_rpn_module_equals_the_direct_call(gpu_device):
    """one spec through RegionProposalNetwork with a stored head: bit-equal to ops.rpn_proposals on the same tensors"""
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd.stock.anchors import AnchorGenerator, ImageList
    spec = G.rpn_spec(G.RPN_WRAPPED)
    geo, N = spec["geo"], spec["N"]
    head = StoredHead([o.to(gpu_device) for o in spec["obj"]], [d.to(gpu_device) for d in spec["dl"]])
    rpn = S.RegionProposalNetwork(AnchorGenerator(geo["sizes"], geo["ratios"]), head, 0.7, 0.3, 256, 0.5,
                                  dict(training=2000, testing=spec["pre"]), dict(training=2000, testing=spec["post"]), spec["nms"],
                                  score_thresh=spec["score_thresh"]).eval()
    rpn.min_size = spec["min_size"]
    assert rpn.post == "hip"
    images = ImageList(torch.zeros((N, 3) + tuple(geo["canvas"]), device=gpu_device), list(spec["image_sizes"]))
    feats = {str(l): torch.zeros((N, 1) + tuple(g), device=gpu_device) for l, g in enumerate(geo["grids"])}
    got, pre = rpn(images, feats)
    boxes, scores, counts, pre_b, pre_p = _rpn_direct(spec, gpu_device)
    for i, c in enumerate(counts.cpu().tolist()):
        assert torch.equal(got[i], boxes[i, :c]) and torch.equal(got[i].cpu(), spec["expected"][0][i])
        assert torch.equal(pre[i]["proposals"], pre_b[i]) and torch.equal(pre[i]["objectness"], pre_p[i])


@pytest.mark.parametrize("pre", [1000, 1023])
def test_hip_rpn_third_radix_pass_on_consecutive_floats(gpu_device, pre):
    """levels of consecutive fp32 numbers (upwards from +1.0, downwards from -1.0): the selected keys share their upper 22 bits, so the
    third pass and its `need` alone decide; level 0 holds more than 32 768 elements (two trips of the histogram's 1024-element loop).
    All values are distinct: the candidates are anchors[torch.sort order][:k], bit for bit and in that order"""
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd.stock.anchors import AnchorGenerator, ImageList
    sp = G.radix_spec()
    N = sp["N"]
    ag = AnchorGenerator(sp["sizes"], sp["ratios"])
    lg, de, hw, strides = [], [], [], []
    for o in sp["obj"]:
        H, W = o.shape[-2:]
        lg.append(o.permute(0, 2, 3, 1).reshape(N * H * W, 1).contiguous().to(gpu_device))
        de.append(torch.zeros((N * H * W, 4), device=gpu_device))
        hw.append((H, W)); strides.append((sp["canvas"][0] // H, sp["canvas"][1] // W))
    _, _, counts, pre_b, pre_p = ops.rpn_proposals(lg, de, hw, strides, ag.cell_anchors, [sp["canvas"]] * N, pre, 50, 0.7, 0.0, 1e-3)
    feats = [torch.zeros((N, 1) + g) for g in sp["grids"]]
    anchors = ag(ImageList(torch.zeros((N, 3) + sp["canvas"]), [sp["canvas"]] * N), feats)[0]
    pos = koff = 0
    for l, (h, w) in enumerate(sp["grids"]):
        n = h * w
        k = min(pre, n)
        for i in range(N):
            flat = sp["obj"][l][i].reshape(-1)
            order = torch.sort(flat, descending=True, stable=True)[1][:k]
            assert torch.equal(pre_b[i, koff:koff + k].cpu(), anchors[pos:pos + n][order]), "level %d image %d" % (l, i)
            _close_scores(pre_p[i, koff:koff + k], torch.sigmoid(flat[order]), "level %d image %d" % (l, i))
        pos += n
        koff += k
    assert int(counts.min()) > 0


# ---- detector ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.DET_SPECS))
def test_hip_det_postprocess_on_exact_grids(gpu_device, name):
    """ops.det_postprocess and ops.det_postprocess_padded == the oracle: foreground and background blocks in exact order with bit-equal
    boxes and equal labels, all_boxes bit for bit; score values within SCORE_ATOL; the padded form bit-equal to the compacted one"""
    from snn_automotive_object_detection_amd import ops
    spec = G.det_spec(name)
    K, rois, N = spec["K"], spec["rois"], len(spec["rois"])
    e_b, e_s, e_l, e_as, e_ab = spec["expected"]
    dev = gpu_device
    boxes, scores, labels, counts, all_s, all_b = ops.det_postprocess(
        spec["logits"].to(dev), spec["reg"].to(dev), torch.cat(spec["props"]).to(dev), rois, list(spec["image_shapes"]), G.BOX_WEIGHTS,
        G.DET_SCORE_THRESH, spec["nms"], spec["det"])
    cnt = counts.cpu().tolist()
    pos = 0
    for i in range(N):
        n_fg, n_all = int((e_l[i] > 0).sum()), int(e_l[i].shape[0])
        assert cnt[i] == [n_fg, n_all - n_fg], "%s image %d: counts %s" % (name, i, cnt[i])
        assert torch.equal(labels[i, :n_all].cpu().to(torch.int64), e_l[i]), "%s image %d: labels" % (name, i)
        assert torch.equal(boxes[i, :n_all].cpu(), e_b[i]), "%s image %d: boxes" % (name, i)
        _close_scores(scores[i, :n_all], e_s[i], "%s image %d" % (name, i))
        assert torch.equal(all_b[pos:pos + rois[i]].cpu(), e_ab[i]), "%s image %d: all_boxes" % (name, i)
        _close_scores(all_s[pos:pos + rois[i]], e_as[i], "%s image %d all_scores" % (name, i))
        pos += rois[i]
    # the static-shape form: the same rows laid out [N, cap], the counts in device memory
    lg, rg, pr, cn, cap = G.det_padded_inputs(spec, dev)
    p_boxes, p_scores, p_labels, p_counts, p_all_s, p_all_b = ops.det_postprocess_padded(
        lg, rg, pr, cn, list(spec["image_shapes"]), G.BOX_WEIGHTS, G.DET_SCORE_THRESH, spec["nms"], spec["det"])
    assert torch.equal(p_counts, counts)
    pos = 0
    for i in range(N):
        n_all = sum(cnt[i])
        assert torch.equal(p_boxes[i, :n_all], boxes[i, :n_all]) and torch.equal(p_scores[i, :n_all], scores[i, :n_all])
        assert torch.equal(p_labels[i, :n_all], labels[i, :n_all])
        assert not bool(p_boxes[i, n_all:].any()) and not bool(p_scores[i, n_all:].any()) and not bool(p_labels[i, n_all:].any())
        assert torch.equal(p_all_b.view(N, cap, K, 4)[i, :rois[i]], all_b[pos:pos + rois[i]])
        assert torch.equal(p_all_s.view(N, cap, K)[i, :rois[i]], all_s[pos:pos + rois[i]])
        assert not bool(p_all_b.view(N, cap, K, 4)[i, rois[i]:].any()) and not bool(p_all_s.view(N, cap, K)[i, rois[i]:].any())
        pos += rois[i]
