"""The static-shape path as far as it goes without a GPU: the two new entry points are exported and refuse bad arguments
before any device work, static.unpad rebuilds the list structure, and every configuration the padded path does not take raises the
documented exception instead of falling back to the synchronising stock path."""
import ctypes as C

import pytest
import torch

from snn_automotive_object_detection_amd import _lib

FAKE = C.c_void_p(0x1000)        # a non-null "device pointer" that must never be dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _refused(lib, rc, name):
    assert rc < 0, "%s accepted bad arguments (rc=%d)" % (name, rc)
    assert name in lib.snn_last_error().decode(), lib.snn_last_error()


def test_new_symbols_are_exported(lib):
    for name in ("snn_roi_assign", "snn_det_postprocess_padded"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib.__file__), "..", "include", "snn_hip.h")).read()
    assert "int snn_roi_assign(" in header and "int snn_det_postprocess_padded(" in header


def _assign(lib, boxes=FAKE, counts=FAKE, N=2, cap=70, k_min=2, k_max=5, scale=224.0, rois=FAKE, batch=FAKE, level=FAKE):
    return lib.snn_roi_assign(boxes, counts, N, cap, k_min, k_max, scale, 4.0, rois, batch, level, None)


@pytest.mark.parametrize("kw", [dict(boxes=None), dict(counts=None), dict(rois=None), dict(batch=None), dict(level=None),
                                dict(N=0), dict(N=-1), dict(N=65), dict(cap=0), dict(cap=-5), dict(cap=10241),
                                dict(k_min=5, k_max=2), dict(k_min=0, k_max=8), dict(scale=0.0)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_roi_assign_refuses_bad_arguments(lib, kw):
    _refused(lib, _assign(lib, **kw), "snn_roi_assign")


def _post(lib, logits=FAKE, counts=FAKE, N=2, cap=70, K=5, hw=True, det=10, out_cap=None, ws=FAKE, ws_bytes=1 << 40):
    hw_ = (C.c_float * (2 * max(N, 1)))(*([64.0] * (2 * max(N, 1)))) if hw else None
    bw = (C.c_float * 4)(10.0, 10.0, 5.0, 5.0)
    out_cap = det + cap if out_cap is None else out_cap
    return lib.snn_det_postprocess_padded(logits, FAKE, FAKE, counts, N, cap, K, hw_, bw, 0.05, 0.5, det, 1e-2, *([FAKE] * 6), out_cap,
                                          ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(logits=None), dict(counts=None), dict(hw=False), dict(ws=None),
                                dict(N=0), dict(N=65), dict(cap=0), dict(cap=-1), dict(cap=10241), dict(K=1), dict(K=97), dict(det=0),
                                dict(out_cap=79),                                   # detections_per_img + cap = 80
                                dict(cap=5000, K=9, det=2000),                      # (K-1) * min(det, cap) = 16000 > 8192
                                dict(ws_bytes=64)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_det_postprocess_padded_refuses_bad_arguments(lib, kw):
    _refused(lib, _post(lib, **kw), "snn_det_postprocess_padded")


# ---- static.unpad ----------------------------------------------------------------------------------------------------------------
def _padded(counts, roi_counts, cap=5, K=3, det=4, with_rpn=True):
    N, D = len(counts), det + cap
    g = torch.Generator().manual_seed(3)
    out = {"boxes": torch.rand((N, D, 4), generator=g), "scores": torch.rand((N, D), generator=g),
           "labels": torch.randint(0, K, (N, D), generator=g, dtype=torch.int32), "counts": torch.tensor(counts, dtype=torch.int32),
           "all_scores": torch.rand((N, cap, K), generator=g), "all_boxes": torch.rand((N, cap, K, 4), generator=g),
           "rois": torch.rand((N, cap, 4), generator=g), "roi_counts": torch.tensor(roi_counts, dtype=torch.int32)}
    if with_rpn:
        out["proposals"], out["objectness"] = torch.rand((N, 7, 4), generator=g), torch.rand((N, 7), generator=g)
    return out


@pytest.mark.parametrize("with_rpn", [True, False])
def test_unpad_rebuilds_the_list_structure(with_rpn):
    from snn_automotive_object_detection_amd import static
    counts, roi_counts = [(3, 2), (0, 0), (0, 4)], [5, 0, 4]
    out = _padded(counts, roi_counts, with_rpn=with_rpn)
    res = static.unpad(out)
    assert isinstance(res, list) and len(res) == 3
    keys = ["boxes", "labels", "scores", "all_scores", "all_boxes"] + (["proposals", "objectness"] if with_rpn else [])
    for i, ((fg, bg), r) in enumerate(zip(counts, roi_counts)):
        d = res[i]
        assert list(d) == keys                                   # the key order of model(images)
        assert d["boxes"].shape == (fg + bg, 4) and torch.equal(d["boxes"], out["boxes"][i, :fg + bg])
        assert d["scores"].shape == (fg + bg,) and torch.equal(d["scores"], out["scores"][i, :fg + bg])
        assert d["labels"].dtype == torch.int64 and torch.equal(d["labels"], out["labels"][i, :fg + bg].long())
        assert d["all_scores"].shape == (r, 3) and torch.equal(d["all_scores"], out["all_scores"][i, :r])
        assert d["all_boxes"].shape == (r, 3, 4) and torch.equal(d["all_boxes"], out["all_boxes"][i, :r])
        if with_rpn:
            assert torch.equal(d["proposals"], out["proposals"][i]) and torch.equal(d["objectness"], out["objectness"][i])


# ---- refusals: nothing falls back to the synchronising stock path -------------------------------------------------------------------
def _small_heads(only_one_bbox=False):
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd.model import _default_anchorgen
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    rpn = S.RegionProposalNetwork(_default_anchorgen(), S.RPNHeadSNN(32, 3, 4), 0.7, 0.3, 256, 0.5, dict(training=20, testing=10),
                                  dict(training=20, testing=10), 0.7).eval()
    pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    roi = S.RoIHeadsSNN(pool, S.FastRCNNPredictorSNNFull(32 * 49, 64, 5, 4, only_one_bbox=only_one_bbox), 0.5, 0.5, 512, 0.25, None,
                        0.05, 0.5, 10).eval()
    return rpn, roi


def _rpn_call(rpn, A=3, levels=5):
    from snn_automotive_object_detection_amd.stock.anchors import ImageList
    images = ImageList(torch.empty((2, 0, 64, 64)), [(64, 64)] * 2)
    obj = [torch.zeros((2, A, 16 >> l, 16 >> l)) for l in range(levels)]
    dl = [torch.zeros((2, 4 * A, 16 >> l, 16 >> l)) for l in range(levels)]
    return images, obj, dl


def test_rpn_padded_refusals():
    rpn, _ = _small_heads()
    images, obj, dl = _rpn_call(rpn)
    with pytest.raises(NotImplementedError):
        rpn.proposals_padded(images, None, (obj, dl, [torch.zeros(2, 2)]))          # spike-rate mode: the head's third value
    rpn.train()
    with pytest.raises(NotImplementedError):
        rpn.proposals_padded(images, None, (obj, dl))
    rpn.eval()
    rpn.post = "batched"
    with pytest.raises(ValueError, match="post"):
        rpn.proposals_padded(images, None, (obj, dl))
    rpn.post = "hip"
    images17, obj17, dl17 = _rpn_call(rpn, A=17)
    with pytest.raises(ValueError, match="anchors"):
        rpn.proposals_padded(images17, None, (obj17, dl17))


def test_roi_heads_padded_refusals():
    _, roi = _small_heads()
    feats = {str(l): torch.zeros((2, 32, 16 >> l, 16 >> l)) for l in range(4)}
    boxes, counts, shapes = torch.zeros((2, 10, 4)), torch.zeros((2,), dtype=torch.int32), [(64, 64)] * 2
    call = lambda r=roi, b=boxes: r.forward_padded(feats, b, counts, shapes)
    roi.train()
    with pytest.raises(NotImplementedError):
        call()
    roi.eval()
    roi.box_head_and_predictor.spike_rates = True
    with pytest.raises(NotImplementedError):
        call()
    roi.box_head_and_predictor.spike_rates = False
    with pytest.raises(NotImplementedError):
        call(_small_heads(only_one_bbox=True)[1])
    roi.post = "reference"
    with pytest.raises(ValueError, match="post"):
        call()
    roi.post = "hip"
    roi.fuse_roi_align = False
    with pytest.raises(ValueError, match="RoIAlign"):
        call()
    roi.fuse_roi_align = True
    roi.box_roi_pool.sampling_ratio = 4
    with pytest.raises(ValueError, match="RoIAlign"):
        call()
    roi.box_roi_pool.sampling_ratio = 2
    with pytest.raises(ValueError, match="10240"):
        call(b=torch.zeros((2, 10241, 4)))                                           # the limits are evaluated with cap
    roi.detections_per_img = 5000
    with pytest.raises(ValueError, match="8192"):
        call(b=torch.zeros((2, 5000, 4)))


def test_detector_padded_refusals():
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import static
    rpn, roi = _small_heads()

    class M(torch.nn.Module):
        pass
    m = M()
    m.rpn, m.roi_heads = rpn, roi
    rpn.head.spike_rates = True
    with pytest.raises(NotImplementedError):
        static.heads_padded(m, {"0": torch.zeros((1, 32, 4, 4))}, None)
    rpn.head.spike_rates = False
    model = S.GeneralizedRCNN(torch.nn.Identity(), rpn, roi, torch.nn.Identity())
    model.train()
    with pytest.raises(NotImplementedError):
        model.forward_padded([torch.zeros((3, 8, 8))])
