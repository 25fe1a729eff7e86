"""The sixth call of the static path and its runner, as far as the host alone can check them (CPU).

  1. include/snn_hip.h declares snn_pack_padded_detections, the library exports it, _lib.SYMBOLS binds it;
  2. every bad argument of it returns -1 with a message, before any device work (there is no device here);
  3. static.CapturedHeads refuses the dense / auto routes (attribute and environment default) and slots outside {1, 2} before it touches a
     device, the model or its features; dp.all_gather_padded refuses rows of another max_det;
  4. the row layout, restated here in plain torch, decodes a hand-made record: rows below the count are (x1, y1, x2, y2, score, label),
     rows at or past it zero, dp.unpack_detections reads the record back."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)             # a non-null, 16-byte aligned "device pointer" that must never be dereferenced on the host


# ---- 1. header, export, binding ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry():
    from snn_automotive_object_detection_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snn_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+snn_pack_padded_detections\s*\(([^;]*)\)\s*;", txt)
    assert m, "include/snn_hip.h does not declare snn_pack_padded_detections"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[-1].startswith("snn_stream_t") and [a for a in args if a.startswith("int ")] == ["int N", "int out_cap", "int max_det"]
    res, argtypes = _lib.SYMBOLS["snn_pack_padded_detections"]
    assert res is C.c_int and len(argtypes) == 10 and argtypes[4:7] == [C.c_int] * 3
    lib = _lib.load()
    assert hasattr(lib, "snn_pack_padded_detections")
    from snn_automotive_object_detection_amd import ops, static
    assert callable(ops.pack_padded_detections) and callable(static.pack_padded_detections)


# ---- 2. bad arguments -----------------------------------------------------------------------------------------------------------------------
GOOD = dict(boxes=FAKE, scores=FAKE, labels=FAKE, counts_in=FAKE, N=2, out_cap=140, max_det=100, payload=FAKE, counts=FAKE)
BAD = [("N = 0", dict(N=0)), ("N = -1", dict(N=-1)), ("N = 65", dict(N=65)), ("out_cap = 0", dict(out_cap=0)), ("out_cap = -5", dict(out_cap=-5)),
       ("max_det = 0", dict(max_det=0)), ("max_det = -1", dict(max_det=-1))] + \
      [("%s = null" % k, {k: None}) for k in ("boxes", "scores", "labels", "counts_in", "payload", "counts")] + \
      [("boxes off 16 bytes", dict(boxes=C.c_void_p(0x1008))), ("payload off 8 bytes", dict(payload=C.c_void_p(0x1004)))]


@pytest.mark.parametrize("what,change", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_return_minus_one_with_a_message(what, change):
    from snn_automotive_object_detection_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **change)
    p = _lib.snn_params(0.1, -0.2, 0, 0, 0.25, 0.1, 0, 0)
    assert lib.snn_encode_rows(None, 4, 4, 8, C.byref(p), None, 0, None) < 0 and b"snn_encode_rows" in lib.snn_last_error()    # (another entry's text is in place)
    rc = lib.snn_pack_padded_detections(a["boxes"], a["scores"], a["labels"], a["counts_in"], a["N"], a["out_cap"], a["max_det"], a["payload"],
                                        a["counts"], None)
    assert rc == -1, "%s: rc = %d" % (what, rc)
    assert b"snn_pack_padded_detections" in lib.snn_last_error(), lib.snn_last_error()


def test_the_limit_of_max_det_is_a_limit_not_a_bad_argument():
    from snn_automotive_object_detection_amd import _lib
    lib = _lib.load()
    rc = lib.snn_pack_padded_detections(FAKE, FAKE, FAKE, FAKE, 2, 140, (1 << 24) + 1, FAKE, FAKE, None)
    assert rc == -4 and b"max_det" in lib.snn_last_error()


def test_the_wrapper_refuses_host_tensors_and_wrong_shapes():
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd._lib import SnnHipError
    out = dict(boxes=torch.zeros(2, 5, 4), scores=torch.zeros(2, 5), labels=torch.zeros(2, 5, dtype=torch.int32), counts=torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(SnnHipError, match="GPU"):
        ops.pack_padded_detections(out, 5)


# ---- 3. refusals of the runner and of the DP hook ------------------------------------------------------------------------------------------
def _fake_model(conv_route=None, fc6_route=None):
    head = types.SimpleNamespace(conv_route=conv_route)
    det = types.SimpleNamespace(fc6_route=fc6_route)
    return types.SimpleNamespace(rpn=types.SimpleNamespace(head=head), roi_heads=types.SimpleNamespace(box_head_and_predictor=det))


@pytest.fixture
def no_device(monkeypatch):
    """anything that would reach a device, the model's forward or a capture fails the test"""
    from snn_automotive_object_detection_amd import static

    def boom(*a, **k):
        raise AssertionError("the refusal came too late: device work was reached")
    monkeypatch.setattr(static, "heads_padded", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", boom)
    monkeypatch.delenv("SNN_CONV_ROUTE", raising=False)
    monkeypatch.delenv("SNN_FC6_ROUTE", raising=False)


FEATS = {"0": torch.zeros(1, 4, 2, 2)}


@pytest.mark.parametrize("conv,fc6", [("auto", None), ("dense", None), (None, "auto"), (None, "dense"), ("auto", "auto"), ("sparse", "dense")])
def test_runner_refuses_routes_by_attribute(no_device, conv, fc6):
    from snn_automotive_object_detection_amd import static
    with pytest.raises(ValueError, match="sparse"):
        static.CapturedHeads(_fake_model(conv, fc6), FEATS, None)


@pytest.mark.parametrize("var,value", [("SNN_CONV_ROUTE", "auto"), ("SNN_CONV_ROUTE", "dense"), ("SNN_FC6_ROUTE", "auto"), ("SNN_FC6_ROUTE", "dense")])
def test_runner_refuses_routes_by_environment(no_device, monkeypatch, var, value):
    from snn_automotive_object_detection_amd import static
    monkeypatch.setenv(var, value)
    with pytest.raises(ValueError, match=var):
        static.CapturedHeads(_fake_model(), FEATS, None)
    # an explicit "sparse" attribute overrides the environment default, as in the heads' own forward
    assert static._resolved_routes(_fake_model("sparse", "sparse")) == ("sparse", "sparse")


def test_routes_resolve_like_the_heads_do(no_device, monkeypatch):
    """the real modules: attribute None reads the environment at each forward (rpn.py / faster_rcnn.py), default "sparse" """
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import static
    model = types.SimpleNamespace(rpn=types.SimpleNamespace(head=S.RPNHeadSNN(32, 3, 4)),
                                  roi_heads=types.SimpleNamespace(box_head_and_predictor=S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 4)))
    assert static._resolved_routes(model) == ("sparse", "sparse")
    monkeypatch.setenv("SNN_FC6_ROUTE", "auto")
    assert static._resolved_routes(model) == ("sparse", "auto")
    model.roi_heads.box_head_and_predictor.fc6_route = "sparse"
    model.rpn.head.conv_route = "auto"
    assert static._resolved_routes(model) == ("auto", "sparse")


@pytest.mark.parametrize("slots", [0, 3, -1, None, "2"])
def test_runner_refuses_bad_slots(no_device, slots):
    from snn_automotive_object_detection_amd import static
    with pytest.raises(ValueError, match="slots"):
        static.CapturedHeads(_fake_model(), FEATS, None, slots=slots)


def test_runner_refuses_host_features_and_bad_max_det(no_device):
    from snn_automotive_object_detection_amd import static
    with pytest.raises(ValueError, match="GPU"):
        static.CapturedHeads(_fake_model(), FEATS, None)
    with pytest.raises(ValueError, match="max_det"):
        static.CapturedHeads(_fake_model(), FEATS, None, max_det=0)


def test_all_gather_padded_refuses_rows_of_another_max_det():
    from snn_automotive_object_detection_amd import dp
    with pytest.raises(ValueError, match="payload"):
        dp.all_gather_padded((torch.zeros(2, 7, 6), torch.zeros(2, dtype=torch.int32)), 9)
    with pytest.raises(ValueError, match="payload"):
        dp.all_gather_padded((torch.zeros(2, 7, 6), torch.zeros(3, dtype=torch.int32)), 7)


# ---- 4. the row layout ----------------------------------------------------------------------------------------------------------------------
def rows_expected(boxes, scores, labels, counts, max_det):
    """the contract of snn_pack_padded_detections in plain torch on host tensors (tests/test_gpu_pack_rows.py runs the kernel against it)"""
    N, cap = scores.shape
    payload = torch.zeros((N, max_det, 6), dtype=torch.float32)
    out_counts = torch.zeros((N,), dtype=torch.int32)
    for i in range(N):
        k = min(min(max(int(counts[i, 0]) + int(counts[i, 1]), 0), cap), max_det)
        payload[i, :k, 0:4] = boxes[i, :k]
        payload[i, :k, 4] = scores[i, :k]
        payload[i, :k, 5] = labels[i, :k].to(torch.float32)
        out_counts[i] = k
    return payload, out_counts


def test_the_restated_layout_decodes_a_hand_made_record():
    from snn_automotive_object_detection_amd import dp
    nan = float("nan")
    boxes = torch.tensor([[[1., 2., 3., 4.], [5., 6., 7., 8.], [9., 10., 11., 12.], [nan] * 4],
                          [[nan] * 4] * 4])
    scores = torch.tensor([[0.75, 0.5, 0.25, nan], [nan] * 4])
    labels = torch.tensor([[95, 1, 0, 77], [7, 7, 7, 7]], dtype=torch.int32)
    counts = torch.tensor([[2, 1], [0, 0]], dtype=torch.int32)
    payload, cnt = rows_expected(boxes, scores, labels, counts, 5)
    assert cnt.tolist() == [3, 0]
    assert payload[0, :3].tolist() == [[1., 2., 3., 4., 0.75, 95.], [5., 6., 7., 8., 0.5, 1.], [9., 10., 11., 12., 0.25, 0.]]
    assert not payload[0, 3:].any() and not payload[1].any() and not torch.isnan(payload).any()
    dets = dp.unpack_detections(payload, cnt)
    assert len(dets) == 2 and dets[0]["labels"].tolist() == [95, 1, 0] and dets[0]["labels"].dtype == torch.int64
    assert torch.equal(dets[0]["boxes"], boxes[0, :3]) and torch.equal(dets[0]["scores"], scores[0, :3]) and dets[1]["boxes"].shape == (0, 4)
    # truncation keeps the first max_det rows; a garbage count is clamped to the rows there are
    payload, cnt = rows_expected(boxes[:1, :3], scores[:1, :3], labels[:1, :3], torch.tensor([[-7, 1 << 30]], dtype=torch.int32), 2)
    assert cnt.tolist() == [2] and torch.equal(payload[0, :, :4], boxes[0, :2])
    payload, cnt = rows_expected(boxes[:1, :3], scores[:1, :3], labels[:1, :3], torch.tensor([[-7, 1 << 30]], dtype=torch.int32), 8)
    assert cnt.tolist() == [3] and not payload[0, 3:].any()
    # and it is dp.pack_detections' layout
    ref_p, ref_c = dp.pack_detections([{"boxes": boxes[0, :3], "scores": scores[0, :3], "labels": labels[0, :3].long()}], 8, torch.device("cpu"))
    assert torch.equal(ref_p, payload) and torch.equal(ref_c, cnt)
