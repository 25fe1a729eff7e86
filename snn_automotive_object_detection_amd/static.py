"""The static-shape, sync-free path from FPN features to padded detections.

``heads_padded``  RPN head -> snn_rpn_proposals -> snn_roi_assign -> the fused RoIAlign detector head on N * cap rows ->
                  snn_det_postprocess_padded: every per-image count stays in device memory, every shape depends on the configuration
                  alone, nothing waits for the host.
``unpad``         the one host synchronisation: padded tensors -> the list of per-image dicts ``model(images)`` returns.
``pack_padded_detections``  the sixth call: padded detections -> the exchange rows of dp.py (payload [N, max_det, 6], counts [N]), one launch,
                  the counts read on the device: the fixed-size record a deployment copies to pinned memory or hands to the all-gather.
``CapturedHeads`` the runner: ``heads_padded`` (+ the rows) captured into one graph per slot and replayed on new features.

The list API (``GeneralizedRCNN.forward``, ``StreamPipeline``) is the reference's and does not come through here."""
import os
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib


def heads_padded(model, features: Dict[str, Tensor], images) -> Dict[str, Tensor]:
    """FPN features -> padded detections in the coordinates of ``images`` (an ImageList: the padded batch tensor for its shape, the
    per-image sizes), with no host synchronisation.  With cap = the RPN's post_nms_top_n, D = detections_per_img + cap, K classes,
    Kc pre-NMS candidates per image:
        boxes [N, D, 4], scores [N, D], labels [N, D] int32   per image counts[i, 0] foreground detections by decreasing score, then
                                                              counts[i, 1] background boxes, then zeros
        counts [N, 2] int32                                   (fg, bg)
        all_scores [N, cap, K], all_boxes [N, cap, K, 4]      zero at or past roi_counts[i]
        rois [N, cap, 4], roi_counts [N] int32                the proposals the detector head ran on (padding rows zero)
        proposals [N, Kc, 4], objectness [N, Kc]              the RPN's pre-NMS report
        class_logits [N*cap, K], box_regression [N*cap, 4K]   the detector head's outputs on every row, padding included
    Configurations the HIP path does not take raise (RegionProposalNetwork.proposals_padded, RoIHeadsSNN.forward_padded)."""
    rpn, roi_heads = model.rpn, model.roi_heads
    if getattr(rpn.head, "spike_rates", False) or getattr(roi_heads.box_head_and_predictor, "spike_rates", False):
        raise NotImplementedError("the padded path returns detections; spike-rate mode returns rates - use forward()")
    feats = list(features.values())
    boxes, counts, extras = rpn.proposals_padded(images, feats, rpn.head(feats))
    out = roi_heads.forward_padded(features, boxes, counts, images.image_sizes)
    out["proposals"], out["objectness"] = extras["proposals"], extras["objectness"]
    return out


def unpad(out: Dict[str, Tensor]) -> List[Dict[str, Tensor]]:
    """padded outputs (``forward_padded`` / ``heads_padded``) -> what ``model(images)`` returns: per image ``boxes``, ``labels`` (int64),
    ``scores`` cut to fg + bg rows, ``all_scores`` / ``all_boxes`` cut to the image's RoIs and, when the RPN's report is there,
    ``proposals`` / ``objectness``.  The one host synchronisation of the padded path: the counts come to the host here.  The slices
    are views of the padded tensors."""
    host = torch.cat([out["counts"].sum(1).reshape(-1), out["roi_counts"].reshape(-1)]).tolist()
    n = len(host) // 2
    result = []
    for i in range(n):
        c, r = int(host[i]), int(host[n + i])
        det = {"boxes": out["boxes"][i, :c], "labels": out["labels"][i, :c].to(torch.int64), "scores": out["scores"][i, :c],
               "all_scores": out["all_scores"][i, :r], "all_boxes": out["all_boxes"][i, :r]}
        if "proposals" in out:
            det["proposals"], det["objectness"] = out["proposals"][i], out["objectness"][i]
        result.append(det)
    return result


def pack_padded_detections(out: Dict[str, Tensor], max_det: int) -> Tuple[Tensor, Tensor]:
    """padded detections (the ``boxes`` [N, D, 4], ``scores`` [N, D], ``labels`` [N, D] int32 and ``counts`` [N, 2] int32 of
    ``heads_padded`` / ``forward_padded``) -> (payload [N, max_det, 6] fp32 = (x1, y1, x2, y2, score, label), counts [N] int32): bit for bit
    ``dp.pack_detections(unpad(out), max_det, device)`` without the host reading a count (include/snn_hip.h: snn_pack_padded_detections).
    One launch on the current stream, no workspace, capturable; every element of both results is written on every call."""
    from . import ops
    boxes, scores, labels, counts = out["boxes"], out["scores"], out["labels"], out["counts"]
    ops._need_gpu(boxes, "padded detections")
    if boxes.dim() != 3 or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) or tuple(labels.shape) != tuple(boxes.shape[:2]) \
            or tuple(counts.shape) != (boxes.shape[0], 2):
        raise _lib.SnnHipError("pack_padded_detections: boxes [N, D, 4], scores [N, D], labels [N, D] and counts [N, 2] expected, got %s, %s, %s, %s"
                               % (tuple(boxes.shape), tuple(scores.shape), tuple(labels.shape), tuple(counts.shape)))
    if int(max_det) < 1 or boxes.shape[0] < 1 or boxes.shape[1] < 1:
        raise _lib.SnnHipError("pack_padded_detections: max_det = %r on boxes %s (at least one image, one row, max_det >= 1)" % (max_det, tuple(boxes.shape)))
    lib = _lib.load()
    N, D = int(boxes.shape[0]), int(boxes.shape[1])
    bx, sc = ops._f32c(boxes), ops._f32c(scores)
    lb, cn = labels.detach().to(torch.int32).contiguous(), counts.detach().to(torch.int32).contiguous()
    with torch.cuda.device(boxes.device):
        payload = torch.empty((N, int(max_det), 6), dtype=torch.float32, device=boxes.device)
        rows = torch.empty((N,), dtype=torch.int32, device=boxes.device)
        _lib.check(lib.snn_pack_padded_detections(ops._ptr(bx), ops._ptr(sc), ops._ptr(lb), ops._ptr(cn), N, D, int(max_det), ops._ptr(payload),
                                                  ops._ptr(rows), ops._stream()), "snn_pack_padded_detections")
    return payload, rows


def _resolved_routes(model) -> Tuple[str, str]:
    """the routes a forward of the two heads would take now: the attribute, else the environment default, else "sparse" """
    rpn_head, det_head = model.rpn.head, model.roi_heads.box_head_and_predictor
    conv = getattr(rpn_head, "conv_route", None)
    fc6 = getattr(det_head, "fc6_route", None)
    return (conv if conv is not None else os.environ.get("SNN_CONV_ROUTE", "sparse"),
            fc6 if fc6 is not None else os.environ.get("SNN_FC6_ROUTE", "sparse"))


def _weights(head) -> tuple:
    return tuple(p for p in head.parameters())


def _settings(model) -> tuple:
    """everything a captured graph has baked in and a later call could find changed, read on the host alone"""
    rpn, roi = model.rpn, model.roi_heads
    heads = (rpn.head, roi.box_head_and_predictor)
    return (tuple(int(h.num_steps) for h in heads), tuple(h.precision for h in heads), tuple(h._eff_precision() for h in heads),
            tuple(h.li_order for h in heads), tuple(float(h.dt) for h in heads), _resolved_routes(model),
            tuple((p.data_ptr(), p._version, str(p.device)) for h in heads for p in _weights(h)),
            int(rpn.pre_nms_top_n()), int(rpn.post_nms_top_n()), float(rpn.nms_thresh), float(rpn.score_thresh), float(rpn.min_size),
            float(roi.score_thresh), float(roi.nms_thresh), int(roi.detections_per_img), tuple(float(w) for w in roi.box_coder.weights),
            rpn.post, roi.post, bool(model.training or rpn.training or roi.training))


_SETTING_NAMES = ("num_steps", "precision", "effective precision", "li_order", "dt", "conv_route / fc6_route", "weights", "pre_nms_top_n",
                  "post_nms_top_n", "rpn.nms_thresh", "rpn.score_thresh", "rpn.min_size", "roi_heads.score_thresh", "roi_heads.nms_thresh",
                  "detections_per_img", "box_coder.weights", "rpn.post", "roi_heads.post", "training")


def _feature_spec(features: Dict[str, Tensor]) -> tuple:
    from . import ops
    return tuple((k, tuple(v.shape), v.dtype, ops.feat_layout(v), str(v.device)) for k, v in features.items())


class _Slot:
    """one capture: its static feature tensors, its graph, the dict of tensors the graph writes"""
    def __init__(self, features):
        self.inputs = type(features)((k, v.detach().clone(memory_format=torch.preserve_format)) for k, v in features.items())
        self.graph = None
        self.out: Dict[str, Tensor] = {}


class CapturedHeads:
    """``heads_padded`` captured into a graph and replayed on new features: FPN features -> padded detections in ONE
    graph launch, no host synchronisation, and - with ``max_det`` - the exchange rows ``payload`` [N, max_det, 6] / ``payload_counts`` [N]
    of ``pack_padded_detections`` from the same graph (``counts`` stays the [N, 2] (fg, bg) tensor ``unpad`` reads).

        runner = CapturedHeads(model, features, images, max_det=100, slots=2)
        out = runner(features)           # copy_ into the slot's static inputs, one replay, the slot's output dict
        runner.close()

    ``features`` at construction are example tensors: their keys, shapes, dtypes, memory formats and device are what every call must
    bring; ``images`` (an ImageList) fixes the image sizes.  Construction runs ONE eager warm-up call on the example features (packed
    weights, the host copy of the cell anchors and the ratio tables are cached there; every refusal of ``heads_padded`` surfaces from
    it unchanged), then captures once per slot on one stream with ``torch.cuda.graph``: no parallel branches, no extra streams.  The
    backbone stays outside: the runner starts at the FPN features.

    LIFETIME OF THE RESULTS: the tensors a call returns are the slot's static outputs.  They are valid until that slot is used
    again - the next call with ``slots=1``, the call after the next with ``slots=2`` (so a consumer can still read batch k, or run its
    copy to pinned memory, while batch k + 1 replays).  Copy what has to live longer.

    Refusals, all before any device work, none falling back or re-capturing: ValueError for a ``conv_route`` / ``fc6_route`` that resolves
    (attribute, else SNN_CONV_ROUTE / SNN_FC6_ROUTE) to anything but "sparse" - the ``auto`` routes under replay at these shapes have an
    open defect and stay excluded until it is closed - for ``slots`` outside {1, 2}, and for a call whose features differ
    from the captured ones in keys, shape, dtype, memory format or device; RuntimeError for a call after ``num_steps``, ``precision``, the
    weights (in-place edits, ``invalidate_packed_weights``), ``post_nms_top_n``, a threshold or a route changed since the capture, or
    after ``close()`` (the check reads the host only).

    The runner holds every tensor its graphs reference: the static inputs and outputs, the packed weights, and its workspaces.  Every
    slot captures on a workspace of its OWN: what ``ops._WS`` / ``ops._WS_RATES`` hold for the capture stream is set aside for the
    duration of the capture and put back afterwards, so the buffers handed out in between belong to this slot's graph alone - no other
    graph, runner or eager call is ever handed them.  ``close()`` drops the graphs and takes exactly those buffers out of ``captured``."""

    def __init__(self, model, features: Dict[str, Tensor], images, max_det: Optional[int] = None, slots: int = 1):
        from . import ops
        if slots not in (1, 2):
            raise ValueError("CapturedHeads: slots must be 1 or 2, got %r" % (slots,))
        if max_det is not None and int(max_det) < 1:
            raise ValueError("CapturedHeads: max_det must be >= 1 or None, got %r" % (max_det,))
        routes = _resolved_routes(model)
        if routes != ("sparse", "sparse"):
            raise ValueError("CapturedHeads: conv_route = %r, fc6_route = %r (attribute or SNN_CONV_ROUTE / SNN_FC6_ROUTE): only \"sparse\" is "
                             "captured - the auto routes under replay have an open defect (DESIGN.md 8)" % routes)
        for k, v in features.items():
            if not isinstance(v, Tensor) or not v.is_cuda:
                raise ValueError("CapturedHeads: feature %r must be a tensor on the GPU" % (k,))
        self.model, self.images, self.max_det = model, images, None if max_det is None else int(max_det)
        self._spec = _feature_spec(features)
        self._device = next(iter(features.values())).device
        self._graphs_closed = False
        self._next = 0
        self._mine = {"_WS": [], "_WS_RATES": []}          # workspaces handed out during this runner's captures
        with torch.cuda.device(self._device):
            self._slots = [_Slot(features) for _ in range(slots)]
            self._run(self._slots[0].inputs)               # warm-up: caches fill here, refusals of heads_padded surface here
            self._settings = _settings(model)
            self._packed = [c.val for h in (model.rpn.head, model.roi_heads.box_head_and_predictor) for c in h._caches()]
            before = {name: list(getattr(getattr(ops, name), "captured", ())) for name in self._mine}
            try:
                for slot in self._slots:
                    self._capture(slot)
            except BaseException:
                self._note_workspaces(before)
                self.close()                                   # a failed capture leaves nothing behind
                raise
            self._note_workspaces(before)

    def _note_workspaces(self, before) -> None:
        from . import ops
        for name in self._mine:
            now = getattr(getattr(ops, name), "captured", ())
            self._mine[name] = [b for b in now if not any(b is o for o in before[name])]

    def _run(self, inputs) -> Dict[str, Tensor]:
        out = heads_padded(self.model, inputs, self.images)
        if self.max_det is not None:
            out["payload"], out["payload_counts"] = pack_padded_detections(out, self.max_det)
        return out

    def _capture(self, slot: _Slot) -> None:
        torch.cuda.synchronize(self._device)
        graph = torch.cuda.CUDAGraph()
        failure = None
        try:
            with torch.cuda.graph(graph):
                parked = self._park_workspaces()
                try:
                    slot.out = self._run(slot.inputs)
                except BaseException as e:                 # leave the capture first (the context ends it), then wait, then raise: no retry
                    failure = e
                finally:
                    self._unpark_workspaces(parked)
        except BaseException as e:
            failure = failure or e
        if failure is not None:
            torch.cuda.synchronize(self._device)
            raise failure
        slot.graph = graph

    def _park_workspaces(self) -> list:
        """inside a capture: what ops._WS / ops._WS_RATES hold for the capture stream is set aside, so the captured calls are handed fresh
        buffers (from the graph's own pool) that nobody else knows"""
        from . import ops
        key = (self._device.type, self._device.index, torch.cuda.current_stream(self._device).cuda_stream)
        parked = []
        for name in self._mine:
            buf = getattr(getattr(ops, name), "buf", None)
            if isinstance(buf, dict):
                parked.append((buf, key, buf.pop(key, None)))
        return parked

    @staticmethod
    def _unpark_workspaces(parked: list) -> None:
        for buf, key, old in parked:
            buf.pop(key, None)                             # the slot's buffer: ``captured`` and the graph's pool keep it, nobody is handed it again
            if old is not None:
                buf[key] = old

    def _check(self, features: Dict[str, Tensor]) -> None:
        if self._graphs_closed:
            raise RuntimeError("CapturedHeads: called after close()")
        spec = _feature_spec(features)
        if spec != self._spec:
            raise ValueError("CapturedHeads: features differ from the captured ones (key, shape, dtype, layout, device): got %s, captured %s"
                             % (spec, self._spec))
        now = _settings(self.model)
        if now != self._settings:
            changed = [n for n, a, b in zip(_SETTING_NAMES, self._settings, now) if a != b]
            raise RuntimeError("CapturedHeads: %s changed since the capture; make a new runner" % ", ".join(changed))
        heads = (self.model.rpn.head, self.model.roi_heads.box_head_and_predictor)
        if any(held is not None and c.val is not held for held, c in zip(self._packed, [c for h in heads for c in h._caches()])):
            raise RuntimeError("CapturedHeads: the packed weights were dropped or repacked since the capture (invalidate_packed_weights, "
                               ".to(), load_state_dict); make a new runner")

    def __call__(self, features: Dict[str, Tensor]) -> Dict[str, Tensor]:
        self._check(features)
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        with torch.cuda.device(self._device):
            for k, v in features.items():
                slot.inputs[k].copy_(v)
            slot.graph.replay()
        return slot.out

    def close(self) -> None:
        """drop the graphs and release what ops._WS / ops._WS_RATES keep for them; the runner cannot be called afterwards"""
        from . import ops
        if self._graphs_closed:
            return
        self._graphs_closed = True
        torch.cuda.synchronize(self._device)
        for slot in self._slots:
            slot.graph = None
        for name in self._mine:
            ws = getattr(ops, name)
            if hasattr(ws, "captured"):
                ws.captured[:] = [b for b in ws.captured if not any(b is m for m in self._mine[name])]
            self._mine[name] = []
        self._slots, self._packed = [], []
