"""``RoIHeadsSNN`` with the reference's constructor/forward signature (/root/reference/roi_heads.py:
901-1347, inference side): box_roi_pool -> **spiking head** (the accelerated call, roi_heads.py:1230) ->
postprocess_detections (1075-1176) that keeps the surviving background boxes and returns
``all_scores`` / ``all_boxes`` for new-object discovery.  Everything except the head call is stock torch."""
import warnings
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn, Tensor

from .stock import boxes as box_ops
from .rpn import _WARN_LOCK


class RoIHeadsSNN(nn.Module):
    def __init__(self, box_roi_pool, box_head_and_predictor,
                 fg_iou_thresh, bg_iou_thresh, batch_size_per_image, positive_fraction, bbox_reg_weights,
                 score_thresh, nms_thresh, detections_per_img,
                 mask_roi_pool=None, mask_head=None, mask_predictor=None,
                 keypoint_roi_pool=None, keypoint_head=None, keypoint_predictor=None):
        super().__init__()
        if bbox_reg_weights is None:
            bbox_reg_weights = (10.0, 10.0, 5.0, 5.0)                                # roi_heads.py:938-940
        self.box_coder = box_ops.BoxCoder(bbox_reg_weights)
        self.box_roi_pool = box_roi_pool
        self.box_head_and_predictor = box_head_and_predictor
        self.score_thresh = score_thresh
        self.nms_thresh = nms_thresh
        self.detections_per_img = detections_per_img
        self.fuse_roi_align = True        # use the fused RoIAlign+encoder kernel when pool/head support it
        self.post = "hip"                 # "hip": snn_det_postprocess; "reference": the reference's order on stock torch ops
        self._warned = set()              # fallback reasons already reported
        # training-side hyper-parameters: read by head_losses alone (the Matcher's thresholds, the sampler's two numbers)
        self.fg_iou_thresh, self.bg_iou_thresh = fg_iou_thresh, bg_iou_thresh
        self.batch_size_per_image, self.positive_fraction = batch_size_per_image, positive_fraction
        if any(m is not None for m in (mask_roi_pool, mask_head, mask_predictor, keypoint_roi_pool,
                                       keypoint_head, keypoint_predictor)):
            raise NotImplementedError("mask/keypoint branches are dead code in the reference (train.py:263-268)")

    def has_mask(self):
        return False

    def has_keypoint(self):
        return False

    def postprocess_detections(self, class_logits: Tensor, box_regression: Tensor, proposals: List[Tensor],
                               image_shapes: List[Tuple[int, int]]):
        per_image = [p.shape[0] for p in proposals]
        if box_regression.shape[-1] != 4 * class_logits.shape[-1]:
            # --only-one-bbox heads (faster_rcnn.py:460-467) give [R, 4]: the reference's own post-processing then slices
            # boxes[:, 1:] (roi_heads.py:1115) down to nothing while scores keep K-1 columns - not a usable path
            raise NotImplementedError("postprocess_detections needs %d box outputs per RoI (4 per class), got %d "
                                      "(only_one_bbox heads are not supported past the head, SURVEY.md appendix C.6)"
                                      % (4 * class_logits.shape[-1], box_regression.shape[-1]))
        if class_logits.is_cuda and self.post == "hip" and per_image and max(per_image) > 0:
            why = self._hip_postprocess_refusal(len(per_image), max(per_image), class_logits.shape[-1])
            if why is None:
                return self._postprocess_hip(class_logits, box_regression, proposals, image_shapes, per_image)
            with _WARN_LOCK:                                  # loud, once per reason: the stock-torch path is ~4x slower per batch
                first = why not in self._warned
                self._warned.add(why)
            if first:
                warnings.warn("RoIHeadsSNN: detection post-processing falls back to the stock torch ops (%s)" % why, RuntimeWarning)
        return self.postprocess_detections_reference(class_logits, box_regression, proposals, image_shapes)

    def _hip_postprocess_refusal(self, n_images: int, max_rois: int, n_classes: int):
        """the limits of snn_det_postprocess (csrc/snn_kernels.hip / snn_post.h), mirrored so that a configuration outside them
        takes the reference path instead of raising: None if the HIP path can run, else the reason"""
        if n_images > 64:
            return "%d images per batch (HIP path: <= 64)" % n_images
        if n_classes < 2 or n_classes > 96:
            return "%d classes (HIP path: 2..96)" % n_classes
        if max_rois > 10240:                                  # 2 x 64 x ceil(R / 64) x 8 B of LDS for the NMS walk (also <= DET_SORT_MAX)
            return "%d RoIs per image (HIP path: <= 10240)" % max_rois
        if (n_classes - 1) * min(int(self.detections_per_img), max_rois) > 8192:
            return "(K-1) x detections_per_img = %d ranked candidates per image (HIP path: <= 8192)" % (
                (n_classes - 1) * min(int(self.detections_per_img), max_rois))
        return None

    def _postprocess_hip(self, class_logits, box_regression, proposals, image_shapes, per_image):
        """snn_det_postprocess: five launches and one host synchronisation for the batch"""
        from . import ops
        boxes, scores, labels, counts, all_scores, all_boxes = ops.det_postprocess(
            class_logits.detach(), box_regression.detach(), torch.cat(proposals, 0), per_image, image_shapes,
            self.box_coder.weights, self.score_thresh, self.nms_thresh, self.detections_per_img)
        cnt = counts.sum(1).tolist()                                                   # the one host synchronisation
        out = ([], [], [], list(all_scores.split(per_image, 0)), list(all_boxes.split(per_image, 0)))
        for i, c in enumerate(cnt):
            out[0].append(boxes[i, :c]); out[1].append(scores[i, :c]); out[2].append(labels[i, :c].to(torch.int64))
        return out

    def postprocess_detections_reference(self, class_logits: Tensor, box_regression: Tensor, proposals: List[Tensor],
                                         image_shapes: List[Tuple[int, int]]):
        device = class_logits.device
        num_classes = class_logits.shape[-1]
        per_image = [p.shape[0] for p in proposals]
        pred_boxes = self.box_coder.decode(box_regression, proposals)
        pred_scores = F.softmax(class_logits, -1)
        out = ([], [], [], [], [])
        for boxes, scores, shape in zip(pred_boxes.split(per_image, 0), pred_scores.split(per_image, 0), image_shapes):
            boxes = box_ops.clip_boxes_to_image(boxes, shape)
            labels = torch.arange(num_classes, device=device).view(1, -1).expand_as(scores)
            boxes_all, scores_all = boxes.detach().clone(), scores.detach().clone()
            boxes_bg, scores_bg, labels_bg = boxes[:, 0].reshape(-1, 4), scores[:, 0].reshape(-1), labels[:, 0].reshape(-1)
            boxes, scores, labels = boxes[:, 1:].reshape(-1, 4), scores[:, 1:].reshape(-1), labels[:, 1:].reshape(-1)
            inds = torch.where(scores > self.score_thresh)[0]                         # roi_heads.py:1134
            boxes, scores, labels = boxes[inds], scores[inds], labels[inds]
            # background boxes survive only for RoIs without any foreground detection (1137-1148;
            # vectorised form of the reference's per-detection Python loop)
            is_bg = torch.ones(scores_bg.shape[0], dtype=torch.bool, device=device)
            is_bg[torch.div(inds, num_classes - 1, rounding_mode="trunc")] = False
            inds_bg = torch.where(is_bg)[0]
            boxes_bg, scores_bg, labels_bg = boxes_bg[inds_bg], scores_bg[inds_bg], labels_bg[inds_bg]
            keep = box_ops.remove_small_boxes(boxes, min_size=1e-2)
            boxes, scores, labels = boxes[keep], scores[keep], labels[keep]
            keep_bg = box_ops.remove_small_boxes(boxes_bg, min_size=1e-2)
            boxes_bg, scores_bg, labels_bg = boxes_bg[keep_bg], scores_bg[keep_bg], labels_bg[keep_bg]
            keep = box_ops.batched_nms(boxes, scores, labels, self.nms_thresh)[: self.detections_per_img]
            keep_bg = box_ops.batched_nms(boxes_bg, scores_bg, labels_bg, self.nms_thresh)
            out[0].append(torch.cat((boxes[keep], boxes_bg[keep_bg]), dim=0))
            out[1].append(torch.cat((scores[keep], scores_bg[keep_bg]), dim=0))
            out[2].append(torch.cat((labels[keep], labels_bg[keep_bg]), dim=0))
            out[3].append(scores_all)
            out[4].append(boxes_all)
        return out

    def forward(self, features: Dict[str, Tensor], proposals: List[Tensor], image_shapes: List[Tuple[int, int]],
                targets: Optional[List[Dict[str, Tensor]]] = None):
        if self.training:
            raise NotImplementedError("inference only: training the RoI heads is out of scope (DESIGN.md §7)")
        pool, head = self.box_roi_pool, self.box_head_and_predictor
        if self._fuses_roi_align("forward_roialign"):
            # RoIAlign fused into the head's encoder kernel: same values as the two calls below
            feats, scales, rois, lvl = pool.assign(features, proposals, image_shapes)
            head_out = head.forward_roialign(feats, scales, rois, lvl)
        else:
            box_features = pool(features, proposals, image_shapes)                   # roi_heads.py:1217
            head_out = head(box_features)                                            # roi_heads.py:1230 (HIP)
        return self.detections_from_head(head_out, proposals, image_shapes)

    @torch.no_grad()
    def forward_padded(self, features: Dict[str, Tensor], boxes: Tensor, counts: Tensor, image_shapes: List[Tuple[int, int]]) -> Dict[str, Tensor]:
        """``forward`` on padded proposals with no host synchronisation: boxes [N, cap, 4], counts [N] int32 in device
        memory (RegionProposalNetwork.proposals_padded) -> a dict of fixed-shape tensors, D = detections_per_img + cap:
        boxes [N, D, 4], scores [N, D], labels [N, D] int32 (per image counts[i, 0] foreground detections, then counts[i, 1] background
        boxes, then zeros), counts [N, 2], all_scores [N, cap, K], all_boxes [N, cap, K, 4] (zero at or past roi_counts[i]),
        rois [N, cap, 4] (the proposals, padding zeroed), roi_counts [N] (counts clamped to 0 .. cap), and the head's own outputs on
        every row, padding included: class_logits [N*cap, K], box_regression [N*cap, 4K] (what the detections were computed from).
        ops.roi_assign -> the fused RoIAlign head on all N * cap rows -> ops.det_postprocess_padded: the padding rows go through the
        head and are ignored.  Nothing falls back: NotImplementedError for training / spike-rate mode / only_one_bbox, ValueError with the
        reason for ``post`` != "hip", a pool or head the fused RoIAlign path does not take, a shape outside snn_det_postprocess' limits."""
        from . import ops
        pool, head = self.box_roi_pool, self.box_head_and_predictor
        if self.training:
            raise NotImplementedError("inference only: training the RoI heads is out of scope (DESIGN.md §7)")
        if getattr(head, "spike_rates", False):
            raise NotImplementedError("forward_padded: spike-rate mode returns rates, not detections - use forward()")
        if getattr(head, "only_one_bbox", False):
            raise NotImplementedError("forward_padded: only_one_bbox heads are not supported past the head (SURVEY.md appendix C.6)")
        if self.post != "hip":
            raise ValueError("forward_padded: post = %r (only \"hip\" writes padded detections)" % (self.post,))
        if not self._fuses_roi_align("forward_roialign"):
            raise ValueError("forward_padded: needs the fused RoIAlign head path (fuse_roi_align, a head with forward_roialign, "
                             "a 7x7 sampling-2 MultiScaleRoIAlign pool)")
        if boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.shape[0] != len(image_shapes):
            raise ValueError("forward_padded: boxes [N, cap, 4] for %d images expected, got %s" % (len(image_shapes), tuple(boxes.shape)))
        N, cap, K = boxes.shape[0], boxes.shape[1], head.num_classes
        why = self._hip_postprocess_refusal(N, cap, K) if cap > 0 else "cap = 0 rows per image"
        if why is not None:
            raise ValueError("forward_padded: %s" % why)
        feats, scales, k_min, k_max = pool.levels(features, image_shapes)
        rois, roi_batch, roi_level = ops.roi_assign(boxes, counts, k_min, k_max, pool.canonical_scale, pool.canonical_level)
        class_logits, box_regression = head.forward_roialign(feats, scales, rois, roi_level, roi_batch)
        out_boxes, scores, labels, out_counts, all_scores, all_boxes = ops.det_postprocess_padded(
            class_logits, box_regression, rois, counts, image_shapes, self.box_coder.weights, self.score_thresh, self.nms_thresh,
            self.detections_per_img)
        return {"boxes": out_boxes, "scores": scores, "labels": labels, "counts": out_counts,
                "all_scores": all_scores.view(N, cap, K), "all_boxes": all_boxes.view(N, cap, K, 4),
                "rois": rois.view(N, cap, 4), "roi_counts": counts.clamp(0, cap),
                "class_logits": class_logits, "box_regression": box_regression}

    @torch.no_grad()
    def forward_tapped(self, features: Dict[str, Tensor], proposals: List[Tensor], image_shapes: List[Tuple[int, int]], raster: bool = False):
        """``(detections, taps)``: the list of per-image dicts ``forward`` returns, and the spike taps of lif6 and lif7 (see
        FastRCNNPredictorSNNFull.forward_tapped; the groups of ``per_step`` / ``per_channel`` are the images), both from ONE head pass -
        the pass of spike-rate mode, whatever the head's ``spike_rates`` says."""
        if self.training:
            raise NotImplementedError("inference only: training the RoI heads is out of scope (DESIGN.md §7)")
        pool, head = self.box_roi_pool, self.box_head_and_predictor
        per_image = [p.shape[0] for p in proposals]
        if self._fuses_roi_align("forward_roialign_tapped"):
            feats, scales, rois, lvl = pool.assign(features, proposals, image_shapes)
            class_logits, box_regression, taps = head.forward_roialign_tapped(feats, scales, rois, lvl, raster=raster, rois_per_image=per_image)
        else:
            class_logits, box_regression, taps = head.forward_tapped(pool(features, proposals, image_shapes), raster=raster, rois_per_image=per_image)
        boxes, scores, labels, all_scores, all_boxes = self.postprocess_detections(class_logits, box_regression, proposals, image_shapes)
        result = [{"boxes": boxes[i], "labels": labels[i], "scores": scores[i], "all_scores": all_scores[i],
                   "all_boxes": all_boxes[i]} for i in range(len(boxes))]
        return result, taps

    def head_readouts(self, features: Dict[str, Tensor], proposals: List[Tensor], image_shapes: List[Tuple[int, int]], steps) -> dict:
        """the head call of ``forward`` with a readout per T_det of ``steps`` (one pass at steps[-1]; the fused RoIAlign path where
        ``forward`` takes it): {T_det: head output}"""
        pool, head = self.box_roi_pool, self.box_head_and_predictor
        if self._fuses_roi_align("forward_roialign_readouts"):
            feats, scales, rois, lvl = pool.assign(features, proposals, image_shapes)
            return head.forward_roialign_readouts(feats, scales, rois, lvl, steps)
        return head.forward_readouts(pool(features, proposals, image_shapes), steps)

    def head_outputs(self, features: Dict[str, Tensor], proposals: List[Tensor], image_shapes: List[Tuple[int, int]]):
        """the head call of ``forward`` alone: ``(class_logits [R, K], box_regression [R, K4])``, RoIs in the order of ``proposals`` (the
        fused RoIAlign path where ``forward`` takes it).  With ``train_readout`` on the head, grad mode on and a readout weight requiring
        grad, the two outputs carry a ``grad_fn`` (readout.py): a caller puts their own loss on them in eval mode and gets the exact
        gradients of ``cls_score.weight`` / ``bbox_pred.weight``; with ``train_fc7`` on the head and ``fc7.weight`` requiring grad the same
        graph also reaches ``fc7.weight`` through a SuperSpike lif7 (hidden.py), and with ``train_fc6`` and ``fc6.weight`` requiring grad
        ``fc6.weight`` through lif6 as well (fc6_grad.py).  ``model.train()`` stays refused."""
        if self.training:
            raise NotImplementedError("inference only: training the RoI heads is out of scope (DESIGN.md §7)")
        pool, head = self.box_roi_pool, self.box_head_and_predictor
        if getattr(head, "spike_rates", False):
            raise NotImplementedError("head_outputs: spike-rate mode returns rates, not outputs - use forward()")
        if self._fuses_roi_align("forward_roialign"):
            feats, scales, rois, lvl = pool.assign(features, proposals, image_shapes)
            return head.forward_roialign(feats, scales, rois, lvl)
        return head(pool(features, proposals, image_shapes))

    def check_targets(self, targets) -> None:
        """roi_heads.py:1025-1036 and the dtype checks of its forward (1190-1201): boxes float, labels int64"""
        if targets is None:
            raise ValueError("targets should not be None")
        if not all("boxes" in t for t in targets):
            raise ValueError("Every element of targets should have a boxes key")
        if not all("labels" in t for t in targets):
            raise ValueError("Every element of targets should have a labels key")
        for t in targets:
            if t["boxes"].dtype not in (torch.float, torch.double, torch.half):
                raise TypeError("target boxes must of float type, instead got %s" % t["boxes"].dtype)
            if t["labels"].dtype != torch.int64:
                raise TypeError("target labels must of int64 type, instead got %s" % t["labels"].dtype)

    def select_training_samples(self, proposals: List[Tensor], targets, generator=None):
        """roi_heads.py:1037-1073: the ground-truth boxes join the proposals, every box is matched (fg_iou_thresh / bg_iou_thresh, no
        low-quality matches) and encoded with the coder's weights in ONE losses.match_targets call, the sampler picks
        batch_size_per_image of them per image.  Returns ``(proposals, matched_idxs, labels, regression_targets)`` of the sampled boxes."""
        from . import losses
        self.check_targets(targets)
        dtype, device = proposals[0].dtype, proposals[0].device
        gt_boxes = [t["boxes"].to(device=device, dtype=dtype) for t in targets]
        gt_labels = [t["labels"].to(device) for t in targets]
        proposals = [torch.cat((p.detach(), g)) for p, g in zip(proposals, gt_boxes)]
        matched_idxs, labels, regression_targets = losses.match_targets(proposals, gt_boxes, gt_labels, self.fg_iou_thresh, self.bg_iou_thresh, False,
                                                                        self.box_coder.weights)
        pos, neg = losses.BalancedPositiveNegativeSampler(self.batch_size_per_image, self.positive_fraction)(labels, generator)
        out = ([], [], [], [])
        for i, (p, n) in enumerate(zip(pos, neg)):
            keep = torch.where(p | n)[0]
            for dst, src in zip(out, (proposals[i], matched_idxs[i].clamp(min=0), labels[i], regression_targets[i])):
                dst.append(src[keep])
        return out

    def head_losses(self, features: Dict[str, Tensor], proposals: List[Tensor], image_shapes: List[Tuple[int, int]], targets, generator=None):
        """the RoI heads' half of a readout fine-tuning step (roi_heads.py:1203-1245 in eval mode): select_training_samples,
        ``head_outputs`` on the sampled RoIs and losses.fastrcnn_loss -> {"loss_classifier", "loss_box_reg"}.  With ``train_readout`` on
        the head the two losses lead to cls_score.weight and bbox_pred.weight through autograd; with ``train_fc7`` on it (hidden.py; DESIGN.md
        4.15) the head's outputs carry a graph that also reaches fc7.weight, with ``train_fc6`` (fc6_grad.py) fc6.weight as well,
        and so do the two losses - no other code path is involved."""
        from . import losses
        if self.training:
            raise NotImplementedError("head_losses runs in eval mode: training the RoI heads is out of scope (DESIGN.md §7)")
        with torch.no_grad():
            proposals, _, labels, regression_targets = self.select_training_samples(proposals, targets, generator)
        class_logits, box_regression = self.head_outputs(features, proposals, image_shapes)
        if box_regression.shape[-1] != 4 * class_logits.shape[-1]:
            raise NotImplementedError("head_losses needs one box per class (only_one_bbox heads have no fastrcnn_loss in the reference either)")
        loss_classifier, loss_box_reg = losses.fastrcnn_loss(class_logits, box_regression, labels, regression_targets)
        return {"loss_classifier": loss_classifier, "loss_box_reg": loss_box_reg}

    def _fuses_roi_align(self, method: str) -> bool:
        """does the head call take the fused RoIAlign path: the head has ``method`` and the pool is the 7x7, sampling-2 RoIAlign
        the fused kernel restates"""
        pool, head = self.box_roi_pool, self.box_head_and_predictor
        return bool(self.fuse_roi_align and hasattr(head, method) and hasattr(pool, "assign")
                    and tuple(pool.output_size) == (7, 7) and pool.sampling_ratio == 2)

    def detections_from_head(self, head_out, proposals: List[Tensor], image_shapes: List[Tuple[int, int]]):
        """the part of ``forward`` after the head call: detections (or, in spike-rate mode, the head's rates)"""
        if getattr(self.box_head_and_predictor, "spike_rates", False):
            return head_out                                                          # roi_heads.py:1219-1223
        class_logits, box_regression = head_out
        boxes, scores, labels, all_scores, all_boxes = self.postprocess_detections(
            class_logits, box_regression, proposals, image_shapes)
        result = [{"boxes": boxes[i], "labels": labels[i], "scores": scores[i], "all_scores": all_scores[i],
                   "all_boxes": all_boxes[i]} for i in range(len(boxes))]
        return result, {}
