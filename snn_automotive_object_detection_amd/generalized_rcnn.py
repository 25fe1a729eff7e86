"""``GeneralizedRCNN`` with the reference's signature (/root/reference/generalized_rcnn.py:15-170,
inference side): transform -> backbone (no_grad) -> rpn -> roi_heads -> postprocess; in eval the per-image
``proposals`` / ``objectness`` of the RPN are merged into the detections (125-132) and ``all_boxes`` /
``proposals`` are mapped back to the original image size (146-170)."""
from collections import OrderedDict
from typing import Dict, List, Tuple

import torch
from torch import nn, Tensor

from .stock.transform import resize_boxes


class GeneralizedRCNN(nn.Module):
    def __init__(self, backbone: nn.Module, rpn: nn.Module, roi_heads: nn.Module, transform: nn.Module) -> None:
        super().__init__()
        self.transform = transform
        self.backbone = backbone
        self.rpn = rpn
        self.roi_heads = roi_heads

    @torch.no_grad()
    def forward(self, images: List[Tensor], targets=None):
        if self.training:
            raise NotImplementedError("inference only (call .eval()): training is out of scope (DESIGN.md §7)")
        original_image_sizes = [(int(img.shape[-2]), int(img.shape[-1])) for img in images]
        images, targets = self.transform(images, targets)
        features = self.backbone(images.tensors)                                    # generalized_rcnn.py:93-94
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        head = getattr(self.rpn, "head", None)
        if getattr(head, "spike_rates", False):                                     # spike-rate path, 98-111: ONE head call;
            proposals, rpn_rates = self.rpn(images, features, targets)              # the RPN hands the head's rates on (rpn.py:698-701)
            det_rates = self.roi_heads(features, proposals, images.image_sizes, targets)
            return list(rpn_rates) + list(det_rates)
        proposals, proposal_extras = self.rpn(images, features, targets)            # :114
        detections, _ = self.roi_heads(features, proposals, images.image_sizes, targets)   # :118
        return self.finish_detections(detections, proposal_extras, images.image_sizes, original_image_sizes)

    @torch.no_grad()
    def forward_padded(self, images: List[Tensor]) -> Dict[str, Tensor]:
        """``forward`` with fixed shapes: transform -> backbone -> static.heads_padded (both heads, proposal selection,
        RoI assignment, detection post-processing: no host synchronisation from the FPN features on) -> boxes / all_boxes / proposals
        back in the original image sizes.  Returns the dict of padded tensors static.heads_padded documents; ``static.unpad`` turns it
        into what ``forward`` returns, with the one host synchronisation.  ``rois`` stay in the coordinates of the resized images."""
        from . import static
        if self.training:
            raise NotImplementedError("inference only (call .eval()): training is out of scope (DESIGN.md §7)")
        original_image_sizes = [(int(img.shape[-2]), int(img.shape[-1])) for img in images]
        images, _ = self.transform(images, None)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        out = static.heads_padded(self, features, images)
        scale = self._resize_ratios(images.image_sizes, original_image_sizes, out["boxes"].device)      # [N, 1, 4]: (rw, rh, rw, rh)
        out["boxes"] = out["boxes"] * scale
        out["all_boxes"] = out["all_boxes"] * scale[:, :, None, :]
        out["proposals"] = out["proposals"] * scale
        return out

    @torch.no_grad()
    def forward_tapped(self, images: List[Tensor], raster: bool = False):
        """``(detections, taps)``: what ``forward`` returns, and ``taps = {"rpn": ..., "det": ...}`` - the spike taps of the hidden LIF
        layers of both heads (RPNHeadSNN.forward_tapped, RoIHeadsSNN.forward_tapped) - from the SAME two head passes.  The passes are
        those of spike-rate mode, so ``energy.rates_from_taps(taps)`` gives its rate rows as well: one detection pass yields detections
        and the energy report.  The heads' ``spike_rates`` attributes are not touched."""
        if self.training:
            raise NotImplementedError("inference only (call .eval()): training is out of scope (DESIGN.md §7)")
        original_image_sizes = [(int(img.shape[-2]), int(img.shape[-1])) for img in images]
        images, _ = self.transform(images, None)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        feats = list(features.values())
        logits, bbox_reg, rpn_taps = self.rpn.head.forward_tapped(feats, raster=raster)
        proposals, proposal_extras = self.rpn.proposals_from_head(images, feats, (logits, bbox_reg))
        detections, det_taps = self.roi_heads.forward_tapped(features, proposals, images.image_sizes, raster=raster)
        detections = self.finish_detections(detections, proposal_extras, images.image_sizes, original_image_sizes)
        return detections, {"rpn": rpn_taps, "det": det_taps}

    def readout_losses(self, images: List[Tensor], targets: List[Dict[str, Tensor]], generator=None) -> Dict[str, Tensor]:
        """the reference's training forward for the READOUTS (generalized_rcnn.py:60-123 with self.training), in eval mode:
        transform and backbone under no_grad, then RegionProposalNetwork.head_losses and RoIHeadsSNN.head_losses - target matching and the
        fused losses on the GPU (losses.py).  Returns the reference's dict: loss_objectness, loss_rpn_box_reg, loss_classifier,
        loss_box_reg.  With ``train_readout`` on both heads (and readout.freeze_hidden) ``sum(losses.values()).backward()`` gives the four
        readout weights their exact gradients; nothing else receives one - unless the box predictor also has ``train_fc7`` set (with
        hidden.freeze_below_fc7): the detector head's outputs then carry a graph that reaches ``fc7.weight`` too, and the same
        ``backward()`` leaves its SuperSpike gradient there (hidden.py); with ``train_fc6`` (and fc6_grad.freeze_below_fc6) the
        graph reaches ``fc6.weight`` as well (fc6_grad.py).  Proposals are selected with the "training" entries of the
        RPN's two top-n dicts.  ``generator``: the torch.Generator of both samplers.  ``forward`` in training mode still raises."""
        if self.training:
            raise NotImplementedError("readout_losses runs in eval mode: model.train() is out of scope (DESIGN.md §7)")
        self.roi_heads.check_targets(targets)
        for i, t in enumerate(targets):                                             # generalized_rcnn.py:62-77
            b = t["boxes"]
            if not isinstance(b, torch.Tensor) or b.dim() != 2 or b.shape[-1] != 4:
                raise ValueError("Expected target boxes to be a tensor of shape [N, 4], got %s" % (tuple(b.shape) if isinstance(b, torch.Tensor) else type(b),))
        with torch.no_grad():
            images, targets = self.transform(images, targets)
            features = self.backbone(images.tensors)
            if isinstance(features, torch.Tensor):
                features = OrderedDict([("0", features)])
        feats = list(features.values())
        head_out, losses = self.rpn.head_losses(images, features, targets, generator)
        with torch.no_grad():
            proposals, _ = self.rpn.proposals_from_head(images, feats, head_out, top_n="training")
        losses.update(self.roi_heads.head_losses(features, proposals, images.image_sizes, targets, generator))
        return {k: losses[k] for k in ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")}

    def _resize_ratios(self, image_sizes, original_image_sizes, device) -> Tensor:
        """resize_boxes' ratios (fp32 new / old, as it forms them) of every image as one device tensor; uploaded once per set of sizes"""
        cache = self.__dict__.setdefault("_ratio_cache", {})
        key = (tuple(map(tuple, image_sizes)), tuple(map(tuple, original_image_sizes)), str(device))
        if key not in cache:
            if len(cache) >= 64:
                cache.clear()
            rows = []
            for im_s, o_im_s in zip(image_sizes, original_image_sizes):
                rh, rw = [torch.tensor(orig, dtype=torch.float32) / torch.tensor(resized, dtype=torch.float32) for orig, resized in zip(o_im_s, im_s)]
                rows.append(torch.stack((rw, rh, rw, rh)))
            cache[key] = torch.stack(rows)[:, None, :].to(device)
        return cache[key]

    def finish_detections(self, detections, proposal_extras, image_sizes, original_image_sizes):
        """the end of ``forward`` (generalized_rcnn.py:119-132): back to the original sizes, the RPN's extras merged in"""
        detections = self.transform.postprocess(detections, image_sizes, original_image_sizes)
        for i in range(len(detections)):                                            # :125-129
            for k, v in proposal_extras[i].items():
                detections[i][k] = v
        if detections and "all_boxes" in detections[0]:
            detections = self.postprocess(detections, image_sizes, original_image_sizes)
        return detections

    def postprocess(self, result: List[Dict[str, Tensor]], image_shapes: List[Tuple[int, int]],
                    original_image_sizes: List[Tuple[int, int]]) -> List[Dict[str, Tensor]]:
        for i, (pred, im_s, o_im_s) in enumerate(zip(result, image_shapes, original_image_sizes)):
            boxes = pred["all_boxes"]
            shape = boxes.shape
            result[i]["all_boxes"] = resize_boxes(boxes.reshape(shape[0] * shape[1], -1), im_s, o_im_s).reshape(*shape)
            if "proposals" in pred:
                result[i]["proposals"] = resize_boxes(pred["proposals"], im_s, o_im_s)
        return result
