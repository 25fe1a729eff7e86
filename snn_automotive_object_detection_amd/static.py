"""The static-shape, sync-free path from FPN features to padded detections.

``heads_padded``  RPN head -> snn_rpn_proposals -> snn_roi_assign -> the fused RoIAlign detector head on N * cap rows ->
                  snn_det_postprocess_padded: every per-image count stays in device memory, every shape depends on the configuration
                  alone, nothing waits for the host.
``unpad``         the one host synchronisation: padded tensors -> the list of per-image dicts ``model(images)`` returns.

The list API (``GeneralizedRCNN.forward``, ``StreamPipeline``) is the reference's and does not come through here."""
from typing import Dict, List

import torch
from torch import Tensor


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
