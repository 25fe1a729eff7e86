"""The reference's time-step study (metrics_for_different_timesteps.py: T_rpn x T_det, every pair a freshly built model run
over the data) from one backbone pass and one head pass per T_rpn.  The SNN heads are causal and start from zero state, so the
outputs of a T'-step forward are the first T' steps of a longer pass: the heads' readout launches (include/snn_hip.h,
snn_*_readouts) give every T' of a pass at once."""
from collections import OrderedDict

import torch

from . import ops


@torch.no_grad()
def timestep_sweep(model, images, t_rpn_steps, t_det_steps):
    """{(T_rpn, T_det): what ``model`` (a GeneralizedRCNN of create_model) returns for those step counts} - detections, or the
    rate list when its heads are in spike-rate mode.  Runs the transform and backbone once, the RPN head once at max T_rpn,
    then per T_rpn the proposal selection and one detector head pass at max T_det, then per T_det the detection
    post-processing.  The model's ``num_steps`` are not touched."""
    t_rpn_steps, t_det_steps = ops.check_steps(sorted(t_rpn_steps)), ops.check_steps(sorted(t_det_steps))
    if model.training:
        raise NotImplementedError("inference only (call .eval())")
    original_image_sizes = [(int(img.shape[-2]), int(img.shape[-1])) for img in images]
    images, _ = model.transform(images, None)
    features = model.backbone(images.tensors)
    if isinstance(features, torch.Tensor):
        features = OrderedDict([("0", features)])
    feats = list(features.values())
    rpn, roi_heads = model.rpn, model.roi_heads
    rates_mode = getattr(rpn.head, "spike_rates", False)
    rpn_out = rpn.head.forward_readouts(feats, t_rpn_steps)
    out = {}
    for t_rpn in t_rpn_steps:
        proposals, extras = rpn.proposals_from_head(images, feats, rpn_out[t_rpn])
        det_out = roi_heads.head_readouts(features, proposals, images.image_sizes, t_det_steps)
        for t_det in t_det_steps:
            res = roi_heads.detections_from_head(det_out[t_det], proposals, images.image_sizes)
            if rates_mode:
                out[(t_rpn, t_det)] = list(extras) + list(res)
                continue
            detections, _ = res
            out[(t_rpn, t_det)] = model.finish_detections(detections, extras, images.image_sizes, original_image_sizes)
    return out
