"""A small whole model for end-to-end fine-tuning tests (test infrastructure): a fixed 1x1 projection with average pools as the backbone, the
default anchors, RPNHeadSNN(32, 3, 8) and FastRCNNPredictorSNNFull(32 * 49, 64, 5, 8), weights scaled so that the heads spike - the model of
tests/test_gpu_head_losses.py's end-to-end test, kept here so that test files do not import each other."""
from collections import OrderedDict

import torch


class Transform(torch.nn.Module):
    def forward(self, images, targets=None):
        from snn_automotive_object_detection_amd.stock.anchors import ImageList
        return ImageList(torch.stack(list(images)), [tuple(int(s) for s in i.shape[-2:]) for i in images]), targets

    def postprocess(self, result, image_shapes, original_image_sizes):
        return result


class Backbone(torch.nn.Module):
    """five levels (strides 4 .. 64) of C channels: average pools of a fixed 1x1 projection, scaled so that the heads spike"""
    def __init__(self, C):
        super().__init__()
        self.proj = torch.nn.Conv2d(3, C, 1)

    def forward(self, x):
        y = self.proj(x) * 4.0
        return OrderedDict((str(l) if l < 4 else "pool", torch.nn.functional.avg_pool2d(y, 4 << l)) for l in range(5))


def small_model(dev, seed=0):
    """eval-mode GeneralizedRCNN on `dev` with train_readout set on both heads"""
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd.model import _default_anchorgen
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    torch.manual_seed(seed)
    C = 32
    head = S.RPNHeadSNN(C, 3, 8)
    rpn = S.RegionProposalNetwork(_default_anchorgen(), head, 0.7, 0.3, 64, 0.5, dict(training=40, testing=20), dict(training=30, testing=10), 0.7)
    pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    det = S.FastRCNNPredictorSNNFull(C * 49, 64, 5, 8)
    roi = S.RoIHeadsSNN(pool, det, 0.5, 0.5, 32, 0.25, None, 0.05, 0.5, 10)
    with torch.no_grad():
        for m in (head.shared_conv, head.conv_cls, head.conv_bbox, det.fc6, det.fc7, det.cls_score, det.bbox_pred):
            m.weight.mul_(8.0)
    model = S.GeneralizedRCNN(Backbone(C), rpn, roi, Transform()).to(dev).eval()
    head.train_readout = det.train_readout = True
    return model


def targets(dev):
    return [{"boxes": torch.tensor([[8.0, 8.0, 40.0, 44.0], [30.0, 20.0, 60.0, 50.0]], device=dev), "labels": torch.tensor([1, 3], device=dev)},
            {"boxes": torch.tensor([[4.0, 10.0, 30.0, 30.0]], device=dev), "labels": torch.tensor([2], device=dev)}]
