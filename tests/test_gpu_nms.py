"""HIP batched NMS against the greedy definition (loop reference on the host)."""
import pytest
import torch

from snn_automotive_object_detection_amd.stock import boxes as B

pytestmark = pytest.mark.gpu


def _greedy(boxes, scores, idxs, thr):
    order = scores.argsort(descending=True, stable=True).tolist()
    iou = B.box_iou(boxes, boxes).double()                     # float IoU against the double threshold, as the parity target compares
    keep = []
    while order:
        i = order.pop(0)
        keep.append(i)
        order = [j for j in order if not (iou[i, j] > thr and idxs[i] == idxs[j])]
    return torch.tensor(keep, dtype=torch.int64)


@pytest.mark.parametrize("n,ncat,thr", [(1, 1, 0.5), (63, 1, 0.5), (64, 2, 0.7), (65, 3, 0.3), (700, 5, 0.7), (2000, 1, 0.5)])
def test_hip_batched_nms_equals_greedy(gpu_device, n, ncat, thr):
    from snn_automotive_object_detection_amd import ops
    g = torch.Generator().manual_seed(n)
    xy = torch.rand((n, 2), generator=g) * 300
    wh = torch.rand((n, 2), generator=g) * 80 + 1
    boxes = torch.cat([xy, xy + wh], dim=1)
    scores = torch.rand((n,), generator=g)
    idxs = torch.randint(0, ncat, (n,), generator=g)
    exp = _greedy(boxes, scores, idxs, thr)
    got = ops.batched_nms(boxes.to(gpu_device), scores.to(gpu_device), idxs.to(gpu_device), thr).cpu()
    assert torch.equal(got, exp)
    top = ops.batched_nms(boxes.to(gpu_device), scores.to(gpu_device), idxs.to(gpu_device), thr, max_keep=7).cpu()
    assert torch.equal(top, exp[:7])
    # the stock dispatcher routes GPU tensors here and CPU tensors to the plain-torch form: same answer
    assert torch.equal(B.batched_nms(boxes.to(gpu_device), scores.to(gpu_device), idxs.to(gpu_device), thr).cpu(),
                       B.batched_nms(boxes, scores, idxs, thr))


def _greedy_vec(boxes, scores, idxs, thr):
    """the same greedy definition with one vector operation per candidate (for the large cases)"""
    order = scores.argsort(descending=True, stable=True)
    b, c = boxes[order], idxs[order]
    iou = B.box_iou(b, b).double()
    sup = (iou > thr) & (c[:, None] == c[None, :])
    alive = torch.ones(len(order), dtype=torch.bool)
    keep = []
    for i in range(len(order)):
        if alive[i]:
            keep.append(i)
            alive &= ~sup[i]
    return order[torch.tensor(keep, dtype=torch.int64)]


@pytest.mark.parametrize("n,ncat", [(4768, 5), (9984, 4), (10500, 3)])
def test_hip_nms_large_and_keep_mask(gpu_device, n, ncat):
    """RPN-sized candidate sets (double-buffered scan) and one past the double-buffer limit (single buffer)"""
    from snn_automotive_object_detection_amd import ops
    g = torch.Generator().manual_seed(n)
    xy = torch.rand((n, 2), generator=g) * 1500
    wh = torch.rand((n, 2), generator=g) * 120 + 1
    boxes = torch.cat([xy, xy + wh], dim=1)
    scores = torch.rand((n,), generator=g)
    idxs = torch.randint(0, ncat, (n,), generator=g)
    exp = _greedy_vec(boxes, scores, idxs, 0.7)
    got = ops.batched_nms(boxes.to(gpu_device), scores.to(gpu_device), idxs.to(gpu_device), 0.7).cpu()
    assert torch.equal(got, exp)
    top = ops.batched_nms(boxes.to(gpu_device), scores.to(gpu_device), idxs.to(gpu_device), 0.7, max_keep=1000).cpu()
    assert torch.equal(top, exp[:1000])
    order, kept = ops.nms_keep_mask(boxes.to(gpu_device), scores.to(gpu_device), idxs.to(gpu_device), 0.7)
    assert torch.equal(order[kept].cpu(), exp)


@pytest.mark.parametrize("n,clusters", [(220, 12), (1000, 25), (4000, 60)])
def test_hip_nms_on_clustered_boxes(gpu_device, n, clusters):
    """boxes piled on a few objects: suppression rows are dense, so a kept box often suppresses candidate 31 of its own
    64-candidate chunk - the case in which the scan once sign-extended the low mask word into the upper 32 candidates
    (found in round 2 by the reference-pinned post-processing fixtures; random boxes rarely hit it)"""
    from snn_automotive_object_detection_amd import ops
    from oracle import torchvision_restated as TV
    g = torch.Generator().manual_seed(n + clusters)
    c = torch.rand((clusters, 2), generator=g) * 1200 + 100
    which = torch.arange(n) % clusters
    ctr = c[which] + (torch.rand((n, 2), generator=g) - 0.5) * 14
    wh = (60 + 140 * torch.rand((clusters, 2), generator=g))[which] * (0.9 + 0.2 * torch.rand((n, 2), generator=g))
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    scores = torch.rand((n,), generator=g)
    exp = TV.nms(boxes, scores, 0.5)                            # numpy greedy loop (torchvision's CPU kernel restated)
    got = ops.batched_nms(boxes.to(gpu_device), scores.to(gpu_device), torch.zeros(n, dtype=torch.int64, device=gpu_device), 0.5).cpu()
    assert torch.equal(got, exp), (len(got), len(exp))
