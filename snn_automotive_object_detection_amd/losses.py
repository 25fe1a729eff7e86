"""Readout fine-tuning, from the head outputs to a scalar (include/snn_hip.h: snn_match_targets, snn_rpn_loss_grad, snn_det_loss_grad;
DESIGN.md 4.14): what the reference's training forward does between the heads and ``backward()`` - ``assign_targets_to_anchors`` /
``assign_targets_to_proposals``, ``BoxCoder.encode``, the sampler, ``compute_loss`` and ``fastrcnn_loss`` - for the readouts only.

Matching, labels and encoded targets are one call for all images (a thread owns a box, the ground truth sits in LDS; no G x B IoU matrix);
each loss is one fused call that also writes the gradient with respect to the head outputs, kept for ``backward``.  The losses are
``torch.autograd.Function``s whose gradients chain into ``readout.ReadoutGrad`` through plain autograd: with ``train_readout`` on the heads
a fine-tuning step of the four readout weights is

    losses = model.readout_losses(images, targets)
    sum(losses.values()).backward()
    optimiser.step()

The three calls enqueue on the current stream and synchronise nothing.  Sampling stays torch's ``randperm`` (its ``torch.where`` waits for
the device, before the head it samples for runs).  Hidden-layer gradients, surrogate functions and ``model.train()`` stay out."""
import ctypes as C
import warnings
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib, ops
from ._lib import snn_rpn_level

MAX_GT = 256                                 # LS_MAX_GT: ground-truth boxes per image of snn_match_targets
MAX_IMAGES = 64                              # LS_MAX_IMAGES

_WS_LOSS = ops._Workspace()                  # scratch of the three calls (stream-ordered; never the heads' workspace)
_WARNED = set()


# ---------------------------------------------------------------------------------------------
# stock-torch statements of the same steps (images outside the C limits; the yardstick of the tests)
# ---------------------------------------------------------------------------------------------
def encode_boxes(reference_boxes: Tensor, proposals: Tensor, weights) -> Tensor:
    """torchvision's ``encode_boxes``, operation by operation"""
    wx, wy, ww, wh = weights
    px1, py1, px2, py2 = [proposals[:, i].unsqueeze(1) for i in range(4)]
    gx1, gy1, gx2, gy2 = [reference_boxes[:, i].unsqueeze(1) for i in range(4)]
    ex_w, ex_h = px2 - px1, py2 - py1
    ex_cx, ex_cy = px1 + 0.5 * ex_w, py1 + 0.5 * ex_h
    gt_w, gt_h = gx2 - gx1, gy2 - gy1
    gt_cx, gt_cy = gx1 + 0.5 * gt_w, gy1 + 0.5 * gt_h
    return torch.cat((wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * torch.log(gt_w / ex_w), wh * torch.log(gt_h / ex_h)), dim=1)


def matcher(match_quality_matrix: Tensor, high: float, low: float, allow_low_quality: bool) -> Tensor:
    """torchvision's ``Matcher.__call__`` on a [G, B] quality matrix with G >= 1: int64 [B], -1 below ``low``, -2 between"""
    vals, matches = match_quality_matrix.max(dim=0)
    all_matches = matches.clone()
    below, between = vals < low, (vals >= low) & (vals < high)
    matches[below] = -1
    matches[between] = -2
    if allow_low_quality:
        best_of_gt, _ = match_quality_matrix.max(dim=1)
        upd = torch.where(match_quality_matrix == best_of_gt[:, None])[1]
        matches[upd] = all_matches[upd]
    return matches


def _match_stock(boxes: Tensor, gt: Tensor, gt_labels: Optional[Tensor], high, low, allow_low_quality, weights):
    from .stock.boxes import box_iou
    B = boxes.shape[0]
    if gt.shape[0] == 0:
        idx = torch.zeros(B, dtype=torch.int64, device=boxes.device)
        lab = torch.zeros(B, dtype=torch.int64, device=boxes.device)
        ref = torch.zeros_like(boxes)
    else:
        idx = matcher(box_iou(gt, boxes), high, low, allow_low_quality)
        lab = torch.ones_like(idx) if gt_labels is None else gt_labels[idx.clamp(min=0)].to(torch.int64)
        lab = torch.where(idx == -1, torch.zeros_like(lab), lab)
        lab = torch.where(idx == -2, torch.full_like(lab, -1), lab)
        ref = gt[idx.clamp(min=0)]
    return idx, lab, encode_boxes(ref, boxes, weights)


# ---------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------
def _boxes_list(xs, what: str) -> List[Tensor]:
    xs = list(xs)
    for x in xs:
        if not isinstance(x, Tensor) or x.dim() != 2 or x.shape[1] != 4:
            raise ValueError("%s: a list of [n, 4] tensors expected, got %s" % (what, tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__))
    return xs


def _starts(counts):
    s = [0]
    for c in counts:
        s.append(s[-1] + int(c))
    return (C.c_int64 * len(s))(*s)


def match_targets_raw(boxes: Tensor, box_counts: Sequence[int], gt_boxes: Tensor, gt_labels: Optional[Tensor], gt_counts: Sequence[int],
                      high: float, low: float, allow_low_quality: bool, weights, out=None):
    """one snn_match_targets call on concatenated tensors: boxes [sum B_n, 4] fp32, gt_boxes [sum G_n, 4] fp32, gt_labels [sum G_n] int64 or
    None (RPN mode) -> (matched_idx [sum B_n] int32, label int32, reg_target [sum B_n, 4] fp32); ``out``: write into these three"""
    ops._need_gpu(boxes, "boxes")
    lib = _lib.load()
    N, total = len(box_counts), int(boxes.shape[0])
    if len(gt_counts) != N:
        raise ValueError("match_targets: %d images of boxes, %d of ground truth" % (N, len(gt_counts)))
    if sum(box_counts) != total or sum(gt_counts) != int(gt_boxes.shape[0]):
        raise ValueError("match_targets: the per-image counts do not add up to the rows given")
    boxes, gt_boxes = ops._f32c(boxes), ops._f32c(gt_boxes)
    if gt_labels is not None:
        gt_labels = gt_labels.detach().to(torch.int64).contiguous()
        if gt_labels.shape[0] != gt_boxes.shape[0]:
            raise ValueError("match_targets: %d labels for %d ground-truth boxes" % (gt_labels.shape[0], gt_boxes.shape[0]))
    dev = boxes.device
    if out is None:
        out = (torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev),
               torch.empty((total, 4), dtype=torch.float32, device=dev))
    idx, lab, tgt = out
    scratch = _WS_LOSS.get(dev, max(16, lib.snn_match_targets_workspace_bytes(total, N)))
    w = (C.c_float * 4)(*[float(x) for x in weights])
    _lib.check(lib.snn_match_targets(ops._ptr(boxes), _starts(box_counts), ops._ptr(gt_boxes) if gt_boxes.numel() else None, ops._ptr(gt_labels),
                                     _starts(gt_counts), N, float(high), float(low), int(bool(allow_low_quality)), w, ops._ptr(idx), ops._ptr(lab),
                                     ops._ptr(tgt), ops._ptr(scratch), scratch.numel(), ops._stream()), "snn_match_targets")
    return idx, lab, tgt


@ops._on_tensor_device
def match_targets(boxes: Sequence[Tensor], gt_boxes: Sequence[Tensor], gt_labels: Optional[Sequence[Tensor]], high: float, low: float,
                  allow_low_quality: bool, weights=(1.0, 1.0, 1.0, 1.0)):
    """per-image lists ``(matched_idxs, labels, regression_targets)`` for per-image lists of boxes (anchors or proposals) and ground truth:
    torchvision's Matcher on box_iou, the labels of ``assign_targets_to_anchors`` (``gt_labels`` None: float32 1 / 0 / -1) or
    ``assign_targets_to_proposals`` (int64 class / 0 / -1), and ``BoxCoder(weights).encode`` of the matched ground-truth box.
    ``matched_idxs`` is int64 and keeps -1 (below ``low``) and -2 (between): clamp it as the reference does where an index is needed.
    An image without ground truth: indices 0, labels 0, the encoding of the zero box.  One call for all images; an image with more than
    256 ground-truth boxes (or more than 64 images) sends the call down the stock-torch statement of the same steps, with one RuntimeWarning."""
    boxes, gt_boxes = _boxes_list(boxes, "boxes"), _boxes_list(gt_boxes, "gt_boxes")
    if len(boxes) != len(gt_boxes) or (gt_labels is not None and len(gt_labels) != len(boxes)):
        raise ValueError("match_targets: one entry per image in boxes, gt_boxes and gt_labels")
    if not boxes:
        return [], [], []
    bc, gc = [int(b.shape[0]) for b in boxes], [int(g.shape[0]) for g in gt_boxes]
    rpn_mode = gt_labels is None
    why = None
    if max(gc) > MAX_GT:
        why = "%d ground-truth boxes in an image (HIP path: <= %d)" % (max(gc), MAX_GT)
    elif len(boxes) > MAX_IMAGES:
        why = "%d images (HIP path: <= %d)" % (len(boxes), MAX_IMAGES)
    if why is not None:
        if why not in _WARNED:
            _WARNED.add(why)
            warnings.warn("match_targets falls back to the stock torch ops (%s)" % why, RuntimeWarning)
        res = [_match_stock(b.detach().float(), g.detach().float().to(b.device), None if rpn_mode else gt_labels[i].to(b.device), high, low,
                            allow_low_quality, weights) for i, (b, g) in enumerate(zip(boxes, gt_boxes))]
        idx, lab, tgt = [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
        return idx, ([l.to(torch.float32) for l in lab] if rpn_mode else lab), tgt
    dev = boxes[0].device
    idx, lab, tgt = match_targets_raw(torch.cat(boxes, 0), bc, torch.cat([g.to(dev) for g in gt_boxes], 0),
                                      None if rpn_mode else torch.cat([l.to(dev) for l in gt_labels], 0), gc, high, low, allow_low_quality, weights)
    lab = lab.to(torch.float32 if rpn_mode else torch.int64)
    return list(idx.to(torch.int64).split(bc)), list(lab.split(bc)), list(tgt.split(bc))


# ---------------------------------------------------------------------------------------------
# sampler (stock torch: randperm)
# ---------------------------------------------------------------------------------------------
class BalancedPositiveNegativeSampler:
    """torchvision's sampler: per image up to ``batch_size_per_image`` elements, at most ``positive_fraction`` of them positive (label >= 1),
    the rest negative (label == 0), chosen with ``torch.randperm``; returns per-image uint8 masks ``(pos, neg)``.  ``generator``: the
    torch.Generator of the permutations (None: the default generator of the labels' device)"""

    def __init__(self, batch_size_per_image: int, positive_fraction: float, generator: Optional[torch.Generator] = None):
        self.batch_size_per_image, self.positive_fraction, self.generator = batch_size_per_image, positive_fraction, generator

    def __call__(self, matched_idxs: Sequence[Tensor], generator: Optional[torch.Generator] = None) -> Tuple[List[Tensor], List[Tensor]]:
        gen = generator if generator is not None else self.generator
        pos_idx, neg_idx = [], []
        for m in matched_idxs:
            positive, negative = torch.where(m >= 1)[0], torch.where(m == 0)[0]
            num_pos = min(positive.numel(), int(self.batch_size_per_image * self.positive_fraction))
            num_neg = min(negative.numel(), self.batch_size_per_image - num_pos)
            perm1 = torch.randperm(positive.numel(), device=positive.device, generator=gen)[:num_pos]
            perm2 = torch.randperm(negative.numel(), device=negative.device, generator=gen)[:num_neg]
            pos_mask, neg_mask = torch.zeros_like(m, dtype=torch.uint8), torch.zeros_like(m, dtype=torch.uint8)
            pos_mask[positive[perm1]] = 1
            neg_mask[negative[perm2]] = 1
            pos_idx.append(pos_mask)
            neg_idx.append(neg_mask)
        return pos_idx, neg_idx


# ---------------------------------------------------------------------------------------------
# the two losses
# ---------------------------------------------------------------------------------------------
def rpn_loss_grad(shapes: Sequence[Sequence[int]], A: int, logits: Tensor, deltas: Tensor, label: Tensor, sampled: Tensor, reg_target: Tensor,
                  out=None):
    """one snn_rpn_loss_grad call: shapes = (N, H, W) per level, logits [P, A] / deltas [P, 4A] in the head's row order, label int32 /
    sampled uint8 / reg_target [., 4] per anchor in the reference's order -> (loss [2], g_logits [P, A], g_deltas [P, 4A])"""
    N = int(shapes[0][0])
    P = sum(int(n) * int(h) * int(w) for n, h, w in shapes)
    if tuple(logits.shape) != (P, A) or tuple(deltas.shape) != (P, 4 * A):
        raise ValueError("rpn_loss: logits [%d, %d] and deltas [%d, %d] expected, got %s and %s" % (P, A, P, 4 * A, tuple(logits.shape), tuple(deltas.shape)))
    if label.numel() != P * A or sampled.numel() != P * A or tuple(reg_target.shape) != (P * A, 4):
        raise ValueError("rpn_loss: %d anchors, got %d labels, %d sampled flags and targets %s" % (P * A, label.numel(), sampled.numel(), tuple(reg_target.shape)))
    if label.dtype != torch.int32 or sampled.dtype != torch.uint8:
        raise ValueError("rpn_loss: label must be int32 and sampled uint8")
    ops._need_gpu(logits, "logits")
    lib = _lib.load()
    logits, deltas, reg_target = ops._f32c(logits), ops._f32c(deltas), ops._f32c(reg_target)
    label, sampled = label.contiguous(), sampled.contiguous()
    dev = logits.device
    if out is None:
        out = (torch.empty(2, dtype=torch.float32, device=dev), torch.empty_like(logits), torch.empty_like(deltas))
    loss, g_l, g_d = out
    lv = (snn_rpn_level * len(shapes))(*[snn_rpn_level(None, int(n), int(h), int(w), 0) for n, h, w in shapes])
    scratch = _WS_LOSS.get(dev, max(16, lib.snn_rpn_loss_grad_workspace_bytes(P * A)))
    _lib.check(lib.snn_rpn_loss_grad(lv, len(shapes), int(A), N, ops._ptr(logits), ops._ptr(deltas), ops._ptr(label), ops._ptr(sampled),
                                     ops._ptr(reg_target), ops._ptr(loss), ops._ptr(g_l), ops._ptr(g_d), ops._ptr(scratch), scratch.numel(),
                                     ops._stream()), "snn_rpn_loss_grad")
    return loss, g_l, g_d


def det_loss_grad(logits: Tensor, box: Tensor, label: Tensor, reg_target: Tensor, out=None):
    """one snn_det_loss_grad call: logits [R, K], box [R, 4K], label [R] int32 (-1: row left out), reg_target [R, 4] ->
    (loss [2], g_logits [R, K], g_box [R, 4K])"""
    if logits.dim() != 2 or box.dim() != 2 or box.shape[0] != logits.shape[0]:
        raise ValueError("fastrcnn_loss: class_logits [R, K] and box_regression [R, 4K] expected, got %s and %s" % (tuple(logits.shape), tuple(box.shape)))
    R, K = int(logits.shape[0]), int(logits.shape[1])
    if label.numel() != R or tuple(reg_target.shape) != (R, 4):
        raise ValueError("fastrcnn_loss: %d rows, got %d labels and targets %s" % (R, label.numel(), tuple(reg_target.shape)))
    if label.dtype != torch.int32:
        raise ValueError("fastrcnn_loss: label must be int32 here")
    if R < 1:
        raise ValueError("fastrcnn_loss: no rows")
    ops._need_gpu(logits, "class_logits")
    lib = _lib.load()
    logits, box, reg_target, label = ops._f32c(logits), ops._f32c(box), ops._f32c(reg_target), label.contiguous()
    dev = logits.device
    if out is None:
        out = (torch.empty(2, dtype=torch.float32, device=dev), torch.empty_like(logits), torch.empty_like(box))
    loss, g_l, g_b = out
    scratch = _WS_LOSS.get(dev, max(16, lib.snn_det_loss_grad_workspace_bytes(R, K)))
    _lib.check(lib.snn_det_loss_grad(ops._ptr(logits), ops._ptr(box), ops._ptr(label), ops._ptr(reg_target), R, K, int(box.shape[1]), ops._ptr(loss),
                                     ops._ptr(g_l), ops._ptr(g_b), ops._ptr(scratch), scratch.numel(), ops._stream()), "snn_det_loss_grad")
    return loss, g_l, g_b


def _level_rows(levels: Sequence[Tensor], width: int) -> Tensor:
    """per-level NCHW tensors [N, width, H, W] -> the head's row buffer [P, width] (level-major, then n, y, x).  The head returns views of
    exactly such a buffer: then this is that buffer again, no copy; anything else is gathered"""
    first = levels[0]
    ptr, ok = first.data_ptr(), True
    for t in levels:
        n, w, h, x = t.shape
        ok = ok and t.dtype == torch.float32 and t.data_ptr() == ptr and t.stride() == (h * x * w, 1, x * w, w) and w == width
        ptr += n * w * h * x * 4
    P = sum(t.shape[0] * t.shape[2] * t.shape[3] for t in levels)
    if ok and first.untyped_storage().nbytes() - first.storage_offset() * 4 >= P * width * 4:
        return first.detach().as_strided((P, width), (width, 1))
    return torch.cat([t.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(-1, width) for t in levels], 0)


def _level_views(rows: Tensor, shapes, width: int) -> List[Tensor]:
    out, pos = [], 0
    for n, h, w in shapes:
        out.append(rows[pos:pos + n * h * w].view(n, h, w, width).permute(0, 3, 1, 2))
        pos += n * h * w
    return out


class _RpnLoss(torch.autograd.Function):
    """(objectness loss, box loss) of the per-level head outputs; forward is the fused call and keeps the gradient rows"""

    @staticmethod
    def forward(ctx, L, label, sampled, reg_target, *levels):
        objectness, deltas = levels[:L], levels[L:]
        A = int(objectness[0].shape[1])
        shapes = [(int(o.shape[0]), int(o.shape[2]), int(o.shape[3])) for o in objectness]
        loss, g_l, g_d = rpn_loss_grad(shapes, A, _level_rows(objectness, A), _level_rows(deltas, 4 * A), label, sampled, reg_target)
        ctx.g, ctx.shapes, ctx.A, ctx.L = (g_l, g_d), shapes, A, L
        return loss[0].clone(), loss[1].clone()

    @staticmethod
    def backward(ctx, d_obj, d_box):
        (g_l, g_d), L = ctx.g, ctx.L
        need = ctx.needs_input_grad[4:]
        gl = _level_views(g_l * d_obj, ctx.shapes, ctx.A) if d_obj is not None and any(need[:L]) else [None] * L
        gd = _level_views(g_d * d_box, ctx.shapes, 4 * ctx.A) if d_box is not None and any(need[L:]) else [None] * L
        return (None, None, None, None) + tuple(gl) + tuple(gd)


class _DetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, box, label, reg_target):
        loss, g_l, g_b = det_loss_grad(logits, box, label, reg_target)
        ctx.g = (g_l, g_b)
        return loss[0].clone(), loss[1].clone()

    @staticmethod
    def backward(ctx, d_cls, d_box):
        g_l, g_b = ctx.g
        return (g_l * d_cls if d_cls is not None and ctx.needs_input_grad[0] else None,
                g_b * d_box if d_box is not None and ctx.needs_input_grad[1] else None, None, None)


def _cat(xs, dtype=None) -> Tensor:
    t = torch.cat(list(xs), 0) if isinstance(xs, (list, tuple)) else xs
    return t if dtype is None else t.to(dtype)


@ops._on_tensor_device
def rpn_loss(objectness: Sequence[Tensor], pred_bbox_deltas: Sequence[Tensor], labels, regression_targets, sampled) -> Tuple[Tensor, Tensor]:
    """the reference's ``compute_loss`` on the head's own outputs: ``objectness`` / ``pred_bbox_deltas`` are the per-level lists the RPN head
    returns ([N, A, H, W] / [N, 4A, H, W]); ``labels`` (1 / 0 / -1), ``regression_targets`` and ``sampled`` (the sampler's positive | negative
    masks) are per-image lists, or concatenated tensors, over the anchors in the reference's order - what ``match_targets`` returns for the
    images' anchors.  Returns ``(loss_objectness, loss_rpn_box_reg)``; differentiable with respect to the head outputs."""
    objectness, pred_bbox_deltas = list(objectness), list(pred_bbox_deltas)
    if not objectness or len(objectness) != len(pred_bbox_deltas):
        raise ValueError("rpn_loss: one objectness and one delta tensor per level")
    for o, d in zip(objectness, pred_bbox_deltas):
        if o.dim() != 4 or d.dim() != 4 or d.shape[1] != 4 * o.shape[1] or d.shape[0] != o.shape[0] or d.shape[2:] != o.shape[2:]:
            raise ValueError("rpn_loss: a level is [N, A, H, W] and [N, 4A, H, W], got %s and %s" % (tuple(o.shape), tuple(d.shape)))
    label = _cat(labels, torch.int32)
    smp = _cat(sampled)
    smp = (smp != 0).to(torch.uint8) if smp.dtype != torch.uint8 else smp
    return _RpnLoss.apply(len(objectness), label, smp, _cat(regression_targets, torch.float32), *objectness, *pred_bbox_deltas)


@ops._on_tensor_device
def fastrcnn_loss(class_logits: Tensor, box_regression: Tensor, labels, regression_targets) -> Tuple[Tensor, Tensor]:
    """the reference's ``fastrcnn_loss`` (same signature): ``(classification_loss, box_loss)`` for class_logits [R, K], box_regression
    [R, 4K], per-image lists (or tensors) of labels and regression targets.  Rows with label -1 are left out of both terms (the head may run
    on unsampled RoIs); with none the value is the reference's.  Differentiable with respect to the two head outputs."""
    return _DetLoss.apply(class_logits, box_regression, _cat(labels, torch.int32), _cat(regression_targets, torch.float32))
