#!/usr/bin/env python3
"""Fixtures of the head losses (tests/golden/loss_rpn_*.npz, loss_det_*.npz) from the reference's own bodies.

Runs where the reference lies beside the repository (oracle/make_golden.py's REF), never on the GPU box; it imports that module's shims and
loaders unchanged and reads the reference at run time only.  What runs:
  * RegionProposalNetwork.assign_targets_to_anchors and RoIHeadsSNN.assign_targets_to_proposals - the reference's bodies on a stub ``self`` whose
    ``proposal_matcher`` is the restated Matcher of tests/_head_losses.py and whose ``box_similarity`` is the restated box_iou;
  * RegionProposalNetwork.compute_loss on a stub ``self`` whose sampler returns the stored masks, on the outputs of the reference's
    concat_box_prediction_layers, and roi_heads.fastrcnn_loss: each in fp32 and once more on double inputs, with autograd for the gradients
    with respect to the head outputs.
BoxCoder.encode is torchvision's, not the reference's: tests/_head_losses.encode restates it (fp32 and fp64).
The fixtures are tensors only (inputs and expected outputs), loadable with allow_pickle=False.

Usage:  python tools/make_loss_golden.py [--out tests/golden]"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG                 # noqa: E402
from oracle import torchvision_restated as TV        # noqa: E402
from tests import _head_losses as HL                 # noqa: E402

RPN_CASES = {
    # name: (pyramid, N, A, ground-truth boxes per image, seed)
    "pyr_a3": (HL.PYRAMID, 2, 3, (2, 5), 1),
    "one_level": (((4, 5),), 3, 3, (1, 0, 3), 2),
}
DET_CASES = {
    # name: (RoIs per image, ground-truth boxes per image, K, seed)
    "k9": ((40, 25), (3, 2), 9, 3),
    "k11_bg": ((33, 30, 2), (4, 0, 1), 11, 4),
}
RPN_THRESH, DET_THRESH = (0.7, 0.3), (0.5, 0.5)
RPN_WEIGHTS, DET_WEIGHTS = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)


def np_(t):
    return t.detach().cpu().numpy()


def _anchors(shapes, A, g):
    """A anchors per position of every level, around the cell centres of a 64-pixel image (any boxes would do: the anchors are stored)"""
    out = []
    for H, W in shapes:
        cy, cx = torch.meshgrid((torch.arange(H) + 0.5) * (64.0 / H), (torch.arange(W) + 0.5) * (64.0 / W), indexing="ij")
        c = torch.stack((cx, cy), dim=-1).reshape(-1, 1, 2)
        half = (4.0 + 12.0 * torch.rand((1, A, 2), generator=g)) * (32.0 / max(H, W)) ** 0.5
        out.append(torch.cat((c - half, c + half), dim=-1).reshape(-1, 4))
    return torch.cat(out, 0)


def _sample(labels, batch, frac, g):
    pos_m, neg_m = [], []
    for lab in labels:
        pos, neg = torch.where(lab >= 1)[0], torch.where(lab == 0)[0]
        n_pos = min(pos.numel(), int(batch * frac))
        n_neg = min(neg.numel(), batch - n_pos)
        p, n = torch.zeros_like(lab, dtype=torch.uint8), torch.zeros_like(lab, dtype=torch.uint8)
        p[pos[torch.randperm(pos.numel(), generator=g)[:n_pos]]] = 1
        n[neg[torch.randperm(neg.numel(), generator=g)[:n_neg]]] = 1
        pos_m.append(p)
        neg_m.append(n)
    return pos_m, neg_m


def gen_rpn(ref_rpn, name, spec, out):
    shapes, N, A, n_gt, seed = spec
    g = torch.Generator().manual_seed(seed)
    anchors = _anchors(shapes, A, g)
    gts = []
    for G in n_gt:
        pick = anchors[torch.randint(0, anchors.shape[0], (G,), generator=g)]
        gts.append(pick + (torch.rand((G, 4), generator=g) - 0.5) * 3.0)
    stub = types.SimpleNamespace(box_similarity=TV.box_iou, proposal_matcher=HL.Matcher(RPN_THRESH[0], RPN_THRESH[1], True))
    labels, matched_gt = ref_rpn.RegionProposalNetwork.assign_targets_to_anchors(stub, [anchors] * N, [{"boxes": b} for b in gts])
    t32 = [HL.encode(m, anchors, RPN_WEIGHTS) for m in matched_gt]
    t64 = [HL.encode(m.double(), anchors.double(), RPN_WEIGHTS) for m in matched_gt]
    pos, neg = _sample(labels, 48, 0.5, g)
    stub.fg_bg_sampler = lambda _labels: (pos, neg)
    obj = [torch.randn((N, A, H, W), generator=g) * 2.0 for H, W in shapes]
    dl = [torch.randn((N, 4 * A, H, W), generator=g) * 0.2 for H, W in shapes]
    res = {}
    for tag, dt, tg in (("32", torch.float32, t32), ("64", torch.float64, t64)):
        o = [x.to(dt).requires_grad_() for x in obj]
        d = [x.to(dt).requires_grad_() for x in dl]
        of, df = ref_rpn.concat_box_prediction_layers(o, d)
        l_obj, l_box = ref_rpn.RegionProposalNetwork.compute_loss(stub, of, df, [x.to(dt) for x in labels], [x.to(dt) for x in tg])
        go = torch.autograd.grad(l_obj, o, retain_graph=True)
        gd = torch.autograd.grad(l_box, d)
        res["loss" + tag] = np_(torch.stack((l_obj, l_box)))
        res["g_logits" + tag] = np_(torch.cat([x.permute(0, 2, 3, 1).reshape(-1, A) for x in go], 0))
        res["g_deltas" + tag] = np_(torch.cat([x.permute(0, 2, 3, 1).reshape(-1, 4 * A) for x in gd], 0))
    idx = [HL.match(anchors, b, None, RPN_THRESH[0], RPN_THRESH[1], True)[0] for b in gts]
    np.savez_compressed(
        os.path.join(out, "loss_rpn_%s.npz" % name), shapes=np.array(shapes, dtype=np.int64), N=np.int64(N), A=np.int64(A), anchors=np_(anchors),
        gt_boxes=np_(torch.cat(gts, 0)), gt_counts=np.array(n_gt, dtype=np.int64), thresholds=np.array(RPN_THRESH), weights=np.array(RPN_WEIGHTS),
        logits=np_(torch.cat([x.permute(0, 2, 3, 1).reshape(-1, A) for x in obj], 0)),
        deltas=np_(torch.cat([x.permute(0, 2, 3, 1).reshape(-1, 4 * A) for x in dl], 0)),
        labels=np_(torch.cat(labels, 0)), matched_idx=np_(torch.cat(idx, 0)), sampled=np_(torch.cat([p | n for p, n in zip(pos, neg)], 0)),
        targets32=np_(torch.cat(t32, 0)), targets64=np_(torch.cat(t64, 0)), **res)
    print("loss_rpn_%s: %d anchors, %d sampled, losses %s" % (name, N * anchors.shape[0], int(sum(int((p | n).sum()) for p, n in zip(pos, neg))), res["loss32"]))


def gen_det(ref_roi, name, spec, out):
    rois, n_gt, K, seed = spec
    g = torch.Generator().manual_seed(seed)
    props, gts, gls = [], [], []
    for R, G in zip(rois, n_gt):
        b, gt, _ = HL.random_image(R, G, int(torch.randint(0, 1 << 30, (1,), generator=g)))
        props.append(torch.cat((b, gt)))                              # add_gt_proposals
        gts.append(gt)
        gls.append(torch.randint(1, K, (G,), generator=g, dtype=torch.int64))
    stub = types.SimpleNamespace(proposal_matcher=HL.Matcher(DET_THRESH[0], DET_THRESH[1], False))
    matched, labels = ref_roi.RoIHeadsSNN.assign_targets_to_proposals(stub, props, gts, gls)
    ref_boxes = [gt[m] if gt.shape[0] else torch.zeros((m.shape[0], 4)) for gt, m in zip(gts, matched)]
    t32 = torch.cat([HL.encode(r, p, DET_WEIGHTS) for r, p in zip(ref_boxes, props)], 0)
    t64 = torch.cat([HL.encode(r.double(), p.double(), DET_WEIGHTS) for r, p in zip(ref_boxes, props)], 0)
    keep = torch.cat(labels, 0) >= 0                                  # (the sampler never picks -1: the loss sees sampled rows only)
    Rt = int(keep.sum())
    logits = torch.randn((Rt, K), generator=g) * 2.0
    box = torch.randn((Rt, 4 * K), generator=g) * 0.2
    lab = torch.cat(labels, 0)[keep]
    res = {}
    for tag, dt, tg in (("32", torch.float32, t32[keep]), ("64", torch.float64, t64[keep])):
        lo, bo = logits.to(dt).requires_grad_(), box.to(dt).requires_grad_()
        l_cls, l_box = ref_roi.fastrcnn_loss(lo, bo, [lab], [tg])
        res["loss" + tag] = np_(torch.stack((l_cls, l_box)))
        res["g_logits" + tag] = np_(torch.autograd.grad(l_cls, lo, retain_graph=True)[0])
        res["g_box" + tag] = np_(torch.autograd.grad(l_box, bo)[0])
    idx = [HL.match(p, gt, gl, DET_THRESH[0], DET_THRESH[1], False)[0] for p, gt, gl in zip(props, gts, gls)]
    np.savez_compressed(
        os.path.join(out, "loss_det_%s.npz" % name), K=np.int64(K), proposals=np_(torch.cat(props, 0)), box_counts=np.array([p.shape[0] for p in props], dtype=np.int64),
        gt_boxes=np_(torch.cat(gts, 0)), gt_labels=np_(torch.cat(gls, 0)), gt_counts=np.array(n_gt, dtype=np.int64), thresholds=np.array(DET_THRESH),
        weights=np.array(DET_WEIGHTS), matched_idx=np_(torch.cat(idx, 0)), labels_all=np_(torch.cat(labels, 0)), targets32_all=np_(t32), targets64_all=np_(t64),
        keep=np_(keep), logits=np_(logits), box=np_(box), labels=np_(lab), targets32=np_(t32[keep]), targets64=np_(t64[keep]), **res)
    print("loss_det_%s: %d rows (%d foreground), losses %s" % (name, Rt, int((lab > 0).sum()), res["loss32"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    ref_rpn, _ = MG.load_reference()
    ref_roi = MG.load_reference_roi_heads()
    for name, spec in RPN_CASES.items():
        gen_rpn(ref_rpn, name, spec, args.out)
    for name, spec in DET_CASES.items():
        gen_det(ref_roi, name, spec, args.out)


if __name__ == "__main__":
    main()
