"""Target matching and the two head losses at the headline shapes: each entry against the stock-torch formulation of the same step, one GPU, one
process, interleaved repeats.  Prints (and with --out writes) the lines of profiles/head_losses.txt.  Nothing is asserted.

  matching  Cityscapes b = 2: 294 624 anchors per image (pyramid 192x384 .. 12x24, A = 3), G = 32 and G = 128 ground-truth boxes per image, RPN
            thresholds, low-quality matches allowed
            arm N  losses.match_targets_raw: one snn_match_targets call for both images (three launches)
            arm S  per image: box_iou -> Matcher (max over dim 0, thresholds, max over dim 1, where) -> labels -> encode_boxes   (stock torch)
  rpn loss  the same pyramid: 589 248 anchors, 256 sampled per image
            arm N  losses.rpn_loss_grad (three launches; gradients with respect to the head's own row order)
            arm S  permute to the reference's order -> smooth_l1 + binary_cross_entropy_with_logits on the gathered rows -> autograd backward
  det loss  R = 1024 RoIs, K = 9 classes
            arm N  losses.det_loss_grad (three launches)
            arm S  cross_entropy + smooth_l1 on the gathered class boxes -> autograd backward
Times are device times (events around `--iters` back-to-back calls, after warm-up), the two arms alternating `--repeats` times.
usage: python tools/time_head_losses.py [--repeats 5] [--iters 20] [--warmup 3] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PYRAMID = ((192, 384), (96, 192), (48, 96), (24, 48), (12, 24))
IMAGE = (768, 1536)


def device_ms(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from snn_automotive_object_detection_amd import losses
    from snn_automotive_object_detection_amd.model import _default_anchorgen
    from snn_automotive_object_detection_amd.stock.anchors import ImageList
    if not torch.cuda.is_available():
        raise SystemExit("time_head_losses.py needs the GPU: nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    N, A = 2, 3
    lines = ["# python tools/time_head_losses.py --repeats %d --iters %d --warmup %d   (device times, events around back-to-back calls; arms alternate)"
             % (args.repeats, args.iters, args.warmup), "# device: %s" % torch.cuda.get_device_name(0)]

    def report(title, new, stock, note):
        for _ in range(args.warmup):
            new(), stock()
        t_new, t_stock = [], []
        for _ in range(args.repeats):
            t_new.append(device_ms(new, args.iters))
            t_stock.append(device_ms(stock, max(2, args.iters // 4)))
        lines.extend(["", title, "  new entry            ms per call: %s   (min %.4f)" % (" ".join("%.4f" % t for t in t_new), min(t_new)),
                      "  stock formulation    ms per call: %s   (min %.4f)" % (" ".join("%.4f" % t for t in t_stock), min(t_stock)),
                      "  stock / new = %.1fx (min over min); every repeat of the new entry %s every repeat of the stock one"
                      % (min(t_stock) / min(t_new), "faster than" if max(t_new) < min(t_stock) else "NOT faster than"), "  " + note])

    feats = [torch.empty((N, 1, h, w), device=dev) for h, w in PYRAMID]
    anchors = _default_anchorgen()(ImageList(torch.empty((N, 3) + IMAGE, device=dev), [IMAGE] * N), feats)
    per = int(anchors[0].shape[0])
    all_anchors = torch.cat(anchors)
    g = torch.Generator().manual_seed(1)
    for G in (32, 128):
        xy = torch.rand((N * G, 2), generator=g) * torch.tensor([IMAGE[1] - 320.0, IMAGE[0] - 320.0])
        gt = torch.cat((xy, xy + 20.0 + 280.0 * torch.rand((N * G, 2), generator=g)), dim=1).to(dev)
        gts = list(gt.split(G))

        def new():
            return losses.match_targets_raw(all_anchors, [per] * N, gt, None, [G] * N, 0.7, 0.3, True, (1.0, 1.0, 1.0, 1.0))

        def stock():
            return [losses._match_stock(anchors[n], gts[n], None, 0.7, 0.3, True, (1.0, 1.0, 1.0, 1.0)) for n in range(N)]
        idx = new()[0]
        ref = torch.cat([r[0] for r in stock()])
        report("matching: %d images x %d anchors, G = %d per image; the stock IoU matrix is %.0f MB per image" % (N, per, G, G * per * 4 / 1e6), new, stock,
               "decisions that differ between the two arms: %d of %d" % (int((idx.to(torch.int64) != ref).sum()), idx.numel()))

    # the RPN loss on the same pyramid
    shapes = [(N, h, w) for h, w in PYRAMID]
    P = sum(n * h * w for n, h, w in shapes)
    logits = torch.randn((P, A), generator=g).to(dev)
    deltas = (torch.randn((P, 4 * A), generator=g) * 0.2).to(dev)
    label = torch.zeros(N * per, dtype=torch.int32)
    sampled = torch.zeros(N * per, dtype=torch.uint8)
    for n in range(N):
        pick = torch.randperm(per, generator=g)[:256] + n * per
        sampled[pick] = 1
        label[pick[:128]] = 1
    label, sampled = label.to(dev), sampled.to(dev)
    targets = (torch.randn((N * per, 4), generator=g) * 0.2).to(dev)
    obj_levels, dl_levels = losses._level_views(logits, shapes, A), losses._level_views(deltas, shapes, 4 * A)
    pos = torch.where((sampled != 0) & (label == 1))[0]
    smp = torch.cat([pos, torch.where((sampled != 0) & (label == 0))[0]])
    lab_f = label.float()

    def new_rpn():
        return losses.rpn_loss_grad(shapes, A, logits, deltas, label, sampled, targets)

    def stock_rpn():
        o = [x.detach().requires_grad_() for x in obj_levels]
        d = [x.detach().requires_grad_() for x in dl_levels]
        of = torch.cat([x.permute(0, 2, 3, 1).reshape(N, -1, 1) for x in o], dim=1).reshape(-1)
        df = torch.cat([x.permute(0, 2, 3, 1).reshape(N, -1, 4) for x in d], dim=1).reshape(-1, 4)
        box = F.smooth_l1_loss(df[pos], targets[pos], beta=1 / 9, reduction="sum") / smp.numel()
        ob = F.binary_cross_entropy_with_logits(of[smp], lab_f[smp])
        (ob + box).backward()
        return ob, box, o, d
    mine, theirs = new_rpn()[0], stock_rpn()
    report("rpn loss: %d anchors, %d sampled" % (N * per, int(sampled.sum())), new_rpn, stock_rpn,
           "losses: new (%.6f, %.6f), stock (%.6f, %.6f)" % (float(mine[0]), float(mine[1]), float(theirs[0]), float(theirs[1])))

    # the detector loss
    R, K = 1024, 9
    cl = (torch.randn((R, K), generator=g) * 2.0).to(dev)
    bx = (torch.randn((R, 4 * K), generator=g) * 0.2).to(dev)
    lb = torch.randint(0, K, (R,), generator=g)
    lb[::4] = 0
    lb32, lb64 = lb.to(torch.int32).to(dev), lb.to(dev)
    tg = (torch.randn((R, 4), generator=g) * 0.2).to(dev)

    def new_det():
        return losses.det_loss_grad(cl, bx, lb32, tg)

    def stock_det():
        c, b = cl.detach().requires_grad_(), bx.detach().requires_grad_()
        ce = F.cross_entropy(c, lb64)
        p = torch.where(lb64 > 0)[0]
        box = F.smooth_l1_loss(b.reshape(R, K, 4)[p, lb64[p]], tg[p], beta=1 / 9, reduction="sum") / R
        (ce + box).backward()
        return ce, box
    mine, theirs = new_det()[0], stock_det()
    report("det loss: R = %d, K = %d" % (R, K), new_det, stock_det,
           "losses: new (%.6f, %.6f), stock (%.6f, %.6f)" % (float(mine[0]), float(mine[1]), float(theirs[0]), float(theirs[1])))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
