"""Three-way timing of FPN features -> detections on the host, on the Cityscapes b = 2 pyramid of bench.py's default leg (needs the GPU).

  python tools/time_static.py [--iters 30] [--rounds 4] [--inputs backbone|randn] [--out FILE]

  (a) list        the list path: model.rpn + model.roi_heads forward on the features (counts come to the host twice inside)
  (b) eager       static.heads_padded + static.unpad (one host synchronisation, in unpad)
  (c) replay      static.CapturedHeads (max_det = detections_per_img + cap) + ONE copy of payload / payload_counts to pinned memory;
                  slots = 1 and slots = 2, each call waited for ("serial"), and slots = 2 with the wait for call k's copy issued after call
                  k + 1 was enqueued ("pipelined": what the second slot is for)

One process, one model, the same features for every path.  Every path is warmed up, then the paths alternate for --rounds rounds of --iters
calls each; a call is timed by device events around it (the time the stream was busy or waiting for the host) and by the host clock from the
call to the moment its results are on the host.  Medians with the 10th / 90th percentiles are printed, with the row counts every path found
and the check that (c)'s rows equal dp.pack_detections(unpad(b)) bit for bit.  Nothing here is a pass / fail criterion."""
import argparse
import os
import statistics
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--inputs", choices=["backbone", "randn"], default="backbone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import dp, static
    from snn_automotive_object_detection_amd.stock.anchors import ImageList
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_static.py needs an MI355X: a timing without one says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    wl = bench.WORKLOADS["cityscapes"]
    torch.manual_seed(4321)                                        # bench.py's model_for / make_leg: the same weights, the same features
    model = S.create_model(wl["dataset"], wl["K"], True, True, 0, False, False, wl["T_rpn"], wl["T_det"]).to(dev).eval()
    leg = bench.Leg(wl, "bf16x3", dev, 1000, args.inputs, model if args.inputs == "backbone" else None)
    feats = OrderedDict(zip(["0", "1", "2", "3", "pool"], leg.feats))
    del leg
    N = wl["batch"]
    images = ImageList(torch.empty((N, 0, 768, 1536)), [(768, 1536)] * N)
    cap, D = model.rpn.post_nms_top_n(), model.roi_heads.detections_per_img + model.rpn.post_nms_top_n()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("# python tools/time_static.py --iters %d --rounds %d --inputs %s" % (args.iters, args.rounds, args.inputs))
    say("# %s, %s; cityscapes pyramid b = %d, T = %d / %d, K = %d, cap = %d, detections_per_img = %d, max_det = %d, precision bf16x3, routes sparse"
        % (torch.cuda.get_device_name(dev), torch.__version__, N, wl["T_rpn"], wl["T_det"], wl["K"], cap, model.roi_heads.detections_per_img, D))

    # ---- the three paths: each call ends with its results on the host -------------------------------------------------------------------
    def list_path():
        props, _ = model.rpn(images, feats)
        dets, _ = model.roi_heads(feats, props, images.image_sizes)
        return dets

    def eager_path():
        return static.unpad(static.heads_padded(model, feats, images))

    runners = {1: static.CapturedHeads(model, feats, images, max_det=D, slots=1), 2: static.CapturedHeads(model, feats, images, max_det=D, slots=2)}
    pinned = {s: [(torch.empty((N, D, 6), dtype=torch.float32).pin_memory(), torch.empty((N,), dtype=torch.int32).pin_memory()) for _ in range(s)]
              for s in runners}
    turn = {1: 0, 2: 0}

    def replay_enqueue(slots):
        out = runners[slots](feats)
        p, c = pinned[slots][turn[slots]]
        turn[slots] = (turn[slots] + 1) % slots
        p.copy_(out["payload"], non_blocking=True)
        c.copy_(out["payload_counts"], non_blocking=True)
        return p, c

    def replay_path(slots):
        rows = replay_enqueue(slots)
        torch.cuda.current_stream().synchronize()
        return rows

    # ---- the same answer first (measuring-on-mi355x 6) ------------------------------------------------------------------------------------
    with torch.no_grad():
        lst, eag = list_path(), eager_path()
        ref = dp.pack_detections(eag, D, dev)
        for s in runners:
            p, c = replay_path(s)
            same = torch.equal(p.view(torch.int32), ref[0].cpu().view(torch.int32)) and torch.equal(c, ref[1].cpu())
            say("# replay slots=%d rows == dp.pack_detections(unpad(eager)) bit for bit: %s" % (s, same))
            if not same:
                raise SystemExit("the replay's rows differ from the eager path's: no timing of a wrong answer")
        say("# rows per image (fg + bg): list %s, eager %s, replay %s; RoIs per image: eager %s"
            % ([int(d["boxes"].shape[0]) for d in lst], [int(d["boxes"].shape[0]) for d in eag], c.tolist(), [int(d["all_scores"].shape[0]) for d in eag]))

    paths = OrderedDict([("a list (rpn + roi_heads forward)", list_path), ("b eager heads_padded + unpad", eager_path),
                         ("c replay slots=1 + pinned D2H, serial", lambda: replay_path(1)), ("c replay slots=2 + pinned D2H, serial", lambda: replay_path(2))])
    dev_ms = {k: [] for k in paths}
    host_ms = {k: [] for k in paths}
    piped = []
    with torch.no_grad():
        for name, fn in paths.items():                               # warm-up of every path at the timed shapes
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            print("warmed up: %s" % name, file=sys.stderr, flush=True)
        for rnd in range(args.rounds):
            for name, fn in paths.items():
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
                for a, b in ev:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    host_ms[name].append((time.perf_counter() - t0) * 1e3)
                dev_ms[name] += [a.elapsed_time(b) for a, b in ev]
                print("round %d timed: %s" % (rnd, name), file=sys.stderr, flush=True)
            # slots = 2, pipelined: call k + 1 is enqueued before the host waits for the copy of call k
            torch.cuda.synchronize()
            done = None
            t0 = time.perf_counter()
            for _ in range(args.iters):
                replay_enqueue(2)
                e = torch.cuda.Event()
                e.record()
                if done is not None:
                    done.synchronize()
                done = e
            done.synchronize()
            piped.append((time.perf_counter() - t0) * 1e3 / args.iters)
            print("round %d timed: pipelined" % rnd, file=sys.stderr, flush=True)
    say()
    say("%-46s %28s %28s" % ("path (per call, ms)", "device events  med [p10, p90]", "host clock  med [p10, p90]"))
    for name in paths:
        d, h = dev_ms[name], host_ms[name]
        say("%-46s %10.3f [%7.3f, %7.3f] %12.3f [%7.3f, %7.3f]   n = %d" % (name, statistics.median(d), pct(d, 0.1), pct(d, 0.9), statistics.median(h),
                                                                               pct(h, 0.1), pct(h, 0.9), len(d)))
    say("%-46s %28s %12.3f [%7.3f, %7.3f]   n = %d rounds of %d calls" % ("c replay slots=2 + pinned D2H, pipelined", "-", statistics.median(piped), min(piped),
                                                                               max(piped), len(piped), args.iters))
    base = statistics.median(host_ms["a list (rpn + roi_heads forward)"])
    say()
    say("host-clock medians, (a) over the path (> 1: faster than the list path):")
    for n in list(paths)[1:]:
        say("  %-44s %.3f x" % (n, base / statistics.median(host_ms[n])))
    say("  %-44s %.3f x" % ("c replay slots=2 + pinned D2H, pipelined", base / statistics.median(piped)))
    for r in runners.values():
        r.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
