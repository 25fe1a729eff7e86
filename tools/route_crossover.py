"""Where does the dense conv + LIF launch overtake the structured-sparse one?  (run on an MI355X)

  python tools/route_crossover.py [--windows 5] [--iters 20] > profiles/route_crossover.txt

Shapes: the Cityscapes pyramid, b = 2, C = 256, T = 8, precision bf16x3.  Base: the backbone-fed pyramid, built the way bench.py builds it (same
seeds).  Ladder: a fraction f of the aligned runs of 16 positions of every level (positions in (n, y, x) order) is replaced by
bench.worst_case_tensor values - every occupied nibble of the planes e_3 .. full.  Per point: the device's hit rate (route_stat of an `auto`
call), and the RPN head (encoder, conv + LIF, LI heads) timed with HIP events under conv_route = sparse, dense and auto - each the median of
the windows' means, with the spread (max - min) of the windows beside it.  SNN_ROUTE_DEFAULT_CROSSOVER is the hit rate of the lowest ladder
point at which dense beats sparse by more than that spread; `auto - sparse` at f = 0 is the price of the route."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LADDER = (0.0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.75, 1.0)


def ladder_point(base, worst, f, gen):
    """per level: a seeded fraction f of the aligned 16-position runs takes the worst-case values"""
    import torch
    out = []
    for b, w in zip(base, worst):
        N, C, H, W = b.shape
        P = N * H * W
        runs = (P + 15) // 16
        k = int(round(f * runs))
        pick = torch.zeros(runs, dtype=torch.bool)
        pick[torch.randperm(runs, generator=gen)[:k]] = True
        mask = pick.repeat_interleave(16)[:P].view(N, 1, H, W).to(b.device)
        out.append(torch.where(mask, w, b).contiguous())
    return out


def time_windows(fn, windows, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        means.append(a.elapsed_time(b) / iters)
    return statistics.median(means), max(means) - min(means)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if args.windows < 3:
        ap.error("--windows must be >= 3")
    import torch
    import bench
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import _lib
    dev = torch.device("cuda", 0)
    wl = dict(bench.WORKLOADS["cityscapes"])
    torch.manual_seed(4321)
    model = S.create_model(wl["dataset"], wl["K"], True, True, 0, False, False, 8, 12).eval()
    leg = bench.Leg(wl, "bf16x3", dev, 1000, "backbone", model)
    head, base = leg.rpn_head, leg.feats
    T = wl["T_rpn"]
    g = torch.Generator(device="cpu").manual_seed(1000)
    worst = [bench.worst_case_tensor(tuple(b.shape), g, T).to(dev) for b in base]
    print("# tools/route_crossover.py: Cityscapes pyramid, b = 2, C = 256, T = 8, bf16x3; RPN head (encoder + conv + LIF + LI heads), HIP events,")
    print("# median of %d windows of %d calls (ms), spread = max - min of the windows; f = share of aligned 16-position runs on worst-case values" % (args.windows, args.iters))
    print("# %5s %9s | %8s %7s | %8s %7s | %8s %7s | %5s" % ("f", "hit rate", "sparse", "spread", "dense", "spread", "auto", "spread", "route"))
    rows = []
    for f in LADDER:
        feats = ladder_point(base, worst, f, torch.Generator(device="cpu").manual_seed(77))
        res = {}
        for route in ("sparse", "dense", "auto"):
            head.conv_route = route
            res[route] = time_windows(lambda: head(feats), args.windows, args.iters)
        hits, blocks, taken, _ = head.route_stat.tolist()
        rate = hits / max(blocks, 1)
        rows.append((f, rate, res, taken))
        print("  %5.2f %9.4f | %8.4f %7.4f | %8.4f %7.4f | %8.4f %7.4f | %5d" % (f, rate, *res["sparse"], *res["dense"], *res["auto"], taken), flush=True)
    head.conv_route = None
    price = rows[0][2]["auto"][0] - rows[0][2]["sparse"][0]
    print("# price of `auto` on backbone inputs (auto - sparse at f = 0): %+.4f ms (sparse %.4f ms, spread %.4f / %.4f)" % (
        price, rows[0][2]["sparse"][0], rows[0][2]["sparse"][1], rows[0][2]["auto"][1]))
    cross = None
    for f, rate, res, _ in rows:
        spread = max(res["sparse"][1], res["dense"][1])
        if res["sparse"][0] - res["dense"][0] > spread:
            cross = (f, rate)
            break
    if cross:
        print("# lowest ladder point at which dense beats sparse by more than the spread: f = %.2f, hit rate %.4f" % cross)
    else:
        print("# dense never beats sparse by more than the spread on this ladder")
    print("# header: SNN_ROUTE_DEFAULT_CROSSOVER %g (this run decided with %g)" % (_lib.ROUTE_DEFAULT_CROSSOVER, _lib.ROUTE_DEFAULT_CROSSOVER))
    worst_excess = None
    for f, rate, res, _ in rows:
        spread = max(res["sparse"][1], res["dense"][1], res["auto"][1])
        excess = res["auto"][0] - (min(res["sparse"][0], res["dense"][0]) + max(price, 0.0) + spread)
        flag = "ok" if excess <= 0 else "OVER by %.4f ms" % excess
        print("# f = %.2f: auto %.4f <= min(sparse, dense) %.4f + price %.4f + spread %.4f ? %s" % (
            f, res["auto"][0], min(res["sparse"][0], res["dense"][0]), max(price, 0.0), spread, flag))
        worst_excess = excess if worst_excess is None else max(worst_excess, excess)
    print("# requirement (auto <= min(sparse, dense) + price + spread on every point): %s" % ("met" if worst_excess <= 0 else "NOT met"))
    for f, rate, res, _ in rows:
        gain = res["sparse"][0] - min(res["sparse"][0], res["dense"][0])
        if 0 < f < 1 and price > gain and res["dense"][0] < res["sparse"][0]:
            print("# finding: at f = %.2f the price of auto (%.4f ms) exceeds what the dense side gains (%.4f ms)" % (f, price, gain))


if __name__ == "__main__":
    main()
