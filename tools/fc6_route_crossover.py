"""Where does the dense fc6 + LIF launch overtake the structured-sparse one?  (run on an MI355X)

  python tools/fc6_route_crossover.py [--windows 5] [--iters 20] > profiles/fc6_route_crossover.txt

Shapes: the bench's detector head - 2 x 1000 RoIs, C = 256 (D = 12544), Hd = 1024, K = 9, T_det = 12, precision bf16x3.  Base: the RoI features
bench.py pools from its backbone-fed pyramid (same seeds).  Ladder: a fraction f of the aligned runs of 16 RoIs is replaced by
bench.worst_case_tensor values - every occupied nibble of the bin-major planes e_3 .. full.  The head is the row-fed one (what bench.py's step
runs): a ladder over RoIs needs the RoI features themselves, which the RoIAlign-fed entry never materialises.  Per point: the device's hit
rate (route_stat of an `auto` call), and the detector head (encoder, fc6 + LIF, fc7 + LIF, LI heads) timed with HIP events under fc6_route =
sparse and dense, then under auto at the crossover those two columns give - each the median of the windows' means, with the spread (max - min) of the windows beside it.
SNN_FC6_ROUTE_DEFAULT_CROSSOVER is the hit rate of the lowest ladder point at which dense beats sparse by more than that spread, rounded down to
three digits so that this point itself takes the dense side (1.0 if none does); `auto - sparse` at f = 0 is the price of the route (it includes the encoder fold that `auto` gives up)."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.route_crossover import LADDER, time_windows  # noqa: E402


def ladder_point(base, worst, f, gen):
    """a seeded fraction f of the aligned 16-RoI runs takes the worst-case values"""
    import torch
    R = base.shape[0]
    runs = (R + 15) // 16
    pick = torch.zeros(runs, dtype=torch.bool)
    pick[torch.randperm(runs, generator=gen)[:int(round(f * runs))]] = True
    mask = pick.repeat_interleave(16)[:R].view(R, 1, 1, 1).to(base.device)
    return torch.where(mask, worst, base).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--crossover", type=float, default=None, help="the crossover `auto` decides with (default: what this run's sparse / dense columns say)")
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
    head, base = leg.det_head, leg.rois
    T = wl["T_det"]
    g = torch.Generator(device="cpu").manual_seed(1000)
    worst = bench.worst_case_tensor(tuple(base.shape), g, T - 1).to(dev)
    print("# tools/fc6_route_crossover.py: %d RoIs, C = %d, Hd = %d, T_det = %d, bf16x3; row-fed detector head (encoder + fc6 + LIF + fc7 + LIF + LI heads), HIP events,"
          % (base.shape[0], base.shape[1], head.representation_size, T))
    print("# median of %d windows of %d calls (ms), spread = max - min of the windows; f = share of aligned 16-RoI runs on worst-case values" % (args.windows, args.iters))
    print("# %5s %9s | %8s %7s | %8s %7s | %8s %7s | %5s" % ("f", "hit rate", "sparse", "spread", "dense", "spread", "auto", "spread", "route"))
    points = []
    for f in LADDER:
        x = ladder_point(base, worst, f, torch.Generator(device="cpu").manual_seed(77))
        res = {}
        for route in ("sparse", "dense"):
            head.fc6_route = route
            res[route] = time_windows(lambda: head(x), args.windows, args.iters)
        head.fc6_route = "auto"
        head(x)
        hits, blocks, _, _ = head.route_stat.tolist()
        points.append((f, x, hits / max(blocks, 1), res))
    # the crossover this run's `auto` decides with: --crossover, else what the sparse / dense columns say, else the header's
    cross = None
    for f, _, rate, res in points:
        if res["sparse"][0] - res["dense"][0] > max(res["sparse"][1], res["dense"][1]):
            cross = (f, rate)
            break
    # (rounded DOWN to three digits: `auto` takes the dense side where hits > crossover x blocks, and the crossover point itself belongs to it)
    decide = args.crossover if args.crossover is not None else (math.floor(cross[1] * 1000.0) / 1000.0 if cross else 1.0)
    head.fc6_crossover = decide
    rows = []
    for f, x, rate, res in points:
        res["auto"] = time_windows(lambda: head(x), args.windows, args.iters)
        taken = head.route_stat.tolist()[2]
        rows.append((f, rate, res, taken))
        print("  %5.2f %9.4f | %8.4f %7.4f | %8.4f %7.4f | %8.4f %7.4f | %5d" % (f, rate, *res["sparse"], *res["dense"], *res["auto"], taken), flush=True)
    head.fc6_route = head.fc6_crossover = None
    price = rows[0][2]["auto"][0] - rows[0][2]["sparse"][0]
    print("# price of `auto` on backbone RoI features (auto - sparse at f = 0): %+.4f ms (sparse %.4f ms, spread %.4f / %.4f)" % (
        price, rows[0][2]["sparse"][0], rows[0][2]["sparse"][1], rows[0][2]["auto"][1]))
    if cross:
        print("# lowest ladder point at which dense beats sparse by more than the spread: f = %.2f, hit rate %.4f" % cross)
    else:
        print("# dense never beats sparse by more than the spread on this ladder: SNN_FC6_ROUTE_DEFAULT_CROSSOVER stays 1.0 (auto never leaves sparse)")
    print("# header: SNN_FC6_ROUTE_DEFAULT_CROSSOVER %g (this run decided with %g)" % (_lib.FC6_ROUTE_DEFAULT_CROSSOVER, decide))
    worst_excess = None
    for f, rate, res, _ in rows:
        spread = max(res["sparse"][1], res["dense"][1], res["auto"][1])
        excess = res["auto"][0] - (min(res["sparse"][0], res["dense"][0]) + max(price, 0.0) + spread)
        flag = "ok" if excess <= 0 else "OVER by %.4f ms" % excess
        print("# f = %.2f: auto %.4f <= min(sparse, dense) %.4f + price %.4f + spread %.4f ? %s" % (
            f, res["auto"][0], min(res["sparse"][0], res["dense"][0]), max(price, 0.0), spread, flag))
        worst_excess = excess if worst_excess is None else max(worst_excess, excess)
    print("# requirement (auto <= min(sparse, dense) + price + spread on every point): %s" % ("met" if worst_excess <= 0 else "NOT met"))


if __name__ == "__main__":
    main()
