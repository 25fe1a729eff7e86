"""Readout weight gradients at the two headline shapes: snn_li_heads_wgrad against the stock formulation, one GPU, one process, interleaved
repeats.  Prints (and with --out writes) the lines of profiles/readout_grad.txt.

  shapes   RPN at Cityscapes b = 2: rows 196 416, 256 columns (SPLIT4 planes), NA + NB = 3 + 12, T = 8
           detector:               rows 2000, 1024 columns (ROWS planes), NA + NB = 9 + 36, T = 12
  arm N    ops.li_heads_wgrad on the planes (two launches)
  arm S    what the parent can do: taps.planes_raster_rows -> .float() -> kappa fold over t -> g.T @ S   (stock torch on the byte raster)
Times are device times (events around `--iters` back-to-back calls, after warm-up), the two arms alternating `--repeats` times; the plane read
of arm N is rows x words x T x 4 bytes over its time.  The shader clock the chip holds while arm N runs comes from bench.held_clock_ghz.  The
two arms' results are compared at the shapes that are timed.
usage: python tools/time_readout_grad.py [--repeats 5] [--iters 20] [--warmup 3] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("rpn_cityscapes_b2", 196416, 256, "split4", 3, 12, 8), ("detector", 2000, 1024, "rows", 9, 36, 12))


def kappa_last(a, cb, T, li_order=0):
    """li_kappa (csrc/snn_post.h) restated: the last membrane of a unit current at step s, in double, cast to fp32 by the caller"""
    out = []
    for s in range(T):
        v = i = 0.0
        for t in range(s, T):
            x = 1.0 if t == s else 0.0
            if li_order == 0:
                i_in = i + x
                v = v + a * (i_in - v)
                i = i_in + cb * i_in
            else:
                v = v + a * (i - v)
                i = i + cb * i + x
        out.append(v)
    return out


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
    import numpy as np
    import torch
    import bench
    from snn_automotive_object_detection_amd import _lib, ops, taps
    if not torch.cuda.is_available():
        raise SystemExit("time_readout_grad.py needs the GPU: nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    p = ops.make_params(ops.LIFParameters(v_th=torch.as_tensor(0.25)), ops.LIFParameters(v_th=torch.as_tensor(0.1)))
    lines = ["# python tools/time_readout_grad.py --repeats %d --iters %d --warmup %d   (device times, events around back-to-back calls; arms alternate)"
             % (args.repeats, args.iters, args.warmup), "# device: %s" % torch.cuda.get_device_name(0)]
    for name, rows, n_cols, layout, NA, NB, T in SHAPES:
        words = n_cols // 32
        g = torch.Generator(device="cpu").manual_seed(rows)
        # random planes at a hidden layer's density (about one bit in eight): three ANDed words
        raw = [torch.randint(-2 ** 31, 2 ** 31, (T * rows * words,), dtype=torch.int64, generator=g).to(torch.int32) for _ in range(3)]
        planes = (raw[0] & raw[1] & raw[2]).to(dev).view(torch.uint8)
        view = _lib.snn_planes_view(0, rows * words, rows, words, _lib.PLANE_LAYOUTS[layout], T, 0)
        grad = torch.randn((rows, NA + NB), generator=g).to(dev)
        g_a, g_b = grad[:, :NA].contiguous(), grad[:, NA:].contiguous()
        kap = torch.tensor(kappa_last(float(np.float32(p.dt_tau_mem)), float(np.float32(p.neg_dt_tau_syn)), T), dtype=torch.float32, device=dev)

        def new():
            return ops.li_heads_wgrad(planes, view, n_cols, T, p, g_a, g_b)

        def stock():
            raster = taps.planes_raster_rows(planes, view, n_cols, T)                   # bytes [T, rows, n_cols]
            S = (raster.float() * kap[:, None, None]).sum(0)
            return grad.t() @ S
        for _ in range(args.warmup):
            n_out, s_out = new(), stock()
        torch.cuda.synchronize()
        got, ref = torch.cat(n_out), s_out
        scale = float(ref.abs().max())
        diff = float((got - ref).abs().max())
        t_new, t_stock = [], []
        for _ in range(args.repeats):
            t_new.append(device_ms(new, args.iters))
            t_stock.append(device_ms(stock, max(2, args.iters // 4)))
        ghz = bench.held_clock_ghz(new, min(t_new), dev)
        plane_bytes = rows * words * T * 4
        best = min(t_new)
        lines += ["", "%s: rows %d, columns %d (%s), NA + NB = %d + %d, T = %d, planes %.1f MB, stock raster %.0f MB + fp32 %.0f MB"
                  % (name, rows, n_cols, layout, NA, NB, T, plane_bytes / 1e6, T * rows * n_cols / 1e6, 4 * T * rows * n_cols / 1e6),
                  "  snn_li_heads_wgrad   ms per call: %s   (min %.4f)" % (" ".join("%.4f" % t for t in t_new), best),
                  "  stock formulation    ms per call: %s   (min %.4f)" % (" ".join("%.4f" % t for t in t_stock), min(t_stock)),
                  "  stock / new = %.1fx (min over min); every repeat of the new entry %s every repeat of the stock one"
                  % (min(t_stock) / best, "faster than" if max(t_new) < min(t_stock) else "NOT faster than"),
                  "  plane read of the new entry: %.1f MB in %.4f ms = %.2f TB/s; held shader clock while it runs: %s GHz"
                  % (plane_bytes / 1e6, best, plane_bytes / best / 1e9, "%.2f" % ghz if ghz else "not measured"),
                  "  largest |new - stock| = %.3g at a largest |value| of %.3g (fp32 sums in another order)" % (diff, scale)]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
