"""fc7's SuperSpike gradient at the fine-tuning shape of the default model: the chain of hidden.py against the stock formulation, one GPU, one
process, interleaved repeats.  Prints (and with --out writes) the lines of profiles/fc7_grad.txt.

  shape    R = 1024 RoIs, Hd = 1024, T = 12 (Tc = 11 current steps); lif6's planes word-major, lif7's as rows, about one bit in eight
  arm N    planes_to_rows x 2 -> spike_gemm_bf16x3 -> lif_surrogate_bwd -> spike_linear_wgrad (hidden.py), timed per launch and as a whole
  arm S    taps.planes_raster_rows -> .float() -> torch.matmul for the currents and for the weight gradient, the recurrence as a torch loop
           over T (the same teacher-forced adjoint, element-wise torch operators)
Times are device times (events around `--iters` back-to-back calls, after warm-up), the two arms alternating `--repeats` times.  Two ceilings
go next to them: 2 N K Tc R flop against 155 TF for the weight gradient (what the guide gives for v_mfma_f32_32x32x2_f32), and the scan's
bytes against the rate a device-to-device copy of the same size reaches in this run.  Exit status 1 unless the new chain is faster than the stock
one in EVERY repeat (the one gate of the measurement).
usage: python tools/time_fc7_grad.py [--repeats 20] [--iters 5] [--warmup 3] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, HD, T = 1024, 1024, 12
MFMA_F32_TF = 155.0


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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from snn_automotive_object_detection_amd import _lib, hidden, ops, taps
    from tools.time_readout_grad import kappa_last
    if not torch.cuda.is_available():
        raise SystemExit("time_fc7_grad.py needs the GPU: nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    Tc, W = T - 1, HD // 32
    p_lif = ops.LIFParameters(alpha=100, v_th=torch.as_tensor(0.1))
    p = ops.make_params(ops.LIFParameters(v_th=torch.as_tensor(0.25)), p_lif)
    alpha = float(p_lif.alpha)
    g = torch.Generator(device="cpu").manual_seed(7)

    def planes(steps):                                               # about one bit in eight: three ANDed words
        raw = [torch.randint(-2 ** 31, 2 ** 31, (steps * R * W,), dtype=torch.int64, generator=g).to(torch.int32) for _ in range(3)]
        return (raw[0] & raw[1] & raw[2]).to(dev).view(torch.uint8)
    ws6, ws7 = planes(Tc), planes(T)
    v6 = _lib.snn_planes_view(0, R * W, R, W, _lib.PLANE_LAYOUTS["word_major"], Tc, 0)
    v7 = _lib.snn_planes_view(0, R * W, R, W, _lib.PLANE_LAYOUTS["rows"], T, 0)
    w7 = (torch.randn((HD, HD), generator=g) * (3.0 / HD ** 0.5)).to(dev)
    w7p = ops.pack_linear_bf16x3(w7)
    gu = torch.randn((R, HD), generator=g).to(dev)
    a, b, th = float(p.dt_tau_mem), float(p.neg_dt_tau_syn), float(p.v_th_lif)
    kap = torch.tensor(kappa_last(a, b, T), dtype=torch.float32, device=dev)

    # arm N, launch by launch (each stage on the outputs of the one before)
    def n_rows6():
        return hidden.planes_to_rows(ws6, v6, Tc)

    def n_rows7():
        return hidden.planes_to_rows(ws7, v7, T)
    z6, z7 = n_rows6(), n_rows7()

    def n_gemm():
        return ops.spike_gemm_bf16x3(z6.view(Tc * R, W), HD, HD, w7p)
    cur = n_gemm().view(Tc, R, -1)

    def n_scan():
        return hidden.lif_surrogate_bwd(cur, z7, HD, p, alpha, gu=gu)
    d_cur = n_scan()

    def n_wgrad():
        return hidden.spike_linear_wgrad(z6, d_cur, HD, HD)

    def n_chain():
        a6, a7 = hidden.planes_to_rows(ws6, v6, Tc), hidden.planes_to_rows(ws7, v7, T)
        c = ops.spike_gemm_bf16x3(a6.view(Tc * R, W), HD, HD, w7p).view(Tc, R, -1)
        return hidden.spike_linear_wgrad(a6, hidden.lif_surrogate_bwd(c, a7, HD, p, alpha, gu=gu), HD, HD)

    # arm S
    def s_scan(c, zf):
        v = torch.zeros((R, HD), device=dev)
        i = torch.zeros_like(v)
        vds = []
        for t in range(T):
            vd = v + a * ((0.0 - v) + i) if t else v.clone()
            vds.append(vd)
            v = vd * (1.0 - zf[t])
            if t < Tc:
                i = (i + b * i) + c[t]
        Gv, Gi = torch.zeros_like(v), torch.zeros_like(v)
        out = [None] * Tc
        for t in range(Tc, -1, -1):
            if t < Tc:
                out[t] = Gi
            d = alpha * (vds[t] - th).abs() + 1.0
            dz = kap[t] * gu + Gv * (0.0 - vds[t])
            dvd = Gv * (1.0 - zf[t]) + dz / (d * d)
            Gi = dvd * a + Gi * (1.0 + b)
            Gv = dvd * (1.0 - a)
        return torch.stack(out)

    def s_raster():
        return taps.planes_raster_rows(ws6, v6, HD, Tc).float(), taps.planes_raster_rows(ws7, v7, HD, T).float()
    r6, r7 = s_raster()

    def s_gemm():
        return torch.matmul(r6.view(Tc * R, HD), w7.t()).view(Tc, R, HD)
    s_cur = s_gemm()
    s_d = s_scan(s_cur, r7)

    def s_wgrad():
        return torch.matmul(s_d.view(Tc * R, HD).t(), r6.view(Tc * R, HD))

    def s_chain():
        f6, f7 = s_raster()
        c = torch.matmul(f6.view(Tc * R, HD), w7.t()).view(Tc, R, HD)
        return torch.matmul(s_scan(c, f7).view(Tc * R, HD).t(), f6.view(Tc * R, HD))
    src = torch.empty(Tc * R * HD, device=dev)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)
    arms = [("N planes_to_rows lif6", n_rows6), ("N planes_to_rows lif7", n_rows7), ("N spike_gemm_bf16x3", n_gemm), ("N lif_surrogate_bwd", n_scan),
            ("N spike_linear_wgrad", n_wgrad), ("N whole chain", n_chain), ("S raster + float", s_raster), ("S matmul currents", s_gemm),
            ("S torch-loop adjoint", lambda: s_scan(s_cur, r7)), ("S matmul weight gradient", s_wgrad), ("S whole chain", s_chain),
            ("copy of d_cur's size", copy)]
    for _ in range(args.warmup):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    got, ref = n_chain(), s_chain()
    scale, diff = float(ref.abs().max()), float((got - ref).abs().max())
    times = {name: [] for name, _ in arms}
    for _ in range(args.repeats):
        for name, fn in arms:
            times[name].append(device_ms(fn, args.iters))
    ghz = bench.held_clock_ghz(n_wgrad, min(times["N spike_linear_wgrad"]), dev)
    lines = ["# python tools/time_fc7_grad.py --repeats %d --iters %d --warmup %d   (device times in ms, events around back-to-back calls; all arms alternate)"
             % (args.repeats, args.iters, args.warmup), "# device: %s" % torch.cuda.get_device_name(0),
             "# shape: R = %d, Hd = %d, T = %d (Tc = %d), planes at about one bit in eight; arm N = hidden.py's chain, arm S = the stock formulation" % (R, HD, T, Tc), ""]
    for name, _ in arms:
        ts = times[name]
        lines.append("  %-28s min %.4f  median %.4f  max %.4f" % (name, min(ts), sorted(ts)[len(ts) // 2], max(ts)))
    n, s = times["N whole chain"], times["S whole chain"]
    wins = sum(1 for x, y in zip(n, s) if x < y)
    lines += ["", "whole chain: stock / new = %.2fx (min over min); the new chain is faster in %d of %d repeats (slowest new %.4f, fastest stock %.4f)"
              % (min(s) / min(n), wins, len(n), max(n), min(s)),
              "weight gradient alone: torch.matmul on rasterised planes / snn_spike_linear_wgrad = %.2fx (min over min)"
              % (min(times["S matmul weight gradient"]) / min(times["N spike_linear_wgrad"]))]
    flop = 2.0 * HD * HD * Tc * R
    t_w = min(times["N spike_linear_wgrad"])
    lines.append("weight gradient ceiling: %.1f GFLOP in %.4f ms = %.1f TF = %.0f %% of the %.0f TF of v_mfma_f32_32x32x2_f32; held shader clock while it runs: %s GHz"
                 % (flop / 1e9, t_w, flop / t_w / 1e9, 100.0 * flop / t_w / 1e9 / MFMA_F32_TF, MFMA_F32_TF, "%.2f" % ghz if ghz else "not measured"))
    scan_bytes = 4.0 * Tc * R * HD * 4 + R * HD * 4 + T * R * W * 4
    t_s, t_c = min(times["N lif_surrogate_bwd"]), min(times["copy of d_cur's size"])
    copy_rate = 2.0 * Tc * R * HD * 4 / t_c / 1e9
    lines.append("scan ceiling: %.1f MB in %.4f ms = %.2f TB/s; a copy of %.1f MB (read + write) runs at %.2f TB/s here: the scan reaches %.0f %% of the copy rate"
                 % (scan_bytes / 1e6, t_s, scan_bytes / t_s / 1e9, 2.0 * Tc * R * HD * 4 / 1e6, copy_rate, 100.0 * scan_bytes / t_s / 1e9 / copy_rate))
    lines.append("largest |new - stock| of fc7's gradient = %.3g at a largest |value| of %.3g (fp32 sums in another order)" % (diff, scale))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if wins < len(n):                                                # the one gate of this measurement
        raise SystemExit("the new chain was faster in only %d of %d repeats" % (wins, len(n)))


if __name__ == "__main__":
    main()
