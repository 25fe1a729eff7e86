"""fc6's SuperSpike gradient at the fine-tuning shape of the default model: what fc6_grad.py adds below fc7's chain against the stock formulation,
and snn_spike_wgrad_bf16x3 against the fp32 kernel at fc7's shape.  One GPU, one process, interleaved repeats.  Prints (and with --out writes)
the lines of profiles/fc6_grad.txt.

  (a) shape  R = 1024 RoIs, C = 256 (D = 12544), Hd = 1024, T = 12: Tc6 = 10 current steps, encoder rows at about one bit in eight
      arm N  gz6 = d_cur7 W7 (torch.matmul) -> spike_gemm_bf16x3 on the encoder rows (fc6 packed in the natural order) -> lif_surrogate_bwd with gz
             -> spike_wgrad_bf16x3, timed per launch and as a whole
      arm S  the same matmul -> raster (shift-and-mask / taps.planes_raster_rows) -> .float() -> torch.matmul for the currents and for the weight gradient, the recurrence
             as a torch loop over T (the same teacher-forced adjoint, element-wise torch operators)
      the attach-time re-encode (ops.encode_rows and ops.roi_align_encode for T - 2 steps) is timed beside them: training passes only
      full   the WHOLE hidden backward of Fc6Grad below the readout gradients - planes_to_rows x 2, fc7's currents, adjoint (gu) and fp32 weight
             gradient (hidden.py's chain), then arm N - against the stock formulation of all of it, both adjoints as torch loops
      Exit status 1 unless the new chain is faster than the stock one in EVERY repeat, for the added chain AND for the whole backward (the gate).
  (b) shape  K = N = 1024, T' = 11, R = 1024 (fc7's, which both kernels accept): snn_spike_wgrad_bf16x3 against snn_spike_linear_wgrad and against
             torch.matmul on rasterised planes; the TF reached counted as 3 x 2 N K M flop against 2.5 PF, and the held shader clock.  No gate.
Times are device times (events around `--iters` back-to-back calls, after warm-up), all arms alternating `--repeats` times.
usage: python tools/time_fc6_grad.py [--repeats 20] [--iters 3] [--warmup 2] [--out FILE] [--ratios FILE]
  --ratios FILE: lines appended verbatim (the error / tolerance ratios tests/test_gpu_fc6_grad.py logs)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, C_IN, HD, T = 1024, 256, 1024, 12
D = 49 * C_IN
BF16_PF = 2.5
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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ratios", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from snn_automotive_object_detection_amd import _lib, fc6_grad, hidden, ops, taps
    from tools.time_readout_grad import kappa_last
    if not torch.cuda.is_available():
        raise SystemExit("time_fc6_grad.py needs the GPU: nothing is measured on a CPU")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    T7, T6, W6, Wd = T - 1, T - 2, HD // 32, D // 32
    p_lif = ops.LIFParameters(alpha=100, v_th=torch.as_tensor(0.1))
    p = ops.make_params(ops.LIFParameters(v_th=torch.as_tensor(0.25)), p_lif)
    alpha = float(p_lif.alpha)
    g = torch.Generator(device="cpu").manual_seed(7)

    def planes(steps, words):                                        # about one bit in eight: three ANDed words
        raw = [torch.randint(-2 ** 31, 2 ** 31, (steps * R * words,), dtype=torch.int64, generator=g).to(torch.int32) for _ in range(3)]
        return (raw[0] & raw[1] & raw[2]).view(steps, R, words).to(dev)
    enc, z6 = planes(T6, Wd), planes(T7, W6)
    v_z6 = _lib.snn_planes_view(0, R * W6, R, W6, _lib.PLANE_LAYOUTS["rows"], T7, 0)
    w7 = (torch.randn((HD, HD), generator=g) * (3.0 / HD ** 0.5)).to(dev)
    w6 = (torch.randn((HD, D), generator=g) * (3.0 / D ** 0.5)).to(dev)
    w6p = ops.pack_linear_bf16x3(w6)
    d_cur7 = (torch.randn((T7, R, HD), generator=g) * 0.01).to(dev)
    a, b, th = float(p.dt_tau_mem), float(p.neg_dt_tau_syn), float(p.v_th_lif)

    # ---- (a) arm N, launch by launch (each stage on the outputs of the one before)
    def n_gz():
        return torch.matmul(d_cur7.view(T7 * R, HD), w7).view(T7, R, HD)
    gz6 = n_gz()

    def n_gemm():
        return ops.spike_gemm_bf16x3(enc.view(T6 * R, Wd), D, HD, w6p)
    cur6 = n_gemm().view(T6, R, -1)

    def n_scan():
        return hidden.lif_surrogate_bwd(cur6, z6, HD, p, alpha, gz=gz6)
    d_cur6 = n_scan()

    def n_wgrad():
        return fc6_grad.spike_wgrad_bf16x3(enc, d_cur6, D, HD)

    def n_chain():
        gz = torch.matmul(d_cur7.view(T7 * R, HD), w7).view(T7, R, HD)
        c = ops.spike_gemm_bf16x3(enc.view(T6 * R, Wd), D, HD, w6p).view(T6, R, -1)
        return fc6_grad.spike_wgrad_bf16x3(enc, hidden.lif_surrogate_bwd(c, z6, HD, p, alpha, gz=gz), D, HD)

    # ---- (a) arm S
    def s_scan(c, zf, gz, Tc=T6, gu=None):                            # the window Tc: zf [Tc + 1], upstream gz[t] or kap[t] gu
        v = torch.zeros((R, HD), device=dev)
        i = torch.zeros_like(v)
        vds = []
        for t in range(Tc + 1):
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
            dz = (gz[t] if gu is None else kap[t] * gu) + Gv * (0.0 - vds[t])
            dvd = Gv * (1.0 - zf[t]) + dz / (d * d)
            Gi = dvd * a + Gi * (1.0 + b)
            Gv = dvd * (1.0 - a)
        return torch.stack(out)
    z6_ws = z6.view(-1).view(torch.uint8)

    shifts = torch.arange(32, dtype=torch.int32, device=dev)

    def s_raster():                                                  # (the raster entry takes rows of up to 256 words: fc6's 392 are unpacked by stock torch operators)
        f_enc = ((enc.unsqueeze(-1) >> shifts) & 1).view(T6, R, D).float()
        return f_enc, taps.planes_raster_rows(z6_ws, v_z6, HD, T7).float()
    r_enc, r_z6 = s_raster()

    def s_gemm():
        return torch.matmul(r_enc.view(T6 * R, D), w6.t()).view(T6, R, HD)
    s_cur = s_gemm()
    s_d = s_scan(s_cur, r_z6, gz6)

    def s_wgrad():
        return torch.matmul(s_d.view(T6 * R, HD).t(), r_enc.view(T6 * R, D))

    def s_chain():
        gz = torch.matmul(d_cur7.view(T7 * R, HD), w7).view(T7, R, HD)
        f_enc, f_z6 = s_raster()
        c = torch.matmul(f_enc.view(T6 * R, D), w6.t()).view(T6, R, HD)
        return torch.matmul(s_scan(c, f_z6, gz).view(T6 * R, HD).t(), f_enc.view(T6 * R, D))

    # ---- the whole hidden backward: fc7's half in front of each arm
    z7 = planes(T, W6)
    z7_ws = z7.view(-1).view(torch.uint8)
    v_z7 = _lib.snn_planes_view(0, R * W6, R, W6, _lib.PLANE_LAYOUTS["rows"], T, 0)
    w7p = ops.pack_linear_bf16x3(w7)
    gu = torch.randn((R, HD), generator=g).to(dev)
    kap = torch.tensor(kappa_last(a, b, T), dtype=torch.float32, device=dev)

    def n_full():
        a6, a7 = hidden.planes_to_rows(z6_ws, v_z6, T7), hidden.planes_to_rows(z7_ws, v_z7, T)
        c7 = ops.spike_gemm_bf16x3(a6.view(T7 * R, W6), HD, HD, w7p).view(T7, R, -1)
        d7 = hidden.lif_surrogate_bwd(c7, a7, HD, p, alpha, gu=gu)
        gw7 = hidden.spike_linear_wgrad(a6, d7, HD, HD)
        gz = torch.matmul(d7.view(T7 * R, HD), w7).view(T7, R, HD)
        c6 = ops.spike_gemm_bf16x3(enc.view(T6 * R, Wd), D, HD, w6p).view(T6, R, -1)
        return gw7, fc6_grad.spike_wgrad_bf16x3(enc, hidden.lif_surrogate_bwd(c6, a6, HD, p, alpha, gz=gz), D, HD)

    def s_full():
        f_enc, f6 = s_raster()
        f7 = taps.planes_raster_rows(z7_ws, v_z7, HD, T).float()
        c7 = torch.matmul(f6.view(T7 * R, HD), w7.t()).view(T7, R, HD)
        d7 = s_scan(c7, f7, None, Tc=T7, gu=gu)
        gw7 = torch.matmul(d7.view(T7 * R, HD).t(), f6.view(T7 * R, HD))
        gz = torch.matmul(d7.view(T7 * R, HD), w7).view(T7, R, HD)
        c6 = torch.matmul(f_enc.view(T6 * R, D), w6.t()).view(T6, R, HD)
        return gw7, torch.matmul(s_scan(c6, f6, gz).view(T6 * R, HD).t(), f_enc.view(T6 * R, D))

    # ---- the attach-time re-encode (training passes only)
    x_rows = (torch.rand((R, D), generator=g) * 0.6).to(dev)
    feats = [(torch.rand((2, C_IN, h, w), generator=g) * 0.6).to(dev) for h, w in ((200, 304), (100, 152), (50, 76), (25, 38))]
    scales = [0.25, 0.125, 0.0625, 0.03125]
    xy = torch.rand((R, 2), generator=g) * torch.tensor([1000.0, 600.0])
    rois = torch.cat([xy, xy + torch.rand((R, 2), generator=g) * 200.0 + 8.0], dim=1).to(dev)
    roi_batch = (torch.arange(R) % 2).to(torch.int32).to(dev)
    roi_level = (torch.arange(R) % 4).to(torch.int32).to(dev)

    def e_rows():
        return ops.encode_rows(x_rows, T6, p)

    def e_roi():
        return ops.roi_align_encode(feats, scales, rois, roi_batch, roi_level, T6, p)

    # ---- (b) fc7's shape
    Tb = T - 1
    zb = planes(Tb, W6)
    db = (torch.randn((Tb, R, HD), generator=g) * 0.01).to(dev)
    vb = _lib.snn_planes_view(0, R * W6, R, W6, _lib.PLANE_LAYOUTS["rows"], Tb, 0)
    rb = taps.planes_raster_rows(zb.view(-1).view(torch.uint8), vb, HD, Tb).float()

    def b_x3():
        return fc6_grad.spike_wgrad_bf16x3(zb, db, HD, HD)

    def b_f32():
        return hidden.spike_linear_wgrad(zb, db, HD, HD)

    def b_torch():
        return torch.matmul(db.view(Tb * R, HD).t(), rb.view(Tb * R, HD))

    arms = [("N matmul gz6 = d_cur7 W7", n_gz), ("N spike_gemm_bf16x3 (fc6)", n_gemm), ("N lif_surrogate_bwd (gz)", n_scan), ("N spike_wgrad_bf16x3", n_wgrad),
            ("N whole chain", n_chain), ("S raster + float", s_raster), ("S matmul currents", s_gemm),
            ("S torch-loop adjoint", lambda: s_scan(s_cur, r_z6, gz6)), ("S matmul weight gradient", s_wgrad), ("S whole chain", s_chain),
            ("N whole hidden backward", n_full), ("S whole hidden backward", s_full),
            ("re-encode: encode_rows", e_rows), ("re-encode: roi_align_encode", e_roi),
            ("(b) spike_wgrad_bf16x3", b_x3), ("(b) spike_linear_wgrad", b_f32), ("(b) matmul on rasters", b_torch)]
    for _ in range(args.warmup):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    got, ref = n_chain(), s_chain()
    scale, diff = float(ref.abs().max()), float((got - ref).abs().max())
    gb, rb32 = b_x3(), b_f32()
    diff_b, scale_b = float((gb - rb32).abs().max()), float(rb32.abs().max())
    (g7n, g6n), (g7s, g6s) = n_full(), s_full()
    diff_f7, diff_f6 = float((g7n - g7s).abs().max()), float((g6n - g6s).abs().max())
    del got, ref, gb, rb32, g7n, g6n, g7s, g6s
    times = {name: [] for name, _ in arms}
    for _ in range(args.repeats):
        for name, fn in arms:
            times[name].append(device_ms(fn, args.iters))
    ghz_a = bench.held_clock_ghz(n_wgrad, min(times["N spike_wgrad_bf16x3"]), dev)
    ghz_b = bench.held_clock_ghz(b_x3, min(times["(b) spike_wgrad_bf16x3"]), dev)
    scratch_a = lib.snn_spike_wgrad_bf16x3_workspace_bytes(R, D, HD, T6)
    lines = ["# python tools/time_fc6_grad.py --repeats %d --iters %d --warmup %d   (device times in ms, events around back-to-back calls; all arms alternate)"
             % (args.repeats, args.iters, args.warmup), "# device: %s" % torch.cuda.get_device_name(0),
             "# (a) R = %d, C = %d (D = %d), Hd = %d, T = %d (Tc6 = %d), rows at about one bit in eight; arm N = fc6_grad.py's chain below d_cur7, arm S = the stock formulation"
             % (R, C_IN, D, HD, T, T6),
             "# (b) K = N = %d, T' = %d, rows = %d: the weight-gradient kernels alone" % (HD, Tb, R), ""]
    for name, _ in arms:
        ts = times[name]
        lines.append("  %-30s min %.4f  median %.4f  max %.4f" % (name, min(ts), sorted(ts)[len(ts) // 2], max(ts)))
    n, s = times["N whole chain"], times["S whole chain"]
    wins = sum(1 for x, y in zip(n, s) if x < y)
    nf, sf = times["N whole hidden backward"], times["S whole hidden backward"]
    wins_f = sum(1 for x, y in zip(nf, sf) if x < y)
    t_w = min(times["N spike_wgrad_bf16x3"])
    flop = 2.0 * HD * D * T6 * R
    lines += ["", "(a) what Fc6Grad adds below d_cur7: stock / new = %.2fx (min over min); the new chain is faster in %d of %d repeats (slowest new %.4f, fastest stock %.4f)"
              % (min(s) / min(n), wins, len(n), max(n), min(s)),
              "(a) the whole hidden backward (fc7's half + fc6's): stock / new = %.2fx (min over min); the new chain is faster in %d of %d repeats (slowest new %.4f, "
              "fastest stock %.4f); largest |new - stock| of fc7's / fc6's gradient = %.3g / %.3g" % (min(sf) / min(nf), wins_f, len(nf), max(nf), min(sf), diff_f7, diff_f6),
              "(a) weight gradient alone: torch.matmul on rasterised planes / snn_spike_wgrad_bf16x3 = %.2fx (min over min)"
              % (min(times["S matmul weight gradient"]) / t_w),
              "(a) weight gradient: %.1f GFLOP of sums, 3 x that on the matrix cores, in %.4f ms = %.0f TF of bf16 products = %.0f %% of %.1f PF; %.1f TF of sums "
              "(the fp32 pipe's ceiling is %.0f TF); held shader clock while it runs: %s GHz; scratch query %.1f MB"
              % (flop / 1e9, t_w, 3 * flop / t_w / 1e9, 100.0 * 3 * flop / t_w / 1e9 / (BF16_PF * 1e3), BF16_PF, flop / t_w / 1e9, MFMA_F32_TF,
                 "%.2f" % ghz_a if ghz_a else "not measured", scratch_a / 1e6),
              "(a) largest |new - stock| of fc6's gradient = %.3g at a largest |value| of %.3g (fp32 sums in another order)" % (diff, scale)]
    tb_x3, tb_f32, tb_t = (min(times[k]) for k in ("(b) spike_wgrad_bf16x3", "(b) spike_linear_wgrad", "(b) matmul on rasters"))
    flop_b = 2.0 * HD * HD * Tb * R
    lines += ["(b) snn_spike_linear_wgrad / snn_spike_wgrad_bf16x3 = %.2fx; torch.matmul on rasterised planes / snn_spike_wgrad_bf16x3 = %.2fx (min over min)"
              % (tb_f32 / tb_x3, tb_t / tb_x3),
              "(b) %.1f GFLOP of sums in %.4f ms: %.0f TF of bf16 products = %.1f %% of %.1f PF (the fp32 kernel: %.1f TF of %.0f); held shader clock: %s GHz; "
              "largest |bf16x3 - fp32 kernel| = %.3g at a largest |value| of %.3g"
              % (flop_b / 1e9, tb_x3, 3 * flop_b / tb_x3 / 1e9, 100.0 * 3 * flop_b / tb_x3 / 1e9 / (BF16_PF * 1e3), BF16_PF, flop_b / tb_f32 / 1e9, MFMA_F32_TF,
                 "%.2f" % ghz_b if ghz_b else "not measured", diff_b, scale_b)]
    if args.ratios and os.path.exists(args.ratios):
        with open(args.ratios) as f:
            lines += ["", "# tests/test_gpu_fc6_grad.py, largest observed error / tolerance ratios"] + [ln.rstrip("\n") for ln in f if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if wins < len(n) or wins_f < len(nf):                            # the one gate of this measurement
        raise SystemExit("the new chain was faster in only %d of %d repeats (the added chain) / %d of %d (the whole hidden backward)" % (wins, len(n), wins_f, len(nf)))


if __name__ == "__main__":
    main()
