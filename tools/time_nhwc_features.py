"""Channels-last (NHWC) feature maps into both heads: the NHWC path against convert-then-NCHW, one GPU, one process, interleaved repeats:
writes profiles/nhwc_features_ab.txt.

bench.Leg with bench's own stepping (bench.timed_steps) on the cityscapes and bdd workloads, the detector fed by RoIAlign on the FPN maps,
features fp32 and again fp16.
  arm A  channels-last maps, the parent commit's behaviour: .contiguous() on every level inside the step (once per head, as ops did), then the
         NCHW heads
  arm B  the same maps on the NHWC path
  arm C  contiguous maps on the NCHW heads (the default path), for the repeat-to-repeat spread; run the tool once more with
         SNN_HIP_LIB=<the parent's libsnnhip.so> and --only-c for the same arm on the parent's kernels
The gate is "every repeat of B below every repeat of A" on each of the four legs.  The saving is held against the bytes the transposing copies
of arm A move (read + write of all five levels for the RPN head, of four for the detector).

--trace: afterwards one `rocprofv3 --kernel-trace --stats` run per leg, each its own child process under its own timeout that steps arm A and
then arm B, the next only if the previous ended well: per-launch times of the encoder launches of both arms and of arm A's copy kernels.
usage: python tools/time_nhwc_features.py [--repeats 3] [--steps 20] [--warmup 5] [--inputs backbone|randn] [--trace] [--only-c] [--out ...]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = ("cityscapes", "bdd")
DTYPES = ("fp32", "fp16")


def make_leg(name, inputs, dev):
    import torch
    import bench
    import snn_automotive_object_detection_amd as S

    class LayoutLeg(bench.Leg):
        """the leg's FPN maps contiguous (nchw[dtype]) and dense in channels_last (nhwc[dtype]); `arm` and `dtype` select what a step feeds the heads"""
        arm, dtype = "C", "fp32"

        def step(self):
            if self.arm == "A":                                   # (ops converted the levels once per head)
                f, fl = [x.contiguous() for x in self.nhwc[self.dtype]], [x.contiguous() for x in self.nhwc[self.dtype][:4]]
            elif self.arm == "B":
                f, fl = self.nhwc[self.dtype], self.nhwc[self.dtype][:4]
            else:
                f, fl = self.nchw[self.dtype], self.nchw[self.dtype][:4]
            return self.rpn_head(f), self.det_head.forward_roialign(fl, self.scales, self.roi5, self.lvl)

    wl = dict(bench.WORKLOADS[name])
    model = None
    if inputs == "backbone":
        torch.manual_seed(4321)
        model = S.create_model(wl["dataset"], wl["K"], True, True, 0, False, False, 8, 12).eval()
    leg = LayoutLeg(wl, "bf16x3", dev, 1000, inputs, model)
    leg.nchw = {"fp32": [f.float().contiguous() for f in leg.feats]}
    leg.nchw["fp16"] = [f.half() for f in leg.nchw["fp32"]]
    leg.nhwc = {k: [f.contiguous(memory_format=torch.channels_last) for f in v] for k, v in leg.nchw.items()}
    # the RoIAlign feed: 1000 seeded boxes per image (sizes log-uniform 16..512 px, as bench's) on the four FPN levels
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    g = torch.Generator().manual_seed(77)
    H, W = 4 * wl["levels"][0][0], 4 * wl["levels"][0][1]
    props = []
    for _ in range(wl["batch"]):
        size = torch.exp(torch.rand((bench.ROIS_PER_IMG, 2), generator=g) * (6.238 - 2.773) + 2.773)
        ctr = torch.rand((bench.ROIS_PER_IMG, 2), generator=g) * torch.tensor([float(W), float(H)])
        b = torch.cat([ctr - size / 2, ctr + size / 2], 1)
        b[:, 0::2] = b[:, 0::2].clamp(0, float(W))
        b[:, 1::2] = b[:, 1::2].clamp(0, float(H))
        props.append(b.to(dev))
    pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    _, leg.scales, leg.roi5, leg.lvl = pool.assign({str(i): f for i, f in enumerate(leg.nchw["fp32"][:4])}, props, [(H, W)] * wl["batch"])
    return leg


def child(name, dtype, steps, inputs):
    """rocprofv3 target: arm A, then arm B of one leg - warm-up, then `steps` steps each"""
    import torch
    import bench
    leg = make_leg(name, inputs, torch.device("cuda", 0))
    leg.dtype = dtype
    for arm in ("A", "B"):
        leg.arm = arm
        bench.timed_steps(leg, steps, 3, torch.cuda.synchronize)


def kernel_rows(d):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3)
    return rows


def trace(out_lines, steps, inputs, scratch):
    for name in WORKLOADS:
        for dtype in DTYPES:
            d = os.path.join(scratch, "trace_%s_%s" % (name, dtype))
            cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, dtype, "--steps", str(steps), "--inputs", inputs]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:                    # nothing more is started on the GPU after a failed run
                out_lines.append("trace %s %s: rocprofv3 run ended with status %d - no further runs\n%s" % (name, dtype, r.returncode, r.stdout[-800:]))
                return False
            out_lines.append("\n%s, %s maps, arm A then arm B in one process: encoder and copy launches (rocprofv3 --kernel-trace --stats, %d steps + 3 warm-up "
                             "per arm; calls, us per launch)" % (name, dtype, steps))
            for n, (calls, us) in sorted(kernel_rows(d).items(), key=lambda kv: -kv[1][0] * kv[1][1]):
                if "k_encode" in n or "k_roi_align" in n or "copy" in n.lower() or "elementwise" in n.lower():
                    out_lines.append("  %6d x %9.1f us   %s" % (calls, us, n[:110]))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inputs", choices=("backbone", "randn"), default="backbone")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--only-c", action="store_true", help="arm C only (contiguous maps): for a run on another library through SNN_HIP_LIB")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nhwc_features_ab.txt"))
    ap.add_argument("--scratch", default=None, help="where the trace runs leave their output (default: a temporary directory)")
    ap.add_argument("--child", nargs=2, metavar=("WORKLOAD", "DTYPE"))
    a = ap.parse_args()
    if a.scratch is None:
        import tempfile
        a.scratch = tempfile.mkdtemp(prefix="nhwc_ab_")
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.inputs)
    if a.repeats < 3:
        raise SystemExit("at least three repeats per arm")
    import torch
    import bench
    from snn_automotive_object_detection_amd import _lib, ops
    dev = torch.device("cuda", 0)
    arms = ("C",) if a.only_c else ("A", "B", "C")
    lines = ["# tools/time_nhwc_features.py: channels-last maps into both heads - one process, one GPU (%s), library %s," % (torch.cuda.get_device_name(0), os.path.relpath(os.environ.get("SNN_HIP_LIB", _lib.lib_path()), ROOT)),
             "# interleaved repeats of %d steps after %d warm-up steps (bench.timed_steps on bench.Leg, inputs: %s); ms per heads-only step per repeat" % (a.steps, a.warmup, a.inputs),
             "# A = channels-last maps, .contiguous() inside the step, then the NCHW heads (the parent's behaviour); B = the same maps on the NHWC path;",
             "# C = contiguous maps (default path)"]
    verdicts = {}
    for name in WORKLOADS:
        leg = make_leg(name, a.inputs, dev)
        for dtype in DTYPES:
            leg.dtype = dtype
            ms = {arm: [] for arm in arms}
            calls = dict(ops.feature_calls)
            for arm in arms:
                leg.arm = arm
                leg.step()
            torch.cuda.synchronize()
            if not a.only_c:                                      # (arm B ran both heads on the NHWC path, and nothing was converted behind its back)
                now = ops.feature_calls
                assert now["nhwc"] - calls["nhwc"] == 2 and now["no_typed_kernel"] == calls["no_typed_kernel"], (calls, now)
            for _ in range(a.repeats):
                for arm in arms:
                    leg.arm = arm
                    ms[arm].append(1e3 * bench.timed_steps(leg, a.steps, a.warmup, torch.cuda.synchronize) / a.steps)
            lines.append("\n%s, %s maps, detector fed by RoIAlign on the FPN maps (T_rpn %d, T_det %d, batch %d)" % (leg.wl["name"], dtype, leg.wl["T_rpn"], leg.wl["T_det"], leg.wl["batch"]))
            med = {}
            for arm in arms:
                med[arm] = sorted(ms[arm])[len(ms[arm]) // 2]
                lines.append("  arm %s  ms per step: %s   (median %.4f, min-max spread %.1f us)" % (arm, "  ".join("%.4f" % v for v in ms[arm]), med[arm], 1e3 * (max(ms[arm]) - min(ms[arm]))))
            if not a.only_c:
                ok = max(ms["B"]) < min(ms["A"])
                verdicts[(name, dtype)] = ok
                esz = 4 if dtype == "fp32" else 2
                mb = (sum(f.numel() for f in leg.nchw[dtype]) + sum(f.numel() for f in leg.nchw[dtype][:4])) * esz / 1e6
                lines.append("  every repeat of B below every repeat of A: %s;  median saving A - B: %.1f us per step" % ("yes" if ok else "NO", 1e3 * (med["A"] - med["B"])))
                lines.append("  maps read per step (five levels + four): %.0f MB; the copies of A read and write them once more: %.0f MB less in B = %.0f us at 5 TB/s"
                             % (mb, 2 * mb, 2 * mb / 5.0))
            print(json.dumps({"workload": name, "dtype": dtype, "ms_per_step": ms}), flush=True)
        del leg
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)

    def write():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    write()                                               # (the timings are on file before the trace runs start)
    if a.trace:
        torch.cuda.synchronize()
        ok_t = trace(lines, a.steps, a.inputs, a.scratch)
        write()
        if not ok_t:
            return 1
    print("\n".join(lines))
    return 0 if all(verdicts.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
