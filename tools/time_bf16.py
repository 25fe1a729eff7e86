"""Precision "bf16" (one bf16 weight plane) against "bf16x3" on one GPU, one process, interleaved repeats: writes profiles/bf16_ab.txt.

bench.py's --precision choices are fixed, so this tool builds bench.Leg itself (Leg.set_precision only sets the heads' attribute) and times
the three workloads - cityscapes (the headline), bdd, stress - with bench's own stepping (bench.timed_steps).  Per workload: R repeats per
precision, interleaved (bf16x3, bf16, bf16x3, ...), images/s per repeat; the gate is "every bf16 repeat faster than every bf16x3 repeat".
The bf16x3 kernels are the parent's instruction for instruction (profiles/bf16_symbol_diff.txt): the partner IS the parent.

--trace: afterwards one `rocprofv3 --kernel-trace --stats` run per precision of the cityscapes and stress steps (each its own child process
under its own timeout; the second starts only if the first ended well) and the conv + LIF, fc6 and fc7 launch times beside the instruction
ratio of 3.
--pmc: afterwards one `rocprofv3 --pmc <8 SQ counters>` run per precision of the cityscapes and stress steps - counters only, no tracing,
each child under its own timeout, chained - and per launch of the conv + LIF, fc6 and fc7 kernels the executed matrix instructions
(SQ_INSTS_MFMA: secondary passes included), SQ_VALU_MFMA_BUSY_CYCLES and the wait counters, averaged over the launches.
usage: python tools/time_bf16.py [--repeats 3] [--steps 20] [--warmup 5] [--inputs backbone|randn] [--trace] [--pmc] [--out profiles/bf16_ab.txt]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PRECS = ("bf16x3", "bf16")


def make_leg(name, inputs, dev):
    import torch
    import bench
    import snn_automotive_object_detection_amd as S
    wl = dict(bench.WORKLOADS[name])
    model = None
    if inputs == "backbone":
        torch.manual_seed(4321)
        model = S.create_model(wl["dataset"], wl["K"], True, True, 0, False, False, 8, 12).eval()
    return bench.Leg(wl, "bf16x3", dev, 1000, inputs, model)


def child(name, prec, steps, inputs):
    """rocprofv3 target: warm-up, then `steps` steps of one workload at one precision"""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    leg = make_leg(name, inputs, dev)
    leg.set_precision(prec)
    bench.timed_steps(leg, steps, 3, torch.cuda.synchronize)


def kernel_rows(d):
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows[r["Name"]] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3)
    return rows


def trace(out_lines, steps, inputs, scratch):
    for name in ("cityscapes", "stress"):
        per = {}
        for prec in PRECS:
            d = os.path.join(scratch, "trace_%s_%s" % (name, prec))
            cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, prec, "--steps", str(steps), "--inputs", inputs]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:                    # nothing more is started on the GPU after a failed run
                out_lines.append("trace %s %s: rocprofv3 run ended with status %d - no further runs\n%s" % (name, prec, r.returncode, r.stdout[-800:]))
                return False
            per[prec] = kernel_rows(d)
        out_lines.append("\n%s: launches per step (rocprofv3 --kernel-trace --stats, %d steps + 3 warm-up; us per launch)" % (name, steps))

        def pick(rows, pred):
            hit = [(n, c, us) for n, (c, us) in rows.items() if pred(n)]
            return max(hit, key=lambda h: h[1] * h[2]) if hit else None
        picks = launch_picks()
        for what, pred in picks:
            a, b = pick(per["bf16x3"], pred), pick(per["bf16"], pred)
            if a and b:
                out_lines.append("  %-28s bf16x3 %9.1f us   bf16 %9.1f us   ratio %.2f (matrix instructions: 3.00)   [%s | %s]"
                                 % (what, a[2], b[2], a[2] / b[2], a[0][:40], b[0][:40]))
            else:
                out_lines.append("  %-28s not found in the kernel stats (%s / %s)" % (what, a and a[0][:40], b and b[0][:40]))
    return True


PMC = ["GRBM_GUI_ACTIVE", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_WAIT_ANY", "SQ_WAVE_CYCLES", "SQ_LDS_BANK_CONFLICT",
       "SQ_WAIT_INST_ANY"]                            # (the group of tools/prof_round.sh's first pass: profiles/r6_default_summary.txt)


def counter_rows(d):
    """{kernel name: {counter: (mean per launch, launches)}} - a launch's value is the sum over its records (one per XCC / shader engine)"""
    import collections
    per = collections.defaultdict(lambda: collections.defaultdict(lambda: collections.defaultdict(float)))
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            per[r["Kernel_Name"]][r["Counter_Name"]][r.get("Dispatch_Id", r.get("Correlation_Id", "0"))] += float(r["Counter_Value"])
    return {k: {c: (sum(v.values()) / len(v), len(v)) for c, v in cs.items()} for k, cs in per.items()}


def pmc(out_lines, steps, inputs, scratch):
    for name in ("cityscapes", "stress"):
        per = {}
        for prec in PRECS:
            d = os.path.join(scratch, "pmc_%s_%s" % (name, prec))
            cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--pmc"] + PMC + ["--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__), "--child", name, prec, "--steps", str(steps), "--inputs", inputs]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:                    # nothing more is started on the GPU after a failed run
                out_lines.append("pmc %s %s: rocprofv3 run ended with status %d - no further runs\n%s" % (name, prec, r.returncode, r.stdout[-800:]))
                return False
            per[prec] = counter_rows(d)
        out_lines.append("\n%s: counters per launch (rocprofv3 --pmc, no tracing; mean over the launches of %d steps + 3 warm-up)" % (name, steps))
        for what, pred in launch_picks():
            for prec in PRECS:
                hit = [(n, cs) for n, cs in per[prec].items() if pred(n)]
                if not hit:
                    out_lines.append("  %-28s %-7s not found in the counter records" % (what, prec))
                    continue
                n, cs = max(hit, key=lambda h: h[1].get("SQ_WAVE_CYCLES", (0, 0))[0] * h[1].get("SQ_WAVE_CYCLES", (0, 0))[1])
                out_lines.append("  %-28s %-7s %s   [%s]" % (what, prec, "  ".join("%s=%.4g" % (c, cs[c][0]) for c in PMC if c in cs), n[:44]))
            a = [cs for n, cs in per["bf16x3"].items() if pred(n)]
            b = [cs for n, cs in per["bf16"].items() if pred(n)]
            if a and b:
                a = max(a, key=lambda cs: cs.get("SQ_WAVE_CYCLES", (0, 0))[0] * cs.get("SQ_WAVE_CYCLES", (0, 0))[1])
                b = max(b, key=lambda cs: cs.get("SQ_WAVE_CYCLES", (0, 0))[0] * cs.get("SQ_WAVE_CYCLES", (0, 0))[1])
                out_lines.append("  %-28s ratio bf16x3 / bf16: %s" % ("", "  ".join("%s %.2f" % (c, a[c][0] / b[c][0]) for c in PMC if c in a and c in b and b[c][0])))
    return True


def launch_picks():
    def sparse_conv(n, conv):                    # k_gemm_lif_sparse[1]<CONV, ..>, mangled or demangled
        if "k_gemm_lif_sparse" not in n:
            return False
        tail = n.split("k_gemm_lif_sparse")[1].lstrip("1")
        return tail.startswith("<true" if conv else "<false") or tail.startswith("ILb1E" if conv else "ILb0E")
    return [("conv + LIF", lambda n: sparse_conv(n, True)), ("fc6 + LIF", lambda n: sparse_conv(n, False)),
            ("fc7 + LIF (G3_FC_LIF_TILE)", lambda n: ("k_gemm_bf16x3<4" in n or "k_gemm_bf16<4" in n or "k_gemm_bf16x3ILi4E" in n or "k_gemm_bf16ILi4E" in n))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inputs", choices=("backbone", "randn"), default="backbone")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_ab.txt"))
    ap.add_argument("--scratch", default=None, help="where the trace runs leave their output (default: a temporary directory)")
    ap.add_argument("--child", nargs=2, metavar=("WORKLOAD", "PRECISION"))
    a = ap.parse_args()
    if a.scratch is None:
        import tempfile
        a.scratch = tempfile.mkdtemp(prefix="bf16_ab_")
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.inputs)
    if a.repeats < 3:
        raise SystemExit("at least three repeats per precision")
    import torch
    import bench
    dev = torch.device("cuda", 0)
    lines = ["# tools/time_bf16.py: precision \"bf16\" (one bf16 weight plane) against \"bf16x3\" - one process, one GPU (%s), interleaved repeats of"
             % torch.cuda.get_device_name(0),
             "# %d steps after %d warm-up steps (bench.timed_steps on bench.Leg, inputs: %s); images/s per repeat" % (a.steps, a.warmup, a.inputs)]
    verdicts = {}
    for name in ("cityscapes", "bdd", "stress"):
        leg = make_leg(name, a.inputs, dev)
        ips = {p: [] for p in PRECS}
        for p in PRECS:                                   # packs the weights of both precisions before anything is timed
            leg.set_precision(p)
            leg.step()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for p in PRECS:
                leg.set_precision(p)
                dt = bench.timed_steps(leg, a.steps, a.warmup, torch.cuda.synchronize)
                ips[p].append(leg.wl["batch"] * a.steps / dt)
        ok = min(ips["bf16"]) > max(ips["bf16x3"])
        verdicts[name] = ok
        lines.append("\n%s (T_rpn %d, T_det %d, batch %d, spike rates %s)" % (leg.wl["name"], leg.wl["T_rpn"], leg.wl["T_det"], leg.wl["batch"], leg.wl["spike_rates"]))
        for p in PRECS:
            lines.append("  %-7s images/s per repeat: %s   (median %.1f)" % (p, "  ".join("%.1f" % v for v in ips[p]), sorted(ips[p])[len(ips[p]) // 2]))
        lines.append("  ratio of medians bf16 / bf16x3: %.3f;  every bf16 repeat faster than every bf16x3 repeat: %s"
                     % (sorted(ips["bf16"])[a.repeats // 2] / sorted(ips["bf16x3"])[a.repeats // 2], "yes" if ok else "NO"))
        print(json.dumps({"workload": name, "images_per_s": ips, "gate": ok}), flush=True)
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
    if a.pmc:
        torch.cuda.synchronize()
        pmc(lines, a.steps, a.inputs, a.scratch)
        write()
    print("\n".join(lines))
    return 0 if all(verdicts.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
