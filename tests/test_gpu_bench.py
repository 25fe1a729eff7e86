"""bench.py's two kinds of run on the GPU box: a plain run prints the headline line and measures nothing else; --full adds the
per-kernel breakdown, the roofline and the held clock (the CPU baseline and the side legs, minutes of host time, stay off here)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "held_clock", "breakdown_ms", "heads_tflops", "exchange", "cpu_baseline", "extra")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "SNN_DP_DEVICE", "SNN_DIST_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--inputs", "randn"] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only(gpu_device):
    out = _bench()
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["unit"] == "images/s"
    assert out["steps"] == 3 and out["warmup"] == 1
    assert not [k for k in FULL_ONLY if k in out], sorted(out)


def test_full_run_adds_what_it_measures_besides_the_headline(gpu_device):
    out = _bench("--full", "--no-extra", "--no-cpu-baseline")
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["roofline"]["launch_ms"] > 0 and out["breakdown_ms"]["rpn_head"] > 0 and out["heads_tflops"] > 0
    assert out["exchange"]["ranks"] == 1 and out["exchange"]["ms"] is None
    assert out["cpu_baseline"] is None and "held_clock" in out and "extra" not in out
