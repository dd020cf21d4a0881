"""bench.py's two kinds of run on the GPU box: a plain run carries the headline and nothing measured outside the timed steps;
--full adds the other launch modes, the kernels on their own and the roofline (the table and the CPU baseline, its two
longest parts, are skipped here)."""
import json
import os
import subprocess
import sys

import pytest

import bench
from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = {"kernels", "roofline", "eager_ms_per_step", "graph1_ms_per_step", "workloads", "modules", "layers",
             "cpu_baseline", "gpu_over_cpu"}


def _bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]
                         + list(extra), capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, got %d" % len(lines)
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only():
    res = _bench()
    assert res["metric"] == bench.METRIC and res["unit"] == "samples/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["steps"] == 20 and res["warmup"] == 5 and res["ms_per_step"] > 0
    n = bench.WORKLOADS["cfg2_decoder"][0]
    assert res["value"] == pytest.approx(n * 1e3 / res["ms_per_step"], rel=1e-6)
    assert not FULL_ONLY & (set(res) | set(res["config"]))


def test_full_run_adds_launch_modes_kernels_and_roofline():
    res = _bench("--full", "--no-table", "--no-cpu-baseline")
    assert res["steps"] == 20 and res["ms_per_step"] > 0
    assert res["kernels"]["fwd"]["ms"] > 0 and res["kernels"]["bwd"]["ms"] > 0
    assert res["roofline"]["ms"] == res["kernels"]["bwd"]["ms"] and res["roofline"]["copy_GBps_measured"] > 0
    assert res["eager_ms_per_step"] > 0 and res["config"]["eager_ms_per_step"] == res["eager_ms_per_step"]
    assert res["graph1_ms_per_step"] > 0 and res["config"]["graph1_ms_per_step"] == res["graph1_ms_per_step"]
    assert not {"workloads", "modules", "layers", "cpu_baseline"} & set(res)
