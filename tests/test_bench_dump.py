"""bench.py --dump-outputs: the files it writes (CPU), and on the GPU box that they hold what the timed step computed on
bench's seeded inputs (the CPU oracle recomputes it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT, near_boundary_mask, rel_err


def test_dump_outputs_writes_whole_arrays_in_float32_or_float64(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"output": torch.rand(2, 3, 4, generator=g), "grad_value": torch.rand(5, generator=g).to(torch.bfloat16),
              "grad_f64": torch.rand(3, generator=g, dtype=torch.float64)}
    written = bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == sorted(name + ".npy" for name in arrays)
    for name, t in arrays.items():
        a = np.load(tmp_path / (name + ".npy"))
        assert written[name] == (tuple(t.shape), False)
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert np.array_equal(a, t.double().numpy())


def test_dump_outputs_samples_the_same_elements_within_the_limit(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"a": torch.rand(1000, 7, generator=g), "b": torch.rand(300, generator=g)}
    limit = 4 * 2000 + 4096 * len(arrays)                          # room for 2000 of the 7300 elements
    first = bench.dump_outputs(str(tmp_path / "x"), arrays, limit_bytes=limit)
    assert first == bench.dump_outputs(str(tmp_path / "y"), arrays, limit_bytes=limit)
    total = 0
    for name, t in arrays.items():
        x, y = (np.load(tmp_path / d / (name + ".npy")) for d in ("x", "y"))
        assert np.array_equal(x, y)
        flat = t.reshape(-1).numpy()
        pos = {v: i for i, v in enumerate(flat.tolist())}
        idx = np.array([pos[v] for v in x.tolist()])
        assert x.ndim == 1 and first[name] == (x.shape, True)
        assert x.size == flat.size * (limit - 4096 * len(arrays)) // (4 * 7300)
        assert np.all(np.diff(idx) > 0)                            # distinct elements, in storage order
        total += os.path.getsize(tmp_path / "x" / (name + ".npy"))
    assert total <= limit


@pytest.mark.gpu
def test_bench_dump_is_the_last_timed_step(oracle, tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5",
                          "--no-table", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert res["steps"] == 30 and res["ms_per_step"] > 0
    assert "median of 1 blocks of 30 steps" in res["config"]["timing"]
    host, _, _ = bench.make_inputs("cfg2_decoder", 1000, None)          # bench's rank-0 inputs
    h = {k: v.double().numpy() if v.is_floating_point() else v.numpy() for k, v in host.items()}
    args = (h["value"], h["shapes"], h["lsi"], h["loc"], h["attn"])
    ref_out = oracle.forward(*args)
    ref_gv, ref_gl, ref_ga = oracle.backward(h["go"], *args)
    got = {name: np.load(tmp_path / (name + ".npy")) for name in ("output", "grad_value", "grad_sampling_loc", "grad_attn_weight")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["output"].shape == ref_out.shape and got["grad_sampling_loc"].shape == ref_gl.shape
    assert rel_err(got["output"], ref_out) < 5e-6
    assert rel_err(got["grad_value"], ref_gv) < 2e-5
    assert rel_err(got["grad_attn_weight"], ref_ga) < 2e-5
    keep = ~near_boundary_mask({"shapes": h["shapes"], "loc": h["loc"]})
    assert rel_err(got["grad_sampling_loc"][keep], ref_gl[keep]) < 2e-5
