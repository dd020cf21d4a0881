#!/usr/bin/env python3
"""Time, host synchronisations and kernels of one ARCTIC evaluation step after the model forward: B frames
(B = 32 is window 32), synthetic MANO of tests/golden/mano_inputs.py and synthetic objects padded to --obj-len rows (ARCTIC's
meshes are not available here; about 4000 is an assumption).

Routes: `restatement` (MSDA_ARCTIC_EVAL_FUSED=0: prepare_data(flag='eval') with the torch brute-force nearest neighbour and
`.to("cpu")`, then the metrics by the reference's per-frame loops on the CPU, then the per-key means on the host: the
reference's structure; its own route needs pytorch3d and cannot run on ROCm), `dropin` (prepare_data(flag='eval') +
measure_error with the kernels) and `device` (prepare_data(flag='device') + ArcticEvaluator.update).  Per route: wall ms per step and
the device-event interval per step (with some 450 small launches a step the two agree: this is launch-bound step time, not
GPU busy time, which the kernel table gives), host syncs per step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler); and from the
shapes the distance evaluations of the nearest-neighbour launch and the bytes the metric launch must read.  One JSON line per
route, on stdout and appended to --out (default profiles/arctic_eval_time.jsonl).

`--glue` instead compares make_output's HIP glue with the torch glue in one session, `--runs` times over:
`device` and `train` with the kernels of csrc/msda_arctic_output.hip, `device_glue_off` and `train_glue_off` with
MSDA_ARCTIC_OUTPUT_FUSED=0 (the `device` route as it was before those kernels).  `train` is a SmoothNet-style step: the nine
get_arctic_item tensors require grad, prepare_data(flag='train'), a sum over the vertex, joint, 2-d and nearest-neighbour
keys, backward.  Appended to profiles/arctic_output_time.jsonl unless --out says otherwise.

    python tools/arctic_eval_time.py [--iters N] [--batch 32] [--obj-len 4000] [--only ROUTE] [--out FILE] [--glue] [--runs 3]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import arctic_eval_inputs as EI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from smoother_time import count_kernels, count_syncs, measure  # noqa: E402
from uvhand_amd import arctic_eval as AE  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors  # noqa: E402

DEV = torch.device("cuda", 0)


def shape_floors(B, L, NV=778, J=21):
    """(nearest-neighbour distance evaluations of a step, bytes the metric launch must read at least)."""
    nn_evals = 2 * B * L * NV
    metric_bytes = B * (2 * L * 3 * 4 + L * 8 + 2 * NV * (3 * 4 + 4 + 8) + 4 * J * 3 * 4 + 8 * 4)
    return nn_evals, metric_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--obj-len", type=int, default=4000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--glue", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "arctic_output_time.jsonl" if a.glue else "arctic_eval_time.jsonl")
    B, L = a.batch, a.obj_len
    lengths = [L - 37 * i for i in range(11)]                  # arctic_eval_inputs.BIG_LENGTHS at the default --obj-len
    m = dict(EI.mano_models(DEV), arti_head=ObjectTensors.from_arrays(SI.obj_arrays(lengths=lengths)).to(DEV))
    outputs, targets, meta = EI.to_device(*EI.case_inputs("partial", B=B, lengths=lengths, seed=31), DEV)
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    meta = dict(meta, obj_idx=idx, max_len=max_len)
    args = EI.args(DEV)
    metrics = list(AE.DEFAULT_METRICS)
    nn_evals, metric_bytes = shape_floors(B, max_len)
    if a.glue:
        return glue_routes(a, args, outputs, targets, meta, m, metrics, B, max_len)
    for route in ("restatement", "dropin", "device"):
        if a.only and route != a.only:
            continue
        os.environ["MSDA_ARCTIC_EVAL_FUSED"] = "0" if route == "restatement" else "1"
        ev = AE.ArcticEvaluator(metrics)

        def step():
            with torch.no_grad():
                if route == "device":
                    ev.update(AE.prepare_data(args, outputs, targets, meta, EI.CFG, flag="device", models=m))
                    return
                stats = AE.measure_error(AE.prepare_data(args, outputs, targets, meta, EI.CFG, flag="eval", models=m), metrics)
                for k in list(stats):                                   # engine.py:784-794
                    v = stats[k][~np.isnan(stats[k])]
                    stats.overwrite(k, float(v.mean()) if v.size else float("nan"))

        wall, gpu = measure(step, a.iters)
        line = json.dumps({"tool": "arctic_eval_time", "route": route, "batch": B, "obj_len": int(max_len),
                           "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                           "host_syncs_per_step": count_syncs(step), "kernels_per_step": count_kernels(step),
                           "nn_distance_evaluations": nn_evals, "metric_kernel_min_bytes": metric_bytes,
                           "iters": a.iters, "device": torch.cuda.get_device_name(DEV)})
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    os.environ.pop("MSDA_ARCTIC_EVAL_FUSED", None)


TRAIN_KEYS = ("pred.mano.v3d.cam.r", "pred.mano.v3d.cam.l", "pred.mano.j3d.cam.r", "pred.mano.j3d.cam.l", "pred.mano.j2d.r",
              "pred.mano.j2d.l", "pred.object.v.cam", "pred.object.kp2d.norm", "pred.nn_dist_r", "pred.nn_dist_l")


def glue_routes(a, args, outputs, targets, meta, m, metrics, B, max_len):
    items = AE.get_arctic_item(outputs, EI.CFG, DEV)
    leaves = [[t.detach().clone().requires_grad_(True) for t in grp] for grp in items]
    flat = [t for grp in leaves for t in grp]
    meta_in = {k: meta.get(k) for k in ("query_names", "intrinsics", "obj_idx", "max_len")}
    count_syncs(lambda: None)            # torch's one-off notice about the sync debug mode itself names synchronisation too
    steps = {}
    for run in range(a.runs):
        for route in ("device", "device_glue_off", "train", "train_glue_off"):
            if a.only and route != a.only:
                continue
            os.environ["MSDA_ARCTIC_OUTPUT_FUSED"] = "0" if route.endswith("_glue_off") else "1"
            ev = AE.ArcticEvaluator(metrics)

            def step():
                if route.startswith("device"):
                    with torch.no_grad():
                        ev.update(AE.prepare_data(args, outputs, targets, meta, EI.CFG, flag="device", models=m))
                    return
                pred = AE.make_output(args, *leaves, meta_in["query_names"], meta_in["intrinsics"], models=m,
                                      obj_idx=meta_in["obj_idx"], max_len=meta_in["max_len"])
                data = AE.prepare_data(args, None, targets, meta, EI.CFG, pred=pred, flag="train", models=m)
                sum(data[k].sum() for k in TRAIN_KEYS).backward()
                for t in flat:
                    t.grad = None

            steps[route] = step
            wall, gpu = measure(step, a.iters)
            line = json.dumps({"tool": "arctic_eval_time", "mode": "glue", "run": run, "route": route, "batch": B,
                               "obj_len": int(max_len), "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                               "host_syncs_per_step": count_syncs(step), "kernels_per_step": count_kernels(step),
                               "iters": a.iters, "device": torch.cuda.get_device_name(DEV)})
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    os.environ["MSDA_ARCTIC_OUTPUT_FUSED"] = "1"
    for route in ("device", "train"):    # the new kernels' own durations in a profiler trace of one step
        if route not in steps:
            continue
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            steps[route]()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        dur = lambda e: float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))  # noqa: E731
        line = json.dumps({"tool": "arctic_eval_time", "mode": "glue_trace", "route": route, "batch": B, "obj_len": int(max_len),
                           "all_kernels_us": round(sum(dur(e) for e in evs), 1),
                           "kernel_us": {re.search(r"arctic_(?:pose|place|m2aa)_\w+?_kernel", e.name).group(0): round(dur(e), 1) for e in evs
                                         if re.search(r"arctic_(?:pose|place|m2aa)_\w+?_kernel", e.name)},
                           "device": torch.cuda.get_device_name(DEV)})
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    os.environ.pop("MSDA_ARCTIC_OUTPUT_FUSED", None)


if __name__ == "__main__":
    main()
