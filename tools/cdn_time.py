#!/usr/bin/env python3
"""Time, kernels, host synchronisations and library launches of prepare_for_cdn (utils/denoising.py), forward +
backward of a sum, at the training shape: B = 32 frames of 3 targets, dn_number 100 (33 groups, 198 denoising rows a frame),
hidden 256, 900 matching queries, 42-wide keypoints, label_noise_ratio 0.5, box_noise_scale 0.4, 14 classes.

routes: `composition` — prepare_for_cdn_composition: the reference's structure in torch ops with torch's generator, the dead
key-noise draws included — and `drop_in`, prepare_for_cdn as it ships (it packs the targets itself on every call, as a caller
without a criterion would); `drop_in_packed` hands it the PackedTargets a criterion already made.

Three runs of each route, interleaved, in one process.  Per run: wall ms per step, GPU ms from device events, host syncs per
step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler) and library launches per step
(msda_launch_count); then one `summary` row per route with the median of the three runs.  One JSON line each, on stdout and
appended to --out.

    python tools/cdn_time.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from detr_time import DEV, count_kernels, count_syncs, measure  # noqa: E402
from uvhand_amd import _native as MSDA  # noqa: E402
from uvhand_amd.utils import prepare_for_cdn, prepare_for_cdn_composition  # noqa: E402
from uvhand_amd.utils.denoising import _pack  # noqa: E402

B, T_FRAME, DN, HIDDEN, QUERIES, W, K, RATIO, BOX = 32, 3, 100, 256, 900, 42, 14, 0.5, 0.4
ROUTES = ("composition", "drop_in", "drop_in_packed")


def build():
    torch.manual_seed(0)
    enc = nn.Embedding(K + 1, HIDDEN).to(DEV)
    g = torch.Generator().manual_seed(1)
    targets = {"labels": [[int(x) for x in torch.randint(0, K, (T_FRAME,), generator=g)] for _ in range(B)],
               "keypoints": [torch.rand(T_FRAME, W, generator=g).to(DEV) for _ in range(B)]}
    packed = _pack(targets, DEV)
    dn_args = (targets, DN, RATIO, BOX)

    def step(route):
        if route == "composition":
            label, key, _, meta = prepare_for_cdn_composition(dn_args, True, QUERIES, K, HIDDEN, enc)
        else:
            label, key, _, meta = prepare_for_cdn(dn_args, True, QUERIES, K, HIDDEN, enc,
                                                  packed=packed if route == "drop_in_packed" else None)
        assert meta == {"pad_size": 198, "num_dn_group": 33}
        torch.autograd.grad(label.sum() + key.sum(), [enc.weight])
    return step


def count_launches(fn):
    n0 = MSDA.launch_count()
    fn()
    return MSDA.launch_count() - n0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cdn_time.jsonl"))
    args = ap.parse_args()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    step = build()
    gpu_ms = {r: [] for r in ROUTES}
    wall_ms = {r: [] for r in ROUTES}
    last = {}
    for run in range(3):                                              # the routes interleaved, run by run
        for route in ROUTES:
            fn = lambda route=route: step(route)
            wall, gpu = measure(fn, args.iters)
            gpu_ms[route].append(round(gpu, 4))
            wall_ms[route].append(round(wall, 4))
            last[route] = {"tool": "cdn_time", "route": route, "B": B, "targets_per_frame": T_FRAME, "dn_number": DN,
                           "hidden": HIDDEN, "queries": QUERIES, "label_noise_ratio": RATIO, "iters": args.iters,
                           "device": torch.cuda.get_device_name(DEV), "host_syncs_per_step": count_syncs(fn),
                           "kernels_per_step": count_kernels(fn), "library_launches_per_step": count_launches(fn)}
            emit(dict(last[route], run=run, wall_ms_per_step=round(wall, 4), gpu_event_ms_per_step=round(gpu, 4)))
    for route in ROUTES:
        emit(dict(last[route], run="summary", gpu_event_ms_median=statistics.median(gpu_ms[route]), gpu_event_ms_runs=gpu_ms[route],
                  wall_ms_median=statistics.median(wall_ms[route]), wall_ms_runs=wall_ms[route]))


if __name__ == "__main__":
    main()
