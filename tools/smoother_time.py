#!/usr/bin/env python3
"""Time, host synchronisations and kernels of one SmoothNet training step at window 32: query selection
(get_arctic_item over B * 32 frames of 300 queries, 14 classes), the input masking of train_smoothnet and the default
ArcticSmoother (hidden 512, res 256, 3 blocks; 14.8 M parameters) forward + backward in train mode.

Routes: `composition` (the reference's get_arctic_item and boolean-mask masking restated in torch, MSDA_SMOOTHER_FUSED=0) and
`dropin` (uvhand_amd.arctic_item + the drop-in ArcticSmoother: 1 + 9 forward and 9 backward HIP launches).  Per route and
batch: wall ms per step (host clock around the steps, ending in a device synchronise), GPU ms from device events, host syncs
per step (torch.cuda.set_sync_debug_mode("warn")) and kernels per step (torch.profiler).  One JSON line per route and batch,
on stdout and appended to --out (default profiles/smoother_time.jsonl).

    python tools/smoother_time.py [--iters N] [--batches 1,8] [--only composition|dropin] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from uvhand_amd.arctic_item import DEFAULT_SCALE, get_arctic_item, get_arctic_item_reference, perturb_arctic_item  # noqa: E402
from uvhand_amd.modules import ArcticSmoother  # noqa: E402

DEV = torch.device("cuda", 0)
T, Q, K = 32, 300, 14


class Cfg:
    hand_idx = [12, 13]


def detr_outputs(frames):
    g = torch.Generator().manual_seed(0)
    srcs = [torch.randn(frames, Q, w, generator=g).to(DEV) for w in (3, 3, 48, 10, 1, 3)]
    return {"pred_logits": torch.randn(frames, Q, K, generator=g).to(DEV), "pred_cams": srcs[0:2],
            "pred_mano_params": srcs[2:4], "pred_obj_params": srcs[4:6]}


def reference_perturb(items, p_mask=0.05):
    """engine.py:336-344 as written (boolean indexing, a host randn per parameter)."""
    for idx, out in enumerate(items):
        for p_idx, param in enumerate(out):
            s = DEFAULT_SCALE[idx][p_idx] if isinstance(DEFAULT_SCALE[idx], list) else DEFAULT_SCALE[idx]
            mask = torch.empty(param.shape, device=param.device).uniform_() > (1 - p_mask)
            param[mask] += torch.randn(param[mask].shape).to(param.device) * s
    return items


def count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return sum("synchroniz" in str(w.message) for w in caught)


def count_kernels(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def measure(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return wall, a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoother_time.jsonl"))
    args = ap.parse_args()
    for B in [int(b) for b in args.batches.split(",")]:
        torch.manual_seed(0)
        model = ArcticSmoother(B, T).to(DEV).train()
        params = list(model.parameters())
        outputs = detr_outputs(B * T)
        for route in ("composition", "dropin"):
            if args.only and route != args.only:
                continue
            os.environ["MSDA_SMOOTHER_FUSED"] = "0" if route == "composition" else "1"
            select = get_arctic_item_reference if route == "composition" else get_arctic_item
            perturb = reference_perturb if route == "composition" else perturb_arctic_item

            def step():
                with torch.no_grad():
                    items = perturb(select(outputs, Cfg()))
                smoothed = model(items)
                loss = sum(t.square().sum() for group in smoothed for t in group)
                torch.autograd.grad(loss, params)

            wall, gpu = measure(step, args.iters)
            line = json.dumps({"tool": "smoother_time", "route": route, "batch": B, "window": T, "queries": Q,
                               "params": sum(p.numel() for p in params), "wall_ms_per_step": round(wall, 4),
                               "gpu_event_ms_per_step": round(gpu, 4), "host_syncs_per_step": count_syncs(step),
                               "kernels_per_step": count_kernels(step), "iters": args.iters,
                               "device": torch.cuda.get_device_name(DEV)})
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    os.environ.pop("MSDA_SMOOTHER_FUSED", None)


if __name__ == "__main__":
    main()
