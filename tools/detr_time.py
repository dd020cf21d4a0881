#!/usr/bin/env python3
"""Time, host synchronisations and kernels of the DeformableDETR prediction heads, forward + backward, in one window-32 step
(DESIGN.md §4.14): 6 decoder levels, B * Q = 32 x 300 = 9600 rows per level, hidden 256.

  arctic    two-stage, box-refine ARCTIC heads: per-level class Linear (14) and two 256-256-256-42 MLPs, the six shared
            pose / shape / camera Linears
  assembly  box-refine AssemblyHands heads: per-level class Linear (14) and one 256-256-256-63 MLP, 42-d references

Routes: `composition` (MSDA_HEADS_FUSED=0: the reference's per-level Linears and stacks) and `dropin` (functions.heads_func:
3 + 5 HIP launches).  Per route: wall ms per step (host clock around the steps, ending in a device synchronise), GPU ms from
device events, host syncs per step (torch.cuda.set_sync_debug_mode("warn")) and kernels per step (torch.profiler).  One JSON
line per route and model, on stdout and appended to --out (default profiles/detr_time.jsonl).

`--autocast` measures the same step under torch.autocast("cuda", dtype=torch.bfloat16) instead: `amp_composition` (what autocast
gets by default: the torch composition) and `amp_bf16_node` (MSDA_HEADS_BF16=1: the node on the bf16 MFMA,
csrc/msda_heads_bf16.hip), three runs of each, interleaved, in one session; these rows also carry the step's peak memory above
what was allocated before it.

    python tools/detr_time.py [--iters N] [--only ROUTE] [--autocast] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from uvhand_amd.functions.heads_func import ARCTIC, ASSEMBLY, detr_heads  # noqa: E402
from uvhand_amd.modules.detr import MLP  # noqa: E402

DEV = torch.device("cuda", 0)
L, B, Q, C, K = 6, 32, 300, 256, 14


def build(kind):
    torch.manual_seed(0)
    cls = torch.nn.ModuleList([torch.nn.Linear(C, K) for _ in range(L)]).to(DEV)
    D = 42 if kind == ARCTIC else 63
    heads = [torch.nn.ModuleList([MLP(C, C, D, 3) for _ in range(L)]).to(DEV) for _ in range(2 if kind == ARCTIC else 1)]
    shared = [torch.nn.Linear(C, n).to(DEV) for n in (48, 10, 3, 3, 3, 1)] if kind == ARCTIC else None
    hs = (torch.randn(L, B, Q, C, device=DEV) * 0.5).requires_grad_(True)
    init = torch.rand(B, Q, 42, device=DEV)
    inter = torch.rand(L, B, Q, 42, device=DEV) * 2 - 1
    return hs, init, inter, cls, heads, shared


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


def peak_mib(fn):
    """Peak allocated memory of one step above the level before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--autocast", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detr_time.jsonl"))
    args = ap.parse_args()
    for kind in (ARCTIC, ASSEMBLY):
        hs, init, inter, cls, heads, shared = build(kind)
        params = [p for m in [cls] + heads + (shared or []) for p in m.parameters()]

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.autocast):
                logits, keys, outs = detr_heads(kind, hs, init, inter, cls, heads, shared)
            loss = sum(t.sum() for t in [logits] + keys + outs)
            torch.autograd.grad(loss, [hs] + params)

        routes = [("amp_composition", r) for r in range(3)] + [("amp_bf16_node", r) for r in range(3)] if args.autocast \
            else [("composition", None), ("dropin", None)]
        routes.sort(key=lambda x: (x[1] or 0))                       # autocast: the two routes interleaved, run by run
        for route, run in routes:
            if args.only and route != args.only:
                continue
            os.environ["MSDA_HEADS_FUSED"] = "0" if route == "composition" else "1"
            os.environ["MSDA_HEADS_BF16"] = "1" if route == "amp_bf16_node" else "0"
            wall, gpu = measure(step, args.iters)
            row = {"tool": "detr_time", "model": kind, "route": route, "levels": L, "rows_per_level": B * Q,
                   "hidden": C, "classes": K, "wall_ms_per_step": round(wall, 4),
                   "gpu_event_ms_per_step": round(gpu, 4), "host_syncs_per_step": count_syncs(step),
                   "kernels_per_step": count_kernels(step), "iters": args.iters,
                   "device": torch.cuda.get_device_name(DEV)}
            if args.autocast:
                row.update({"autocast": "bfloat16", "run": run, "peak_mib_per_step": round(peak_mib(step), 1)})
            line = json.dumps(row)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    os.environ.pop("MSDA_HEADS_FUSED", None)
    os.environ.pop("MSDA_HEADS_BF16", None)


if __name__ == "__main__":
    main()
