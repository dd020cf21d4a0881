#!/usr/bin/env python3
"""Time, kernels, host synchronisations and host enqueue time of the tail of the training step: gradient
clipping at 0.1 followed by AdamW over the reference's three parameter groups (util/settings.py:405-434: transformer, backbone,
the sampling-offset / reference-point projections at a tenth of the rate), on the parameter set of the Swin-L backbone as
tools/swin_time.py builds it plus the 6 + 6 layer transformer of tools/ddp_step.py, with random gradients.

Routes, --runs (3) runs of each in one process:
  torch_foreach  torch.nn.utils.clip_grad_norm_(params, 0.1) + torch.optim.AdamW (its default, the foreach form)
  torch_fused    the same clip + torch.optim.AdamW(fused=True)
  dropin         uvhand_amd.optim.AdamW.step(max_norm=0.1): three launches, the gradients read twice and never written

--graph runs the device-state form (torch's capturable flag) in place of the two torch routes above, again --runs runs of each:
  torch_capturable_graph    clip_grad_norm_ + torch.optim.AdamW(capturable=True), captured once into a HIP graph and replayed: the
                            yardstick, the only way to capture this step without this package's class
  dropin                    as above (host-side steps and hyperparameters), for a comparison within the one process
  dropin_capturable         uvhand_amd.optim.AdamW(capturable=True).step(max_norm=0.1), eager: three launches
  dropin_capturable_graph   the same step captured once and replayed
For a captured route the figures are those of graph.replay(); library_launches_in_capture counts what the capture enqueued.

Per run: GPU ms per step from device events after warm-up, kernels per step (torch.profiler), host syncs per step
(torch.cuda.set_sync_debug_mode("warn")) and the host's enqueue time per step (wall clock of the calls alone, the device
drained before and not waited for).  One JSON line each, on stdout and appended to --out (default profiles/optim_time.jsonl).

    python tools/optim_time.py [--graph] [--steps K] [--warmup W] [--runs R] [--only ROUTE] [--no-counts] [--out FILE]

--stats FILE reads the <name>_kernel_stats.csv of a `rocprofv3 --kernel-trace --stats -- python tools/optim_time.py --only
dropin --no-counts --runs 1` run of its own and prints profiles/optim_kernel_stats.csv: per library kernel the calls, the
average time, the elements of the parameter set, and the bytes per second it moved as a share of the 6.3 TB/s a float4 copy
measures on this part, at 4 bytes per element for the sum of squares and 28 for the update.

    python tools/optim_time.py --stats DIR/optim_kernel_stats.csv > profiles/optim_kernel_stats.csv"""
import argparse
import csv
import gc
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

MAX_NORM = 0.1
HBM_TBS = 6.3
ROUTES = ("torch_foreach", "torch_fused", "dropin")
GRAPH_ROUTES = ("torch_capturable_graph", "dropin", "dropin_capturable", "dropin_capturable_graph")
BYTES_PER_ELEM = {"grad_sumsq_kernel": 4, "adamw_step_kernel": 28, "grad_scale_kernel": 8}


def build_model(dev):
    from ddp_step import SyntheticDeformableStack
    from uvhand_amd.modules import Joiner, PositionEmbeddingSine, build_swin_transformer
    torch.manual_seed(0)
    body = build_swin_transformer("swin_L_384_22k", pretrain_img_size=384, out_indices=(1, 2, 3), dilation=False,
                                  use_checkpoint=True, drop_path_rate=0.2)
    model = torch.nn.Module()
    model.backbone = Joiner(body, PositionEmbeddingSine(128, normalize=True))
    model.transformer = SyntheticDeformableStack(6, 6, 300, 0.0)
    return model.to(dev)


def param_groups(model, lr=2e-4, lr_backbone=2e-5, proj_mult=0.1):
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    proj = ("reference_points", "sampling_offsets")
    return [
        {"params": [p for n, p in named if "backbone" not in n and not any(k in n for k in proj)], "lr": lr},
        {"params": [p for n, p in named if "backbone" in n], "lr": lr_backbone},
        {"params": [p for n, p in named if "backbone" not in n and any(k in n for k in proj)], "lr": lr * proj_mult},
    ]


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


def time_steps(fn, steps):
    """(GPU event ms per step, host enqueue ms per step) of `steps` calls back to back."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    host = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, host * 1e3 / steps


def capture(step, dev):
    """`step` captured once on a side stream (after the hygiene uvhand_amd/graphs.py asks for); returns the graph."""
    gc.collect()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    return graph


def stats(path):
    """rocprofv3's kernel stats -> the library kernels' share of the HBM rate (see the module's head)."""
    elems = sum(p.numel() for p in build_model("cpu").parameters() if p.requires_grad)
    out = csv.writer(sys.stdout)
    out.writerow(["kernel", "calls", "average_us", "elements", "bytes_per_element", "TB_per_s", "share_of_%.1f_TB_per_s" % HBM_TBS])
    with open(path) as f:
        for row in csv.DictReader(f):
            for key, nbytes in BYTES_PER_ELEM.items():
                if key in row["Name"]:
                    avg = float(row["AverageNs"])
                    rate = elems * nbytes / avg / 1e3
                    out.writerow([key, row["Calls"], "%.1f" % (avg / 1e3), elems, nbytes, "%.2f" % rate, "%.3f" % (rate / HBM_TBS)])
            if "norm_finish_kernel" in row["Name"]:
                out.writerow(["norm_finish_kernel", row["Calls"], "%.1f" % (float(row["AverageNs"]) / 1e3), "", "", "", ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default=None, choices=ROUTES + GRAPH_ROUTES)
    ap.add_argument("--graph", action="store_true", help="the capturable routes: torch's captured, this class eager and captured")
    ap.add_argument("--no-counts", action="store_true", help="skip the profiler and sync passes (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_time.jsonl"))
    ap.add_argument("--stats", default=None, help="rocprofv3's <name>_kernel_stats.csv: print the library kernels' HBM share")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)
    from uvhand_amd import _native
    from uvhand_amd.optim import AdamW
    dev = torch.device("cuda", 0)
    model = build_model(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    groups = param_groups(model)
    assert sum(len(g["params"]) for g in groups) == len(params) and all(g["params"] for g in groups)
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev)
    base = {"tool": "optim_time", "what": "clip_0.1_adamw", "tensors": len(params), "elements": sum(p.numel() for p in params),
            "groups": [len(g["params"]) for g in groups], "steps": args.steps, "warmup": args.warmup,
            "device": torch.cuda.get_device_name(dev)}
    for route in (GRAPH_ROUTES if args.graph else ROUTES):
        if args.only and route != args.only:
            continue
        if route.startswith("dropin"):
            opt = AdamW(param_groups(model), lr=2e-4, weight_decay=1e-4, capturable=route != "dropin")

            def step():
                opt.step(max_norm=MAX_NORM)
        else:
            opt = torch.optim.AdamW(param_groups(model), lr=2e-4, weight_decay=1e-4, fused=(route == "torch_fused") or None,
                                    capturable=route == "torch_capturable_graph")

            def step():
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
        for _ in range(args.warmup):
            step()
        extra = {}
        if route.endswith("_graph"):
            n0 = _native.launch_count()
            graph = capture(step, dev)
            extra = {"library_launches_in_capture": _native.launch_count() - n0}
            step = graph.replay
            for _ in range(args.warmup):
                step()
        for run in range(args.runs):
            n0 = _native.launch_count()
            ms, host_ms = time_steps(step, args.steps)
            rec = dict(base, route=route, run=run, gpu_event_ms_per_step=round(ms, 4), host_enqueue_ms_per_step=round(host_ms, 4),
                       library_launches_per_step=(_native.launch_count() - n0) / args.steps, **extra)
            if not args.no_counts:
                rec.update(kernels_per_step=count_kernels(step), host_syncs_per_step=count_syncs(step))
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        del opt, step, extra                                       # its exp_avg / exp_avg_sq: 1.6 GB per route (and the graph)
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
