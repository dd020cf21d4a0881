#!/usr/bin/env python3
"""Time, kernels, host synchronisations and peak memory of the input-projection neck, forward + backward, in one window-32
ARCTIC training step: N = 32 frames, backbone features 384 / 768 / 1536 channels at 28^2 / 14^2 / 7^2, the
3x3 stride-2 level on the last one (4^2), hidden 256, GroupNorm(32), the 30 % feature mask drawn per step.

Routes: `composition` (MSDA_NECK_FUSED=0: per level Conv2d with bias, GroupNorm, uniform_() > 0.3, multiply — the reference's
loop) and `dropin` (functions.neck_func: the convs without bias, then 1 + 2 HIP launches for all levels).  Per route and run:
GPU ms from device events, wall ms, kernels per step (torch.profiler), host syncs per step and peak memory above the resident
tensors.  `--runs` timed runs after the warm-up (default 3; report their range).  `--conv-ab` times the three 1x1
convolutions as F.conv2d and as a batched matmul.  One JSON line per measurement, on stdout and appended to --out (default
profiles/neck_time.jsonl).

    python tools/neck_time.py [--iters N] [--runs R] [--only composition|dropin] [--conv-ab] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from uvhand_amd.functions.neck_func import input_proj_levels, output_shapes  # noqa: E402

DEV = torch.device("cuda", 0)
N, HIDDEN = 32, 256
LEVELS = [(384, 28, 1), (768, 14, 1), (1536, 7, 1), (1536, 7, 3)]          # (C_in, H = W, kernel)


def build():
    torch.manual_seed(0)
    xs, convs, norms = [], [], []
    for cin, hw, k in LEVELS:
        xs.append(torch.randn(N, cin, hw, hw, device=DEV, requires_grad=True))
        convs.append(torch.nn.Conv2d(cin, HIDDEN, k, stride=2 if k == 3 else 1, padding=1 if k == 3 else 0).to(DEV))
        norms.append(torch.nn.GroupNorm(32, HIDDEN).to(DEV))
    xs[3] = xs[2]                                                      # the extra level reads the last backbone feature
    return xs, convs, norms


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


def measure(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, a.elapsed_time(b) / iters


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20


def emit(args, rec):
    rec.update({"tool": "neck_time", "frames": N, "hidden": HIDDEN, "iters": args.iters,
                "device": torch.cuda.get_device_name(DEV)})
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def run_routes(args, step, what):
    for route in ("composition", "dropin"):
        if args.only and route != args.only:
            continue
        os.environ["MSDA_NECK_FUSED"] = "0" if route == "composition" else "1"
        for _ in range(5):
            step()
        runs = [measure(step, args.iters) for _ in range(args.runs)]
        gpu = [round(g, 4) for _, g in runs]
        emit(args, {"what": what, "route": route, "gpu_event_ms_per_step": gpu, "gpu_event_ms_min": min(gpu),
                    "gpu_event_ms_max": max(gpu), "wall_ms_per_step": [round(w, 4) for w, _ in runs],
                    "kernels_per_step": count_kernels(step), "host_syncs_per_step": count_syncs(step),
                    "peak_mib_per_step": round(peak_mib(step), 2)})
    os.environ.pop("MSDA_NECK_FUSED", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--conv-ab", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neck_time.jsonl"))
    args = ap.parse_args()
    xs, convs, norms = build()
    params = [p for m in convs + norms for p in m.parameters()]
    leaves = xs[:3] + params

    def step():
        uniforms = [torch.empty(s, device=DEV).uniform_() for s in output_shapes(xs, convs)]
        outs = input_proj_levels(xs, convs, norms, uniforms)
        torch.autograd.grad(sum(o.sum() for o in outs), leaves)

    if args.conv_ab:
        w = [c.weight for c in convs[:3]]

        def conv_step():
            ys = [F.conv2d(x, c.weight) for x, c in zip(xs[:3], convs[:3])]
            torch.autograd.grad(sum(y.sum() for y in ys), xs[:3] + w)

        def bmm_step():
            ys = [torch.matmul(c.weight.flatten(1), x.flatten(2)) for x, c in zip(xs[:3], convs[:3])]
            torch.autograd.grad(sum(y.sum() for y in ys), xs[:3] + w)

        for name, fn in (("conv2d", conv_step), ("matmul", bmm_step)):
            for _ in range(5):
                fn()
            gpu = [round(measure(fn, args.iters)[1], 4) for _ in range(args.runs)]
            emit(args, {"what": "1x1 levels, forward + backward", "route": name, "gpu_event_ms_per_step": gpu,
                        "gpu_event_ms_min": min(gpu), "gpu_event_ms_max": max(gpu), "kernels_per_step": count_kernels(fn)})
        return
    run_routes(args, step, "conv + GroupNorm + mask, forward + backward")


if __name__ == "__main__":
    main()
