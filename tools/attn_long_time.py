#!/usr/bin/env python3
"""Time, host synchronisations, kernels and memory of the decoder self-attention — functions/attention_func.self_attention,
forward + backward — at DINO's two shapes: L = 1098 rows under the contrastive-denoising mask of
cdn_attention_mask(3, 33, 900), and L = 900 unmasked (the 900-query evaluation shape, timed in train mode like the other);
N = 32 frames, 8 heads, E = 256, p = 0.1, fp32, training mode.

Routes: `module` (nn.MultiheadAttention itself: what a masked or long input gets without the streaming core) and `long_core`
(the _AttnFn node on csrc/msda_attn_long.hip: the mask routes it at 1098, MSDA_ATTN_LONG=1 at 900), three runs of each,
interleaved, in one process.  Per run: wall ms per step (host clock around the steps, ending in a device synchronise), GPU ms
from device events, host syncs per step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler) and the
step's peak memory above what was allocated before it; then one `summary` row per route and shape with the median of the three
runs.  One JSON line each, on stdout and appended to --out (default profiles/attn_long_time.jsonl).

--autocast: the same two shapes under torch.autocast("cuda", dtype=torch.bfloat16) with MSDA_ATTN_LONG_BF16=1 (DESIGN.md
§4.27a): `module` is then the stock module under autocast — what such an input gets with the knob unset — and `long_core` the
node on the bf16 streaming kernels; the rows carry "autocast": "bf16".

    python tools/attn_long_time.py [--autocast] [--iters N] [--only ROUTE] [--out FILE]
    python tools/attn_long_time.py [--autocast] --trace-steps 5   # a few long_core steps and nothing else: the run to put under rocprofv3"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from detr_time import DEV, count_kernels, count_syncs, measure, peak_mib  # noqa: E402
from uvhand_amd.functions.attention_func import self_attention  # noqa: E402
from uvhand_amd.utils import cdn_attention_mask  # noqa: E402

N, HEADS, E, P = 32, 8, 256, 0.1
SHAPES = (("dino_train_masked", 1098, True), ("eval_900_unmasked", 900, False))
ROUTES = ("module", "long_core")


def build(L, masked, autocast=False):
    torch.manual_seed(0)
    mha = torch.nn.MultiheadAttention(E, HEADS, dropout=P).to(DEV).train()
    x_qk = torch.randn(L, N, E, device=DEV, requires_grad=True)
    x_v = torch.randn(L, N, E, device=DEV, requires_grad=True)
    go = torch.randn(L, N, E, device=DEV)
    mask = cdn_attention_mask(3, 33, 900, DEV) if masked else None
    assert mask is None or tuple(mask.shape) == (L, L)
    params = list(mha.parameters())

    def step(route):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            if route == "module":
                y = mha(x_qk, x_qk, x_v, attn_mask=mask, need_weights=False)[0]
            else:
                y = self_attention(mha, x_qk, x_v, attn_mask=mask)
        torch.autograd.grad(y, [x_qk, x_v] + params, go.to(y.dtype))
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--autocast", action="store_true", help="bf16 autocast, MSDA_ATTN_LONG_BF16=1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_long_time.jsonl"))
    args = ap.parse_args()
    os.environ["MSDA_ATTN_LONG"] = "1"                  # (read at call time; only the long_core route calls the wrapper)
    if args.autocast:
        os.environ["MSDA_ATTN_LONG_BF16"] = "1"
    extra = {"autocast": "bf16"} if args.autocast else {}

    if args.trace_steps:
        for shape, L, masked in SHAPES:
            step = build(L, masked, args.autocast)
            for _ in range(args.trace_steps):
                step("long_core")
        torch.cuda.synchronize()
        return

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for shape, L, masked in SHAPES:
        step = build(L, masked, args.autocast)
        gpu_ms = {r: [] for r in ROUTES}
        last = {}
        for run in range(3):                                          # the two routes interleaved, run by run
            for route in ROUTES:
                if args.only and route != args.only:
                    continue
                fn = lambda route=route: step(route)
                wall, gpu = measure(fn, args.iters)
                gpu_ms[route].append(round(gpu, 4))
                last[route] = {"tool": "attn_long_time", "shape": shape, "route": route, "L": L, "masked": masked, "N": N,
                               "heads": HEADS, "E": E, "p": P, "iters": args.iters, "device": torch.cuda.get_device_name(DEV),
                               "host_syncs_per_step": count_syncs(fn), "kernels_per_step": count_kernels(fn),
                               "peak_mib_per_step": round(peak_mib(fn), 1), **extra}
                emit(dict(last[route], run=run, wall_ms_per_step=round(wall, 4), gpu_event_ms_per_step=round(gpu, 4)))
        for route in ROUTES:
            if gpu_ms[route]:
                emit(dict(last[route], run="summary", gpu_event_ms_median=statistics.median(gpu_ms[route]),
                          gpu_event_ms_runs=gpu_ms[route]))


if __name__ == "__main__":
    main()
