#!/usr/bin/env python3
"""Time, kernels, host synchronisations and peak memory of the Swin backbone's training step at the ARCTIC
recipe: Swin-L 384_22k (embed 192, depths 2/2/18/2, heads 6/12/24/48, window 12) built as build_backbone builds it
(out_indices 1-3, use_checkpoint=True, drop_path_rate 0.2, train mode) under Joiner with the sine encoding, over 32 frames of
3 x 224 x 224 with a padding mask; forward + backward of a weighted sum of the three features.

Routes: `composition` (MSDA_SWIN_FUSED=0: the reference's pad / roll / partition / batched matmuls / mask / softmax / reverse
/ crop) and `dropin` (the qkv and proj Linears on the real rows, one HIP launch forward and three backward per block).  Per
route: GPU ms per step from device events after warm-up, kernels per step (torch.profiler), host syncs per step
(torch.cuda.set_sync_debug_mode("warn")) and max_memory_allocated over one step.  Then one attention-only row per stage
geometry (the window-attention node forward + backward on [32 * H * W, 3 C] rows, both routes).  One JSON line each, on
stdout and appended to --out (default profiles/swin_time.jsonl).

--autocast runs the same model and step under torch.autocast("cuda", dtype=torch.bfloat16) and times the routes
`autocast_composition` (what every block takes under autocast by default) and `autocast_bf16` (MSDA_SWIN_BF16=1: the opt-in bf16
form of the node); the attention-only rows then take bf16 qkv rows.  The default remains the fp32 A/B.

--glue times the kernel route without and with MSDA_SWIN_GLUE=1 (the blocks' norms, residual adds and drop-path products and the
patch mergings on HIP) in one process: `dropin` against `dropin_glue`, or with --autocast `autocast_bf16` against
`autocast_bf16_glue`.  The glue does not touch the attention node, so --glue writes no attention-only rows.

--glue-stream (with --autocast --glue) adds the route `autocast_bf16_glue_stream`: MSDA_SWIN_BF16=1, MSDA_SWIN_GLUE=1 and
MSDA_SWIN_GLUE_BF16=1, the glue over the bf16 residual stream of stages 1 to 3 as well.

    python tools/swin_time.py [--autocast] [--glue] [--glue-stream] [--steps K] [--warmup W] [--only ROUTE] [--no-attn] [--no-backbone] [--out FILE]"""
import argparse
import contextlib
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from uvhand_amd.functions.swin_func import window_attention  # noqa: E402
from uvhand_amd.modules import Joiner, PositionEmbeddingSine, build_swin_transformer  # noqa: E402
from uvhand_amd.modules.detr import NestedTensor  # noqa: E402

DEV = torch.device("cuda", 0)
FRAMES, IMG = 32, 224
STAGES = ((56, 56, 192, 6), (28, 28, 384, 12), (14, 14, 768, 24), (7, 7, 1536, 48))    # H, W, C, heads at 224^2


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


def gpu_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(DEV) / 2 ** 20


def emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def set_route(route):
    """The environment a route reads at call time."""
    os.environ["MSDA_SWIN_FUSED"] = "0" if route.endswith("composition") else "1"
    os.environ["MSDA_SWIN_BF16"] = "1" if route.startswith("autocast_bf16") else "0"
    os.environ["MSDA_SWIN_GLUE"] = "1" if route.endswith(("_glue", "_glue_stream")) else "0"
    os.environ["MSDA_SWIN_GLUE_BF16"] = "1" if route.endswith("_glue_stream") else "0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--autocast", action="store_true", help="bf16 autocast: the composition against MSDA_SWIN_BF16=1")
    ap.add_argument("--glue", action="store_true", help="the kernel route without and with MSDA_SWIN_GLUE=1")
    ap.add_argument("--glue-stream", action="store_true",
                    help="with --autocast --glue: also the route with MSDA_SWIN_GLUE_BF16=1 (the glue over the bf16 stream)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-attn", action="store_true")
    ap.add_argument("--no-backbone", action="store_true", help="only the attention-only rows")
    ap.add_argument("--no-counts", action="store_true", help="skip the profiler / sync / memory passes (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_time.jsonl"))
    args = ap.parse_args()
    routes = ("autocast_composition", "autocast_bf16") if args.autocast else ("composition", "dropin")
    if args.glue_stream and not (args.glue and args.autocast):
        ap.error("--glue-stream needs --autocast --glue: outside autocast the residual stream is fp32")
    if args.glue:
        routes = (routes[1], routes[1] + "_glue") + ((routes[1] + "_glue_stream",) if args.glue_stream else ())
        args.no_attn = True
    amp = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if args.autocast else contextlib.nullcontext
    torch.manual_seed(0)
    body = build_swin_transformer("swin_L_384_22k", pretrain_img_size=384, out_indices=(1, 2, 3), dilation=False,
                                  use_checkpoint=True, drop_path_rate=0.2)
    model = Joiner(body, PositionEmbeddingSine(128, normalize=True)).to(DEV).train()
    params = [p for p in model.parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(1)
    img = torch.randn(FRAMES, 3, IMG, IMG, generator=g).to(DEV)
    mask = torch.zeros(FRAMES, IMG, IMG, dtype=torch.bool, device=DEV)
    mask[FRAMES // 2:, :, IMG - 32:] = True
    weights = None

    def step():
        nonlocal weights
        with amp():
            feats, _ = model(NestedTensor(img, mask))
        if weights is None:
            weights = [torch.randn(f.tensors.shape, generator=g).to(DEV) for f in feats]
        loss = sum((f.tensors * w).sum() for f, w in zip(feats, weights))
        torch.autograd.grad(loss, params)

    for route in routes:
        if args.no_backbone or (args.only and route != args.only):
            continue
        set_route(route)
        ms = gpu_ms(step, args.steps, args.warmup)
        rec = {"tool": "swin_time", "what": "backbone_fwd_bwd", "route": route, "backbone": "swin_L_384_22k", "frames": FRAMES,
               "img": IMG, "checkpoint": True, "drop_path_rate": 0.2, "gpu_event_ms_per_step": round(ms, 3),
               "steps": args.steps, "warmup": args.warmup, "autocast": "bf16" if args.autocast else None,
               "glue": route.endswith(("_glue", "_glue_stream")), "glue_stream": route.endswith("_glue_stream")}
        if not args.no_counts:
            rec.update(kernels_per_step=count_kernels(step), host_syncs_per_step=count_syncs(step),
                       max_memory_allocated_mb=round(peak_mb(step), 1))
        rec["device"] = torch.cuda.get_device_name(DEV)
        emit(args, rec)

    if not args.no_attn:
        for (H, W, C, nH) in STAGES:
            ws = 12
            act = torch.bfloat16 if args.autocast else torch.float32
            qkv = torch.randn(FRAMES * H * W, 3 * C, device=DEV).to(act).requires_grad_(True)
            bias = torch.randn(3 * C, device=DEV, requires_grad=True)
            table = torch.randn((2 * ws - 1) ** 2, nH, device=DEV, requires_grad=True)
            go = torch.randn(FRAMES * H * W, C, device=DEV).to(act)
            geo = (FRAMES, H, W, C, nH, ws, ws // 2)

            def attn():
                with amp():
                    out = window_attention(qkv, bias, table, geo)
                torch.autograd.grad(out, (qkv, bias, table), go)

            for route in routes:
                if args.only and route != args.only:
                    continue
                set_route(route)
                rec = {"tool": "swin_time", "what": "attention_fwd_bwd", "route": route, "frames": FRAMES, "H": H, "W": W,
                       "C": C, "heads": nH, "window": ws, "shift": ws // 2,
                       "gpu_event_ms": round(gpu_ms(attn, args.steps, args.warmup), 4)}
                if not args.no_counts:
                    rec.update(kernels=count_kernels(attn), max_memory_allocated_mb=round(peak_mb(attn), 1))
                emit(args, rec)
    os.environ.pop("MSDA_SWIN_FUSED", None)
    os.environ.pop("MSDA_SWIN_BF16", None)
    os.environ.pop("MSDA_SWIN_GLUE", None)
    os.environ.pop("MSDA_SWIN_GLUE_BF16", None)


if __name__ == "__main__":
    main()
