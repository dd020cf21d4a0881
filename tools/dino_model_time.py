#!/usr/bin/env python3
"""Time, host synchronisations, kernels and memory of the DINO model's prediction heads (modules/dino.py),
forward + backward, fp32, at the training window's shape: 6 decoder layers x 32 frames x (198 denoising + 900 matching) queries =
210 816 rows, hidden 256, 14 classes, shared heads, every reference but the first requiring grad ("look forward twice").

what = heads:  `reference` — functions.heads_func.dino_heads_reference, the reference's per-layer composition (dino.py:329-347) —
               and `drop_in`, functions.heads_func.dino_heads: three forward launches, five backward ones and
               msda_heads_ref_backward_f32.  The stacks of hs and of references[1:] that the node needs are inside its time.
what = model:  DINO.heads (dn_post_process, the output dict, the interm class head) on the same tensors, with
               MSDA_HEADS_FUSED=0 (`reference`) and as it ships (`drop_in`).

Three runs of each route, interleaved, in one process.  Per run: wall ms per step, GPU ms from device events, host syncs per
step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler) and the step's peak memory; then one `summary`
row per route with the median of the three runs.  One JSON line each, on stdout and appended to --out.

    python tools/dino_model_time.py [--iters N] [--what heads|model] [--out FILE]
    python tools/dino_model_time.py --trace-steps 3   # a few drop_in steps of the heads and nothing else: for rocprofv3"""
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

from detr_time import DEV, count_kernels, count_syncs, measure, peak_mib  # noqa: E402
from uvhand_amd.functions.heads_func import dino_heads, dino_heads_reference  # noqa: E402
from uvhand_amd.modules import DINO, DinoDeformableTransformer  # noqa: E402

D, HEADS, LAYERS, K, Q, N = 256, 8, 6, 14, 900, 32
SINGLE_PAD, GROUPS = 3, 33                                       # 2 * 3 * 33 = 198 denoising rows in front of the 900
PAD = 2 * SINGLE_PAD * GROUPS


class _Backbone(nn.Sequential):
    num_channels, strides = [8], [8]


def build_model():
    torch.manual_seed(0)
    tr = DinoDeformableTransformer(d_model=D, nhead=HEADS, num_queries=Q, num_encoder_layers=1, num_decoder_layers=LAYERS,
                                   dim_feedforward=64, dropout=0.0, return_intermediate_dec=True, query_dim=4, modulate_hw_attn=True,
                                   deformable_encoder=True, deformable_decoder=True, num_feature_levels=2,
                                   learnable_tgt_init=True, two_stage_type="standard", decoder_sa_type="sa", embed_init_tgt=True)
    model = DINO(_Backbone(), tr, num_classes=K, num_queries=Q, aux_loss=True, iter_update=True, query_dim=4, num_feature_levels=2,
                 nheads=HEADS, two_stage_type="standard", dn_number=100, dn_labelbook_size=K)
    with torch.no_grad():                                         # the constructor zeroes the keypoint heads' last layers
        for mlp in (model.key_embed[0], model.obj_key_embed[0]):
            nn.init.xavier_uniform_(mlp.layers[-1].weight)
    return model.to(DEV).train()


def build_inputs():
    g = torch.Generator().manual_seed(1)
    L = PAD + Q
    base = [torch.randn(N, L, D, generator=g).to(DEV).requires_grad_(True) for _ in range(LAYERS)]
    # the decoder's points lie in (-1, 1); every one but the first carries a gradient
    pts = [(torch.rand(N, L, 42, generator=g) * 2 - 1).to(DEV).requires_grad_(l > 0) for l in range(LAYERS + 1)]
    hs_enc = torch.randn(1, N, Q, D, generator=g).to(DEV)
    ref_enc = [torch.rand(1, N, Q, 42, generator=g).to(DEV) for _ in range(2)]
    return base, pts, hs_enc, ref_enc


def head_params(model):
    mods = [model.class_embed[0], model.key_embed[0], model.obj_key_embed[0], model.mano_pose_embed[0], model.mano_beta_embed[0],
            model.hand_cam[0], model.obj_cam[0], model.obj_rot[0], model.obj_rad[0]]
    return [p for m in mods for p in m.parameters()]


def build_heads():
    model = build_model()
    base, pts, _, _ = build_inputs()
    shared = [model.mano_pose_embed[0], model.mano_beta_embed[0], model.hand_cam[0], model.obj_cam[0], model.obj_rot[0],
              model.obj_rad[0]]
    leaves = base + pts[1:LAYERS] + head_params(model)

    def step(route):
        fn = dino_heads if route == "drop_in" else dino_heads_reference
        logits, keys, outs = fn(base, pts[:-1], model.class_embed, model.key_embed, model.obj_key_embed, shared)
        loss = sum(t.sum() for t in [logits] + list(keys) + list(outs))
        torch.autograd.grad(loss, leaves)
    return step


def build_whole():
    model = build_model()
    base, pts, hs_enc, ref_enc = build_inputs()
    leaves = base + pts[1:LAYERS] + head_params(model)

    def tensors(v):
        if torch.is_tensor(v):
            return [v] if v.requires_grad else []
        if isinstance(v, dict):
            return [t for x in v.values() for t in tensors(x)]
        if isinstance(v, (list, tuple)):
            return [t for x in v for t in tensors(x)]
        return []

    def step(route):
        os.environ["MSDA_HEADS_FUSED"] = "1" if route == "drop_in" else "0"
        out = model.heads(base, pts, hs_enc, ref_enc, {"pad_size": PAD, "num_dn_group": GROUPS})
        loss = sum(t.sum() for t in tensors(out))
        torch.autograd.grad(loss, leaves)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--what", default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_model_time.jsonl"))
    args = ap.parse_args()

    if args.trace_steps:
        step = build_heads()
        for _ in range(args.trace_steps):
            step("drop_in")
        torch.cuda.synchronize()
        return

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    routes = ("reference", "drop_in")
    for what, build in (("heads", build_heads), ("model", build_whole)):
        if args.what and what != args.what:
            continue
        step = build()
        gpu_ms = {r: [] for r in routes}
        last = {}
        for route in routes:                                              # the counters' own first use stays out of the rows
            count_syncs(lambda route=route: step(route))
        for run in range(3):                                              # the routes interleaved, run by run
            for route in routes:
                fn = lambda route=route: step(route)
                wall, gpu = measure(fn, args.iters)
                gpu_ms[route].append(round(gpu, 4))
                last[route] = {"tool": "dino_model_time", "what": what, "route": route, "N": N, "rows_per_layer": N * (PAD + Q),
                               "layers": LAYERS, "hidden": D, "K": K, "iters": args.iters,
                               "device": torch.cuda.get_device_name(DEV), "host_syncs_per_step": count_syncs(fn),
                               "kernels_per_step": count_kernels(fn), "peak_mib_per_step": round(peak_mib(fn), 1)}
                emit(dict(last[route], run=run, wall_ms_per_step=round(wall, 4), gpu_event_ms_per_step=round(gpu, 4)))
        for route in routes:
            emit(dict(last[route], run="summary", gpu_event_ms_median=statistics.median(gpu_ms[route]),
                      gpu_event_ms_runs=gpu_ms[route]))
        del step
        os.environ.pop("MSDA_HEADS_FUSED", None)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
