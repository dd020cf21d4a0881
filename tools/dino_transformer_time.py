#!/usr/bin/env python3
"""Time, host synchronisations, kernels and memory of the DINO DeformableTransformer (modules/dino_deformable_transformer.py,
DESIGN.md §4.31), forward + backward, fp32, training mode, dropout 0 (what config/DINO sets), 6 + 6 layers, d_ffn 2048, 900
queries out of 14 classes with the heads attached, at two pyramids:

  cfg4   28/14/7/4 (S = 1045), N = 32          cfg2x5   96/48/24/12/6 (S = 12 276), N = 8

what = transformer: `reference` — the module with MSDA_DINO_FUSED=0: the two-stage block in the reference's structure (both
keypoint heads on every row, gathers, boolean-mask assignments) and the decoder's query positions / refinement as torch
compositions; the encoder, the attention cores, LayerNorm and FFN nodes are the package's in both — and `drop_in`, the module
as it ships.
what = two_stage: the block alone (proposals, enc_output + norm, class head, selection, keypoint heads; backward of the
selected rows to memory and the parameters) in three forms: `reference`, `composition_rows` (dino_select_composition, heads
after the selection) and `kernel_rows` (the HIP selection, heads after the selection).
what = select (cfg4 only): the selection alone on one set of logits: `two_stage_select` (msda_two_stage_select_f32, the
older one-launch kernel, S <= 8192), `dino_select` (msda_dino_select_forward_f32) and `topk` (dino_select_composition).

Three runs of each route, interleaved, in one process.  Per run: wall ms per step, GPU ms from device events, host syncs per
step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler) and the step's peak memory; then one `summary`
row per route with the median of the three runs.  One JSON line each, on stdout and appended to --out.

    python tools/dino_transformer_time.py [--iters N] [--what transformer|two_stage|select] [--shape cfg4|cfg2x5] [--out FILE]
    python tools/dino_transformer_time.py --trace-steps 3   # a few kernel_rows steps at cfg2x5 and nothing else: for rocprofv3"""
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
from uvhand_amd import _native as MSDA  # noqa: E402
from uvhand_amd.functions import dino_func as DF  # noqa: E402
from uvhand_amd.modules import DinoDeformableTransformer  # noqa: E402
from uvhand_amd.modules.detr import MLP  # noqa: E402

D, HEADS, FFN, LAYERS, K, Q = 256, 8, 2048, 6, 14, 900
SHAPES = {"cfg4": (32, [(28, 28), (14, 14), (7, 7), (4, 4)]),
          "cfg2x5": (8, [(96, 96), (48, 48), (24, 24), (12, 12), (6, 6)])}


def build_module(levels):
    torch.manual_seed(0)
    tr = DinoDeformableTransformer(d_model=D, nhead=HEADS, num_queries=Q, num_encoder_layers=LAYERS, num_decoder_layers=LAYERS,
                                   dim_feedforward=FFN, dropout=0.0, return_intermediate_dec=True, query_dim=4, modulate_hw_attn=True,
                                   deformable_encoder=True, deformable_decoder=True, num_feature_levels=len(levels),
                                   learnable_tgt_init=True, two_stage_type="standard", two_stage_learn_wh=True, decoder_sa_type="sa",
                                   embed_init_tgt=True)
    tr.decoder.class_embed = nn.ModuleList(nn.Linear(D, K) for _ in range(LAYERS))
    tr.decoder.key_embed = nn.ModuleList(MLP(D, D, 42, 3) for _ in range(LAYERS))
    tr.decoder.obj_key_embed = nn.ModuleList(MLP(D, D, 42, 3) for _ in range(LAYERS))
    tr.enc_out_class_embed = nn.Linear(D, K)
    tr.enc_out_key_embed = MLP(D, D, 42, 3)
    tr.enc_out_obj_key_embed = MLP(D, D, 42, 3)
    return tr.to(DEV).train()


def build_transformer(shape):
    N, levels = SHAPES[shape]
    tr = build_module(levels)
    srcs = [torch.randn(N, D, h, w, device=DEV, requires_grad=True) for h, w in levels]
    poss = [torch.randn(N, D, h, w, device=DEV) for h, w in levels]
    masks = [torch.zeros(N, h, w, dtype=torch.bool, device=DEV) for h, w in levels]
    params = list(tr.parameters())

    def step(route):
        DF.FUSED = route == "drop_in"
        hs, refs, hs_enc, ref_enc, init = tr(srcs, masks, None, poss, None)
        loss = sum(h.sum() for h in hs) + sum(r.sum() for r in refs[1:]) + hs_enc.sum()
        torch.autograd.grad(loss, srcs + params, allow_unused=True)
    return step


def build_two_stage(shape):
    N, levels = SHAPES[shape]
    tr = build_module(levels)
    S = sum(h * w for h, w in levels)
    memory = torch.randn(N, S, D, device=DEV, requires_grad=True)
    pad = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    params = [p for n, p in tr.named_parameters() if n.startswith(("enc_out", "two_stage"))]

    def step(route):
        DF.FUSED = route == "kernel_rows"
        tr.two_stage_route = "reference" if route == "reference" else "selected"
        topk, tgt, obj_kp, hand_kp, init = tr.two_stage_block(memory, pad, levels)
        torch.autograd.grad(tgt.sum(), [memory] + params, allow_unused=True)
    return step


def build_select(shape):
    N, levels = SHAPES[shape]
    S = sum(h * w for h, w in levels)
    torch.manual_seed(0)
    cls = torch.randn(N, S, K, device=DEV)
    mem = torch.randn(N, S, D, device=DEV)
    prop = torch.randn(N, S, 42, device=DEV)
    hand, obj = torch.randn(N, S, 42, device=DEV), torch.randn(N, S, 42, device=DEV)

    def step(route):
        if route == "two_stage_select":
            MSDA.two_stage_select(cls, hand, obj, prop, Q)
        elif route == "dino_select":
            MSDA.dino_select_forward(cls, mem, prop, Q)
        else:
            DF.dino_select_composition(cls, mem, prop, Q)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--what", default=None)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_transformer_time.jsonl"))
    args = ap.parse_args()

    if args.trace_steps:
        step = build_two_stage("cfg2x5")
        for _ in range(args.trace_steps):
            step("kernel_rows")
        torch.cuda.synchronize()
        return

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    jobs = (("transformer", build_transformer, ("reference", "drop_in"), args.iters, ("cfg4", "cfg2x5")),
            ("two_stage", build_two_stage, ("reference", "composition_rows", "kernel_rows"), 2 * args.iters, ("cfg4", "cfg2x5")),
            ("select", build_select, ("two_stage_select", "dino_select", "topk"), 10 * args.iters, ("cfg4",)))
    for what, build, routes, iters, shapes in jobs:
        if args.what and what != args.what:
            continue
        for shape in shapes:
            if args.shape and shape != args.shape:
                continue
            step = build(shape)
            N, levels = SHAPES[shape]
            gpu_ms = {r: [] for r in routes}
            last = {}
            for run in range(3):                                          # the routes interleaved, run by run
                for route in routes:
                    fn = lambda route=route: step(route)
                    wall, gpu = measure(fn, iters)
                    gpu_ms[route].append(round(gpu, 4))
                    last[route] = {"tool": "dino_transformer_time", "what": what, "shape": shape, "route": route, "N": N,
                                   "S": sum(h * w for h, w in levels), "Q": Q, "layers": LAYERS, "d_ffn": FFN, "iters": iters,
                                   "device": torch.cuda.get_device_name(DEV), "host_syncs_per_step": count_syncs(fn),
                                   "kernels_per_step": count_kernels(fn), "peak_mib_per_step": round(peak_mib(fn), 1)}
                    emit(dict(last[route], run=run, wall_ms_per_step=round(wall, 4), gpu_event_ms_per_step=round(gpu, 4)))
            for route in routes:
                emit(dict(last[route], run="summary", gpu_event_ms_median=statistics.median(gpu_ms[route]),
                          gpu_event_ms_runs=gpu_ms[route]))
            del step
            DF.FUSED = True
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
