#!/usr/bin/env python3
"""Time, host synchronisations, kernels and memory of the DINO decoder (modules/dino_transformer.py), forward +
backward, at the training shape: N = 32 frames, L = 1098 rows (198 denoising + 900 matching) under cdn_attention_mask(3, 33, 900),
6 layers, d_ffn = 2048, the 4-level pyramid of tools/transformer_time.py's cfg4 (28/14/7/4, S = 1045), 42-wide points, 14
classes with the three heads attached, fp32, training mode, p = 0.1.

decoder routes: `composition` — the reference's structure: nn.MultiheadAttention under the mask, the LayerNorm / Linear modules
themselves, gen_sineembed_for_position and the MLP in torch ops, the refinement with its boolean-mask adds (the sampling is
the package's MSDeformAttn: on a GPU the reference has no other) — and `drop_in`, the module as it ships.
query_pos routes, alone at M = 35 136 rows: `composition`, `table` (table kernel + the FFN node) and `fused` (one launch).

Three runs of each route, interleaved, in one process.  Per run: wall ms per step, GPU ms from device events, host syncs per
step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler) and the step's peak memory; then one `summary`
row per route with the median of the three runs.  One JSON line each, on stdout and appended to --out.

    python tools/dino_decoder_time.py [--iters N] [--what decoder|query_pos] [--out FILE]
    python tools/dino_decoder_time.py --trace-steps 3    # a few drop_in steps and nothing else: the run to put under rocprofv3"""
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
import uvhand_amd.modules.dino_transformer as DT  # noqa: E402
from uvhand_amd.functions import dino_func as DF  # noqa: E402
from uvhand_amd.modules.detr import MLP  # noqa: E402
from uvhand_amd.utils import cdn_attention_mask  # noqa: E402

N, L, D, HEADS, FFN, LAYERS, K, W, P = 32, 1098, 256, 8, 2048, 6, 14, 42, 0.1
LEVELS = [(28, 28), (14, 14), (7, 7), (4, 4)]
_SHIPPED = (DT.self_attention, DT.add_layer_norm, DT.fused_ffn)


def _route(name):
    """Switch the module between the reference's structure and the shipped one."""
    plain = name == "composition"
    DF.FUSED = not plain
    if plain:
        DT.self_attention = lambda mha, q, v, mask=None: mha(q, q, v, attn_mask=mask, need_weights=False)[0]
        DT.add_layer_norm = lambda x, r, norm: norm(x if r is None else x + r)
        DT.fused_ffn = lambda x, l1, act, drop, l2: l2(drop(act(l1(x))))
    else:
        DT.self_attention, DT.add_layer_norm, DT.fused_ffn = _SHIPPED


def build_decoder():
    torch.manual_seed(0)
    layer = DT.DeformableTransformerDecoderLayer(D, FFN, P, "relu", len(LEVELS), HEADS, 4, decoder_sa_type="sa")
    dec = DT.TransformerDecoder(layer, LAYERS, nn.LayerNorm(D), return_intermediate=True, d_model=D, query_dim=4,
                                num_feature_levels=len(LEVELS), deformable_decoder=True, rm_dec_query_scale=True)
    dec.class_embed = nn.ModuleList(nn.Linear(D, K) for _ in range(LAYERS))
    dec.key_embed = nn.ModuleList(MLP(D, D, W, 3) for _ in range(LAYERS))
    dec.obj_key_embed = nn.ModuleList(MLP(D, D, W, 3) for _ in range(LAYERS))
    dec = dec.to(DEV).train()
    S = sum(h * w for h, w in LEVELS)
    tgt = torch.randn(L, N, D, device=DEV, requires_grad=True)
    memory = torch.randn(S, N, D, device=DEV, requires_grad=True)
    ref = torch.randn(L, N, W, device=DEV)
    shapes = torch.tensor(LEVELS, dtype=torch.long, device=DEV)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    ratios = torch.rand(N, len(LEVELS), 2, device=DEV) * 0.3 + 0.7
    pad = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    mask = cdn_attention_mask(3, 33, 900, DEV)
    assert tuple(mask.shape) == (L, L)
    params = list(dec.parameters())

    def step(route):
        _route(route)
        hs, refs = dec(tgt, memory, tgt_mask=mask, memory_key_padding_mask=pad, refpoints_unsigmoid=ref, level_start_index=lsi,
                       spatial_shapes=shapes, valid_ratios=ratios)
        loss = sum(h.sum() for h in hs) + sum(r.sum() for r in refs[1:])
        torch.autograd.grad(loss, [tgt, memory] + params, allow_unused=True)
    return step


def build_query_pos():
    torch.manual_seed(0)
    head = MLP(D, D, D, 2).to(DEV)
    ref = torch.rand(L, N, W, device=DEV) * 2 - 1
    ratios = torch.rand(N, len(LEVELS), 2, device=DEV) * 0.3 + 0.7
    go = torch.randn(L, N, D, device=DEV)
    params = list(head.parameters())

    def step(route):
        DF.FUSED = True
        y = DF.query_pos_composition(ref, ratios, head) if route == "composition" else DF.query_pos(ref, ratios, head, route=route)
        torch.autograd.grad(y, params, go)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--what", default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_decoder_time.jsonl"))
    args = ap.parse_args()

    if args.trace_steps:
        step = build_decoder()
        for _ in range(args.trace_steps):
            step("drop_in")
        torch.cuda.synchronize()
        return

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    jobs = (("decoder", build_decoder, ("composition", "drop_in"), args.iters),
            ("query_pos", build_query_pos, ("composition", "table", "fused"), 4 * args.iters))
    for what, build, routes, iters in jobs:
        if args.what and what != args.what:
            continue
        step = build()
        gpu_ms = {r: [] for r in routes}
        last = {}
        for run in range(3):                                          # the routes interleaved, run by run
            for route in routes:
                fn = lambda route=route: step(route)
                wall, gpu = measure(fn, iters)
                gpu_ms[route].append(round(gpu, 4))
                last[route] = {"tool": "dino_decoder_time", "what": what, "route": route, "N": N, "L": L, "layers": LAYERS,
                               "d_ffn": FFN, "p": P, "iters": iters, "device": torch.cuda.get_device_name(DEV),
                               "host_syncs_per_step": count_syncs(fn), "kernels_per_step": count_kernels(fn),
                               "peak_mib_per_step": round(peak_mib(fn), 1)}
                emit(dict(last[route], run=run, wall_ms_per_step=round(wall, 4), gpu_event_ms_per_step=round(gpu, 4)))
        for route in routes:
            emit(dict(last[route], run="summary", gpu_event_ms_median=statistics.median(gpu_ms[route]),
                      gpu_event_ms_runs=gpu_ms[route]))
        del step
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
