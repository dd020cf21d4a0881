#!/usr/bin/env python3
"""GPU time of the two-stage DeformableTransformer pieces, HIP events around eager calls:

  pos_trans   pos_trans[0:2] (Linear(5376, 1024) + ReLU) forward and forward + backward at M = N x 300 rows: the fused node
              (PE generated in the GEMM's A operand) against PE materialisation plus torch's fp32 GEMMs (the composition);
              TFLOP/s of the forward GEMM (2 M 1024 5376 flop)
  select      the proposals + query selection block (proposals kernel + three heads + selection) against the composition
  whole       forward + backward of the whole two-stage transformer (6 + 6 layers, d 256, heads as the model attaches them)
              with MSDA_TWO_STAGE_FUSED behaviour on (1) and off (0, the composition for all three pieces)

    python tools/transformer_time.py [cfg4|cfg2] [pos_trans|select|whole]...
cfg4: N = 32 frames, levels 28/14/7/4 (S = 1045); cfg2: N = 2, levels 48/24/12/6 (S = 3060).  One JSON line per figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402
from torch import nn  # noqa: E402

from uvhand_amd.functions import two_stage_func as TS  # noqa: E402

DEV = torch.device("cuda", 0)
CFGS = {"cfg4": (32, [(28, 28), (14, 14), (7, 7), (4, 4)]), "cfg2": (2, [(48, 48), (24, 24), (12, 12), (6, 6)])}


def ms(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def emit(**kw):
    print(json.dumps(kw), flush=True)


def pos_trans(cfg, N):
    M = N * 300
    torch.manual_seed(0)
    lin = nn.Linear(5376, 1024).to(DEV)
    r = (torch.randn(M, 42, device=DEV) * 2)
    gy = torch.randn(M, 1024, device=DEV)
    flop = 2.0 * M * 1024 * 5376

    def fused_f():
        with torch.no_grad():
            TS.pos_embed_linear_relu(r, lin)

    def comp_f():
        with torch.no_grad():
            torch.relu(lin(TS.pos_embed_composition(r)))

    def fused_fb():
        TS.pos_embed_linear_relu(r, lin).backward(gy)

    def comp_fb():
        torch.relu(lin(TS.pos_embed_composition(r))).backward(gy)

    for name, fn in (("fused_fwd", fused_f), ("composition_fwd", comp_f), ("fused_fwd_bwd", fused_fb), ("composition_fwd_bwd", comp_fb)):
        t = ms(fn)
        row = dict(cfg=cfg, piece="pos_trans0", variant=name, M=M, ms=round(t, 4))
        if name.endswith("_fwd"):
            row["tflops"] = round(flop / t / 1e9, 1)
        else:
            row["tflops_3gemm_equiv"] = round(2 * flop / t / 1e9, 1)      # forward GEMM + weight-gradient GEMM
        emit(**row)


def select(cfg, N, hw):
    S = sum(h * w for h, w in hw)
    torch.manual_seed(1)
    memory = torch.randn(N, S, 256, device=DEV)
    mask = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    mask[1::2, -S // 10:] = True
    xy = torch.full((40,), -2.94, device=DEV)
    heads = [nn.Linear(256, 14).to(DEV), nn.Linear(256, 42).to(DEV), nn.Linear(256, 42).to(DEV)]

    def block(fused):
        TS.FUSED = fused
        with torch.no_grad():
            om, props = TS.encoder_output_proposals(memory, mask, hw, xy)
            cls, hand, obj = (h(om) for h in heads)
            hand[..., 0::2] += props[..., 0:1]
            obj[..., 0::2] += props[..., 0:1]
            TS.select_queries(cls, hand, obj, props, 300)

    for fused in (True, False):
        emit(cfg=cfg, piece="proposals_select", variant="fused" if fused else "composition", N=N, S=S, ms=round(ms(lambda: block(fused)), 4))
    TS.FUSED = True


def whole(cfg, N, hw):
    import two_stage_inputs as TI
    from uvhand_amd.modules import DeformableTransformer
    c = dict(TI.CONFIGS["two_stage"], N=N, shapes=hw)
    torch.manual_seed(c["wseed"])
    tr = DeformableTransformer(dropout=0.0, return_intermediate_dec=True, two_stage=True)
    TI.attach_heads(tr, c, 42)
    tr = tr.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    srcs = [torch.randn(N, 256, h, w, device=DEV, generator=g) for h, w in hw]
    poss = [torch.randn(N, 256, h, w, device=DEV, generator=g) for h, w in hw]
    masks = [torch.zeros(N, h, w, dtype=torch.bool, device=DEV) for h, w in hw]
    for m in masks:
        m[1::2, :, -max(1, m.shape[2] // 5):] = True

    def step(fused):
        TS.FUSED = fused
        hs, _, _, cls, _, _ = tr(srcs, masks, poss)
        (hs.sum() + cls.sum()).backward()

    for fused in (True, False):
        emit(cfg=cfg, piece="transformer_fwd_bwd", variant="knob=%d" % int(fused), N=N, ms=round(ms(lambda: step(fused), iters=5, warm=2), 3))
    TS.FUSED = True


if __name__ == "__main__":
    args = sys.argv[1:]
    cfgs = [a for a in args if a in CFGS] or ["cfg4", "cfg2"]
    pieces = [a for a in args if a in ("pos_trans", "select", "whole")] or ["pos_trans", "select", "whole"]
    for cfg in cfgs:
        N, hw = CFGS[cfg]
        if "pos_trans" in pieces:
            pos_trans(cfg, N)
        if "select" in pieces:
            select(cfg, N, hw)
        if "whole" in pieces:
            whole(cfg, N, hw)
