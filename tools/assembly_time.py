#!/usr/bin/env python3
"""GPU time and host synchronisations of the AssemblyHands transformer, HIP events around eager calls:

  refine   the decoder's refinement alone at N x 300 queries (42-d refpoints in, 3 classes): the kernel against the
           reference's composition (MSDA_ASSEMBLY_FUSED off)
  whole    forward + backward of the whole transformer in the path AssemblyHands trains (one-stage, with_box_refine: d 256,
           6 + 6 layers, 300 queries, heads as the model attaches them), knob 1 against 0
  syncs    host synchronisations per forward + backward of `whole` and per decoder forward, counted with
           torch.cuda.set_sync_debug_mode("warn"), knob 1 and 0

    python tools/assembly_time.py [cfg4|cfg2]... [--out FILE]
cfg4: N = 32 frames, levels 28/14/7/4 (S = 1045); cfg2: N = 2, levels 48/24/12/6 (S = 3060).  One JSON line per figure, on
stdout and appended to FILE (default profiles/assembly_time.jsonl)."""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

from uvhand_amd.functions import assembly_func as AF  # noqa: E402

DEV = torch.device("cuda", 0)
CFGS = {"cfg4": (32, [(28, 28), (14, 14), (7, 7), (4, 4)]), "cfg2": (2, [(48, 48), (24, 24), (12, 12), (6, 6)])}
OUT = [os.path.join(ROOT, "profiles", "assembly_time.jsonl")]


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
    line = json.dumps(kw)
    print(line, flush=True)
    with open(OUT[0], "a") as f:
        f.write(line + "\n")


def count_syncs(fn):
    """Host synchronisations one call of fn performs (sync debug mode "warn": one warning per synchronising call)."""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return sum("synchroniz" in str(w.message) for w in caught)


def refine(cfg, N):
    g = torch.Generator(device=DEV).manual_seed(0)
    r = torch.rand(N, 300, 42, device=DEV, generator=g)
    cls = torch.randn(N, 300, 3, device=DEV, generator=g)
    tmp = torch.randn(N, 300, 63, device=DEV, generator=g)
    for fused in (True, False):
        AF.FUSED = fused
        emit(cfg=cfg, piece="refine", variant="knob=%d" % int(fused), N=N, Q=300, ms=round(ms(lambda: AF.refine(r, cls, tmp)), 4))
    AF.FUSED = True


def whole(cfg, N, hw):
    import assembly_inputs as AI
    from uvhand_amd.modules import AssemblyDeformableTransformer
    c = dict(AI.CONFIGS["one_stage"], N=N, shapes=hw)
    torch.manual_seed(c["wseed"])
    tr = AssemblyDeformableTransformer(**AI.build_kwargs(c))
    AI.attach_heads(tr, c)
    AI.TI.perturb(tr, c)
    tr = tr.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    srcs = [torch.randn(N, 256, h, w, device=DEV, generator=g) for h, w in hw]
    poss = [torch.randn(N, 256, h, w, device=DEV, generator=g) for h, w in hw]
    masks = [torch.zeros(N, h, w, dtype=torch.bool, device=DEV) for h, w in hw]
    for m in masks:
        m[1::2, :, -max(1, m.shape[2] // 5):] = True
    query = torch.randn(300, 512, device=DEV, generator=g, requires_grad=True)

    def step():
        hs, init_ref, inter, _, _, _ = tr(srcs, masks, poss, query)
        (hs.sum() + init_ref.sum()).backward()

    captured = {}

    def decoder_forward():
        with torch.no_grad():
            tr.decoder(*captured["args"])

    # the decoder's arguments, as the forward builds them (one call with a hook on the decoder)
    h = tr.decoder.register_forward_pre_hook(lambda mod, args: captured.__setitem__("args", tuple(a.detach() for a in args)))
    with torch.no_grad():
        tr(srcs, masks, poss, query)
    h.remove()
    for fused in (True, False):
        AF.FUSED = fused
        emit(cfg=cfg, piece="transformer_fwd_bwd", variant="knob=%d" % int(fused), N=N, ms=round(ms(step, iters=5, warm=2), 3))
        step()                                                      # warm (shape checks, allocations) before counting
        decoder_forward()
        emit(cfg=cfg, piece="host_syncs", variant="knob=%d" % int(fused), N=N, transformer_fwd_bwd=count_syncs(step),
             decoder_fwd=count_syncs(decoder_forward))
    AF.FUSED = True


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT[0] = args[i + 1]
        del args[i:i + 2]
    cfgs = [a for a in args if a in CFGS] or ["cfg4", "cfg2"]
    for cfg in cfgs:
        N, hw = CFGS[cfg]
        refine(cfg, N)
        whole(cfg, N, hw)
