#!/usr/bin/env python3
"""AssemblyHands transformer fixtures, made by RUNNING THE REFERENCE'S classes of models/assembly_transformer.py (needs the
reference tree):

  assembly_one_stage.npz  the live path: two_stage=False with the per-layer heads attached (with_box_refine): d_model 256,
                          8 heads, FFN 1024, 6 + 6 layers, levels 28/14/7/4 (S = 1045), N = 4 frames (the encoder runs the
                          sampling kernels' LDS-stage plans), 300 queries, cls_embed Linear(256, 3) and the 63-output
                          keypoint MLPs, 2-d initial refpoints refined to 42-d, a ragged padding mask, dropout 0;
  assembly_two_stage.npz  two_stage=True at the H2O label layout (11 classes) with the 3 queries the selection implies:
                          d_model 64, 2 heads, FFN 128, 2 + 2 layers, the same levels and frames.

As gen_golden_r06.py does: the class definitions (and util/misc.py's inverse_sigmoid) are taken out of the file with `ast`
and executed unchanged on the reference's own pure-PyTorch core; heads, inputs, the seeded perturbation and what is stored
come from assembly_inputs.py / two_stage_inputs.py.  Discrete decisions: the first input seed whose smallest margin is
>= 1e-3 is kept — the refinement's class argmax (top-1 minus top-2 logit of every query in every decoder layer) and, in
two-stage mode, the selection's (assembly_inputs.selection_margins); the smallest margins are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r07.py
"""
import ast
import copy
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.init import constant_, normal_, uniform_, xavier_uniform_

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")
REF_TRANSFORMER = REF + "/models/assembly_transformer.py"
REF_MISC = REF + "/util/misc.py"

sys.dont_write_bytecode = True
sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
sys.path.insert(0, REF + "/models")
sys.path.insert(0, HERE)
from ops.functions.ms_deform_attn_func import ms_deform_attn_core_pytorch as ref_core   # noqa: E402
import ops.modules.ms_deform_attn as ref_mod                                             # noqa: E402
import assembly_inputs as AI                                                             # noqa: E402
import two_stage_inputs as TI                                                            # noqa: E402

MIN_MARGIN = 1e-3
LABELS = AI.LABELS


class _FallbackFn:
    @staticmethod
    def apply(value, shapes, lsi, loc, attn, im2col_step):
        return ref_core(value, shapes, loc, attn)


ref_mod.MSDeformAttnFunction = _FallbackFn


def _namespace():
    tree = ast.parse(open(REF_TRANSFORMER).read())
    wanted = ("DeformableTransformer", "DeformableTransformerEncoderLayer", "DeformableTransformerDecoderLayer",
              "DeformableTransformerEncoder", "DeformableTransformerDecoder", "_get_clones", "_get_activation_fn")
    body = [n for n in tree.body if getattr(n, "name", None) in wanted]
    misc = [n for n in ast.parse(open(REF_MISC).read()).body if getattr(n, "name", None) == "inverse_sigmoid"]
    ns = {"torch": torch, "nn": nn, "F": F, "MSDeformAttn": ref_mod.MSDeformAttn, "copy": copy, "math": math,
          "xavier_uniform_": xavier_uniform_, "constant_": constant_, "uniform_": uniform_, "normal_": normal_,
          "Optional": None, "List": None, "Tensor": torch.Tensor}
    exec(compile(ast.Module(body=misc, type_ignores=[]), REF_MISC, "exec"), ns)
    exec(compile(ast.Module(body=body, type_ignores=[]), REF_TRANSFORMER, "exec"), ns)
    return ns


def build(ns, cfg):
    torch.manual_seed(cfg["wseed"])
    tr = ns["DeformableTransformer"](**AI.build_kwargs(cfg))
    AI.attach_heads(tr, cfg)
    return tr


def run(tr, cfg, z, requires_grad):
    srcs = [torch.from_numpy(a).requires_grad_(requires_grad) for a in z["srcs"]]
    poss = [torch.from_numpy(a).requires_grad_(requires_grad) for a in z["poss"]]
    masks = [torch.from_numpy(m) for m in z["masks"]]
    query = torch.from_numpy(z["query"]).requires_grad_(requires_grad)
    outs = tr(srcs, masks, poss, query)
    return outs, srcs, poss, query


def margins(tr, cfg, outs):
    hs, _, _, cls = outs[:4]
    dec = tr.decoder

    def top2(logits):
        t = logits.topk(2, dim=-1)[0]
        return (t[..., 0] - t[..., 1]).flatten()
    m = {"refine_argmax": torch.cat([top2(dec.cls_embed[i](hs[i])) for i in range(cfg["dec"])]).detach().double().numpy()}
    if cfg["two_stage"]:
        m["select"] = AI.selection_margins(cls)
    return m


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-24s %8.1f KB" % (name, os.path.getsize(path) / 1024))


def fixture(name, ns):
    cfg = AI.CONFIGS[name]
    chosen = None
    for seed in range(1, 40):
        tr = build(ns, cfg)
        TI.perturb(tr, cfg)
        z = TI.inputs(cfg, seed)
        with torch.no_grad():
            outs, *_ = run(tr, cfg, z, False)
        mg = margins(tr, cfg, outs)
        low = min(float(v.min()) for v in mg.values())
        print("  %s seed %d: smallest margin %.3e" % (name, seed, low))
        if low >= MIN_MARGIN:
            chosen = seed
            break
    assert chosen is not None, "no seed with all margins >= %g" % MIN_MARGIN
    tr = build(ns, cfg)
    names, sums = TI.state_checksums(tr)
    TI.perturb(tr, cfg)
    z = TI.inputs(cfg, chosen)
    outs, srcs, poss, query = run(tr, cfg, z, True)
    outs = [o for o in outs if o is not None]
    grads = [torch.from_numpy(g) for g in TI.output_grads(cfg, chosen, [tuple(o.shape) for o in outs])]
    pairs = [(o, g) for o, g in zip(outs, grads) if o.requires_grad]        # the refined refpoints are detached
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    arrs = {}
    for lab, o in zip(LABELS, outs):
        o = o.detach()
        rows = o.reshape(-1, o.shape[-1])
        arrs[lab + "_rows"] = rows[::AI.row_step(lab, cfg)].clone()
        arrs[lab + "_rowsum"] = rows.double().sum(-1)
    for i, (s, p) in enumerate(zip(srcs, poss)):
        arrs["grad_src%d_rowsum" % i] = s.grad.double().sum(1)
        arrs["grad_pos%d_rowsum" % i] = p.grad.double().sum(1)
        arrs["grad_src%d_sample" % i] = s.grad.flatten()[::TI.GRAD_STRIDE].clone()
        arrs["grad_pos%d_sample" % i] = p.grad.flatten()[::TI.GRAD_STRIDE].clone()
    arrs["grad_query_rowsum"] = query.grad.double().sum(1)
    arrs["grad_query_sample"] = query.grad.flatten()[::TI.GRAD_STRIDE].clone()
    params = list(tr.named_parameters())
    pnames = [k for k, _ in params]
    pgrad_sum, pgrad_abssum = np.zeros(len(params)), np.zeros(len(params))
    pgrad_val = np.full((len(params), TI.PGRAD_SAMPLES), np.nan, dtype=np.float32)
    pgrad_none = np.zeros(len(params), dtype=bool)
    for j, (k, p) in enumerate(params):
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        flat = g.detach().flatten()
        idx = TI.pgrad_index(chosen, j, flat.numel())
        pgrad_sum[j] = float(flat.double().sum())
        pgrad_abssum[j] = float(flat.double().abs().sum())
        pgrad_val[j, :idx.size] = flat[torch.from_numpy(idx)].numpy()
        pgrad_none[j] = p.grad is None
    arrs.update(pgrad_sum=pgrad_sum, pgrad_abssum=pgrad_abssum, pgrad_val=pgrad_val, pgrad_none=pgrad_none)
    mg = margins(tr, cfg, [o.detach() for o in outs] + [None] * (6 - len(outs)))
    for k, v in mg.items():                             # the smallest margins of each kind (all of them are >= MIN_MARGIN)
        arrs["margin_" + k] = np.sort(v)[:16]
    save("assembly_" + name, seed=np.asarray(chosen), input_checksums=TI.checksums(z), state_names=np.asarray(names),
         state_shapes=np.asarray([str(tuple(v.shape)) for v in tr.state_dict().values()]), state_checksums=sums,
         param_names=np.asarray(pnames), **arrs)


if __name__ == "__main__":
    ns = _namespace()
    for name in sys.argv[1:] or ("two_stage", "one_stage"):
        fixture(name, ns)
