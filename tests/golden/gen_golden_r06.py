#!/usr/bin/env python3
"""Transformer fixtures, made by RUNNING THE REFERENCE'S DeformableTransformer (needs the reference tree):

  transformer_two_stage.npz  models/arctic_transformer.py:23-259 with two_stage=True, two_stage_learn_xy on: d_model 256,
                             8 heads, FFN 1024, 6 + 6 layers, levels 28/14/7/4 (S = 1045), N = 4 frames (N*S*heads =
                             33 440 encoder items: above the sampling kernels' LDS-stage threshold), 300 queries, 42-d
                             refpoints, dropout 0, a padding mask with per-frame valid ratios and a ragged first row;
  transformer_one_stage.npz  the same class with two_stage=False, d_model 64, 2 heads, 2 + 2 layers, 9 queries.

The class definitions (and util/misc.py's inverse_sigmoid) are taken out of the file with `ast` and executed unchanged, with
the reference's own pure-PyTorch core standing in for the CUDA op, as gen_golden_r04.py does for the stacks.  The per-layer
heads are attached as the model attaches them (tests/golden/two_stage_inputs.py: cls_embed Linear(d, 14) and the 3-layer
42-output MLPs, one per prediction); after the construction checksums are taken every parameter is moved by seeded noise
(two_stage_inputs.perturb: the constructed sampling offsets put every point on a bilinear kink).  Inputs are rebuilt from a seed (two_stage_inputs.py), weights come from
torch.manual_seed at construction: the fixtures hold checksums of both, not the weights.

Stored (sizes: two_stage_inputs.py): all six outputs subsampled by rows plus fp64 row sums of every row, and the leading
columns of every selected refpoint (to match the queries); the input gradients of an explicit-gradient backward
(torch.autograd.backward(outputs, grads): the coordinate outputs hold +inf, so no scalar loss) as fp64 channel sums and a
strided sample; per-parameter gradient sums and a seeded sample of elements of every parameter (two_stage_learn_xy
included: all zeros).

Discrete decisions: for each input seed the generator computes the margin of every discrete decision — the gap at the
top-Q boundary of every frame, the class-argmax gap (top-1 minus top-2 logit) of every selected row, and the argmax gap of
every query's refinement in every decoder layer — and keeps the first seed whose smallest margin is >= 1e-3, so that fp32
reordering cannot flip a selection; the margins are stored.  Nothing of the reference's text is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r06.py
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
REF_TRANSFORMER = REF + "/models/arctic_transformer.py"
REF_MISC = REF + "/util/misc.py"

sys.dont_write_bytecode = True
sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
sys.path.insert(0, REF + "/models")
sys.path.insert(0, HERE)
from ops.functions.ms_deform_attn_func import ms_deform_attn_core_pytorch as ref_core   # noqa: E402
import ops.modules.ms_deform_attn as ref_mod                                             # noqa: E402
import two_stage_inputs as TI                                                            # noqa: E402

MIN_MARGIN = 1e-3


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
    tr = ns["DeformableTransformer"](d_model=cfg["d"], nhead=cfg["heads"], num_encoder_layers=cfg["enc"],
                                     num_decoder_layers=cfg["dec"], dim_feedforward=cfg["ffn"], dropout=0.0,
                                     return_intermediate_dec=True, num_feature_levels=len(cfg["shapes"]),
                                     two_stage=cfg["two_stage"], two_stage_num_proposals=cfg["Q"], two_stage_learn_xy=True)
    width = 42 if cfg["two_stage"] else 2
    TI.attach_heads(tr, cfg, width)
    return tr


def run(tr, cfg, z, requires_grad):
    srcs = [torch.from_numpy(a).requires_grad_(requires_grad) for a in z["srcs"]]
    poss = [torch.from_numpy(a).requires_grad_(requires_grad) for a in z["poss"]]
    masks = [torch.from_numpy(m) for m in z["masks"]]
    query = torch.from_numpy(z["query"]).requires_grad_(requires_grad) if not cfg["two_stage"] else None
    outs = tr(srcs, masks, poss, query)
    return outs, srcs, poss, query


def margins(tr, cfg, outs):
    hs, init_ref, inter, cls, _, _ = outs
    m = {}
    dec = tr.decoder
    def top2(logits):
        t = logits.topk(2, dim=-1)[0]
        return (t[..., 0] - t[..., 1]).flatten()
    if cfg["two_stage"]:
        mx = cls.max(-1)[0]
        srt = mx.sort(dim=1, descending=True)[0]
        Q = cfg["Q"]
        m["boundary"] = (srt[:, Q - 1] - srt[:, Q]).detach()
        idx = torch.topk(mx, Q, dim=1)[1]
        m["select_argmax"] = top2(torch.gather(cls, 1, idx[..., None].expand(-1, -1, cls.shape[-1]))).detach()
    m["refine_argmax"] = torch.cat([top2(dec.cls_embed[i](hs[i])) for i in range(cfg["dec"])]).detach()
    return {k: v.numpy().astype(np.float64) for k, v in m.items()}


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-24s %8.1f KB" % (name, os.path.getsize(path) / 1024))


def fixture(name, ns):
    cfg = TI.CONFIGS[name]
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
    pairs = [(o, g) for o, g in zip(outs, grads) if o.requires_grad]        # the refpoint outputs are detached
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    arrs = {}
    labels = ["hs", "init_reference", "inter_references", "enc_class", "enc_hand", "enc_obj"]
    for lab, o in zip(labels, outs):
        o = o.detach()
        rows = o.reshape(-1, o.shape[-1])
        arrs[lab + "_rows"] = rows[::TI.row_step(lab, cfg)].clone()
        arrs[lab + "_rowsum"] = rows.double().sum(-1)
    if cfg["two_stage"]:
        arrs["init_reference_match"] = outs[1].detach()[..., :TI.MATCH_COLS].clone()
    for i, (s, p) in enumerate(zip(srcs, poss)):
        arrs["grad_src%d_rowsum" % i] = s.grad.double().sum(1)
        arrs["grad_pos%d_rowsum" % i] = p.grad.double().sum(1)
        arrs["grad_src%d_sample" % i] = s.grad.flatten()[::TI.GRAD_STRIDE].clone()
        arrs["grad_pos%d_sample" % i] = p.grad.flatten()[::TI.GRAD_STRIDE].clone()
    if query is not None:
        arrs["grad_query"] = query.grad
    # one row per parameter (named_parameters order = param_names): sums, |sums|, the seeded sample (NaN-padded), None-ness
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
    mg = margins(tr, cfg, [o.detach() if o is not None else None for o in outs] + [None] * (6 - len(outs)))
    for k, v in mg.items():                             # the smallest margins of each kind (all of them are >= MIN_MARGIN)
        arrs["margin_" + k] = np.sort(v)[:16]
    save("transformer_" + name, seed=np.asarray(chosen), input_checksums=TI.checksums(z), state_names=np.asarray(names),
         state_shapes=np.asarray([str(tuple(v.shape)) for v in tr.state_dict().values()]), state_checksums=sums,
         param_names=np.asarray(pnames), **arrs)


if __name__ == "__main__":
    ns = _namespace()
    for name in sys.argv[1:] or ("one_stage", "two_stage"):
        fixture(name, ns)
