#!/usr/bin/env python3
"""Swin fixtures, made by RUNNING THE REFERENCE'S SwinTransformer / BasicLayer (models/swin_transformer.py),
PositionEmbeddingSine (models/position_encoding.py) and Joiner (models/backbone.py) on the CPU, over the seeded inputs of
swin_inputs.py:

  swin_<case>.npz   init/<key>         sha256 of each state_dict entry as constructed under the case's seed
                    shape/<key>        its shape
                    x_digest           sha256 of the input swin_inputs makes (image, or the layer's tokens)
                    out<i>, mask<i>, pos<i>   Joiner's eval-mode features, their masks and position encodings
                    grad_x             gradient of swin_inputs.weighted_sum(outputs, seed + 7) w.r.t. the image
                    out0/..., grad_x/...   the layer case's output and input gradient (swin_inputs.store_tokens)
                    <param>/grad/ or <param>/gradsum0/, <param>/gradsum1/   the parameters' gradients (large ones as sums)

As gen_golden_r10.py does, the definitions are taken out of their files with `ast` and executed unchanged (importing the files
needs timm and util.misc).  timm is replaced by stand-ins: to_2tuple, trunc_normal_ = torch.nn.init.trunc_normal_ (the same
algorithm) and a DropPath that the fixtures never exercise (eval mode, drop_path_rate 0).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r12.py
"""
import ast
import math
import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint
from torch import Tensor, nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import swin_inputs as SI   # noqa: E402


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


class DropPath(nn.Module):
    """Stand-in for timm's DropPath (never active in these fixtures)."""

    def __init__(self, drop_prob=0.):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        assert self.drop_prob == 0 or not self.training
        return x


def to_2tuple(x):
    return tuple(x) if isinstance(x, (list, tuple)) else (x, x)


def _record(z, model, outs, seed):
    SI.weighted_sum(outs, seed + 7).backward()
    for k, p in model.named_parameters():
        if p.grad is not None:
            SI.store_grad(z, k + "/", p.grad)


def main():
    (NestedTensor,) = _extract(REF + "/util/misc.py", ["NestedTensor"], {"Optional": Optional, "Tensor": Tensor})
    ns = {"torch": torch, "nn": nn, "F": F, "np": np, "checkpoint": checkpoint, "DropPath": DropPath, "to_2tuple": to_2tuple,
          "trunc_normal_": nn.init.trunc_normal_, "NestedTensor": NestedTensor, "math": math, "List": List, "Dict": Dict}
    names = ["Mlp", "window_partition", "window_reverse", "WindowAttention", "SwinTransformerBlock", "PatchMerging",
             "BasicLayer", "PatchEmbed", "SwinTransformer"]
    got = dict(zip(names, _extract(REF + "/models/swin_transformer.py", names, ns)))
    (PosSine,) = _extract(REF + "/models/position_encoding.py", ["PositionEmbeddingSine"], ns)
    (Joiner,) = _extract(REF + "/models/backbone.py", ["Joiner"], ns)
    torch.use_deterministic_algorithms(True)

    for name, c in SI.BACKBONE_CASES.items():
        m = SI.build_backbone(got["SwinTransformer"], Joiner, PosSine, name)
        z = {}
        for k, v in m.state_dict().items():
            z["init/" + k] = np.array(SI.digest(v))
            z["shape/" + k] = np.array(v.shape, dtype=np.int64)
        img, mask = SI.backbone_input(name)
        x = img.clone().requires_grad_(True)
        feats, pos = m(NestedTensor(x, mask))
        z["x_digest"] = np.array(SI.digest(img))
        for i, (f, p) in enumerate(zip(feats, pos)):
            z["out%d" % i] = f.tensors.detach().numpy().copy()
            z["mask%d" % i] = f.mask.numpy().copy()
            z["pos%d" % i] = p.numpy().copy()
        _record(z, m, [f.tensors for f in feats], c["seed"])
        z["grad_x"] = x.grad.numpy().copy()
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)

    for name, c in SI.LAYER_CASES.items():
        m = SI.build_layer(got["BasicLayer"], name)
        z = {}
        for k, v in m.state_dict().items():
            z["init/" + k] = np.array(SI.digest(v))
            z["shape/" + k] = np.array(v.shape, dtype=np.int64)
        x0 = SI.layer_input(name)
        x = x0.clone().requires_grad_(True)
        y = m(x, c["H"], c["W"])[0]
        z["x_digest"] = np.array(SI.digest(x0))
        _record(z, m, [y], c["seed"])
        SI.store_tokens(z, "out0", y)
        SI.store_tokens(z, "grad_x", x.grad)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **z)


if __name__ == "__main__":
    main()
