#!/usr/bin/env python3
"""DINO decoder fixture, made by RUNNING THE REFERENCE'S TransformerDecoder and DeformableTransformerDecoderLayer
(models/dino/deformable_transformer.py:627-827, :886-1058) with its MLP and gen_sineembed_for_position (models/dino/utils.py) and
inverse_sigmoid (util/misc.py) unchanged, on the seeded parameters and inputs of dino_inputs.py:

  dino_decoder.npz   <case>/hs<i>              the normed output of layer i [N, L, 256]
                     <case>/ref<i>             the n_layers + 1 reference points [N, L, width]
                     <case>/grad_<leaf>        gradients of sum(weight * output) over every returned tensor w.r.t. tgt, memory,
                                               refpoints_unsigmoid
                     <case>/param_names, pgrad_none, pgrad_val, pgrad_sum, pgrad_abssum   seeded samples and fp64 sums of every
                                               parameter gradient, in sorted name order
                     <case>/state_keys         the decoder's state_dict keys, in order
                     <case>/margin             per layer the smallest gap between a row's top two class logits

As gen_golden_r14.py and the AssemblyHands generator do, the definitions are taken out of their files with `ast` and executed
unchanged (importing the files needs the reference's CUDA extension).  The package's MSDeformAttn serves the cross-attention.
CPU, fp32, eval mode.  The generator asserts the fixture's condition: in every layer every row's top two class logits differ
by at least dino_inputs.MIN_MARGIN (a rounding difference cannot flip an argmax) and all three codes (stay / object / hand) occur.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dino_decoder.py
"""
import ast
import copy
import math
import os
import random
import sys
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dino_inputs as DI  # noqa: E402
import uvhand_amd.modules.ms_deform_attn as msda_mod  # noqa: E402
from uvhand_amd.modules import MSDeformAttn  # noqa: E402


class _CpuCore:
    """MSDeformAttnFunction's interface on the oracle's pure-PyTorch core (the library's op refuses CPU tensors)."""

    @staticmethod
    def apply(value, shapes, lsi, loc, attn, im2col_step):
        from oracle.torch_fallback import msda_torch_fallback
        return msda_torch_fallback(value, shapes, loc, attn)


msda_mod.MSDeformAttnFunction = _CpuCore


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _reference():
    (inverse_sigmoid,) = _extract(REF + "/util/misc.py", ["inverse_sigmoid"], {"torch": torch})
    uns = {"torch": torch, "nn": nn, "F": F, "math": math}
    MLP, act, sine = _extract(REF + "/models/dino/utils.py", ["MLP", "_get_activation_fn", "gen_sineembed_for_position"], uns)
    ns = {"torch": torch, "nn": nn, "Tensor": Tensor, "Optional": Optional, "math": math, "random": random, "copy": copy,
          "inverse_sigmoid": inverse_sigmoid, "MLP": MLP, "_get_activation_fn": act, "gen_sineembed_for_position": sine,
          "MSDeformAttn": MSDeformAttn}
    dec, layer, _ = _extract(REF + "/models/dino/deformable_transformer.py",
                             ["TransformerDecoder", "DeformableTransformerDecoderLayer", "_get_clones"], ns)
    return layer, dec


def main():
    layer_cls, dec_cls = _reference()
    out = {}
    for case in DI.CASES:
        dec = DI.build(layer_cls, dec_cls, case)
        logits = []
        hooks = [m.register_forward_hook(lambda mod, inp, o: logits.append(o.detach().double())) for m in dec.class_embed]
        outs, leaves = DI.run(dec, case)
        for h in hooks:
            h.remove()
        margins = []
        for lid, c in enumerate(logits):
            top = torch.topk(c, 2, dim=-1)[0]
            margins.append(float((top[..., 0] - top[..., 1]).min()))
            cl = c.argmax(-1)
            hand = (cl == 12) | (cl == 13)
            codes = set((2 * hand.long() + (~hand & (cl != 0)).long()).flatten().tolist())
            assert codes == {0, 1, 2}, "%s layer %d: codes %s; change the seed" % (case, lid, sorted(codes))
            assert margins[-1] >= DI.MIN_MARGIN, "%s layer %d: class margin %.3e; change the seed" % (case, lid, margins[-1])
        out[case + "/margin"] = np.asarray(margins)
        for lab, o in zip(DI.labels(), outs):
            out["%s/%s" % (case, lab)] = o.detach().numpy()
        for k, leaf in leaves.items():
            out["%s/grad_%s" % (case, k)] = leaf.grad.numpy()
        params = sorted(dec.named_parameters(), key=lambda kv: kv[0])
        out[case + "/param_names"] = np.array([k for k, _ in params])
        out[case + "/state_keys"] = np.array(list(dec.state_dict().keys()))
        none, val, sums, abss = [], np.zeros((len(params), DI.PGRAD_SAMPLES), dtype=np.float32), [], []
        for j, (k, p) in enumerate(params):
            none.append(p.grad is None)
            g = (p.grad if p.grad is not None else torch.zeros_like(p)).flatten().double().numpy()
            idx = DI.pgrad_index(case, j, g.size)
            val[j, :idx.size] = g[idx]
            sums.append(g.sum())
            abss.append(np.abs(g).sum())
        out[case + "/pgrad_none"] = np.asarray(none)
        out[case + "/pgrad_val"] = val
        out[case + "/pgrad_sum"] = np.asarray(sums, dtype=np.float64)
        out[case + "/pgrad_abssum"] = np.asarray(abss, dtype=np.float64)
        print(case, "margins", margins)
    np.savez_compressed(os.path.join(HERE, "dino_decoder.npz"), **out)


if __name__ == "__main__":
    main()
