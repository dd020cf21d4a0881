#!/usr/bin/env python3
"""DINO model fixture, made by RUNNING THE REFERENCE'S DINO class (models/dino/dino.py:46-426) unchanged, with its MLP
(models/dino/utils.py), inverse_sigmoid (util/misc.py), prepare_for_cdn and dn_post_process (models/dino/dn_components.py), on the
stub backbone, seeded parameters, images and targets of dino_model_inputs.py.  The transformer is the package's
DinoDeformableTransformer (its own fixture: gen_dino_transformer.py).

  dino_model.npz   <case>/state_keys      the state_dict keys of the bare construction, in order
                   <case>/init_sums       per-tensor fp64 sums of the state_dict constructed under torch.manual_seed(INIT_SEED)
                   <case>/key_order       the output dict's keys, nested ones too, in order
                   <case>/output_names, out<j>   every tensor of the output dict (dn_meta's denoising part included)
                   <case>/grad_image, grad_src<l>   gradients of the seeded weighted sum w.r.t. the images and the projected levels
                   <case>/param_names, pgrad_none, pgrad_val, pgrad_sum, pgrad_abssum   seeded samples and fp64 sums of every
                                          parameter gradient, in sorted name order

As gen_dino_transformer.py does, the definitions are taken out of their files with `ast` and executed unchanged (importing the
files needs the reference's CUDA extension).  The package's MSDeformAttn serves the sampling on the oracle's pure-PyTorch core.
CPU, fp32; the training cases have label noise 0 and dropout 0, so nothing random reaches an output.  In this process only,
Tensor.cuda is the identity and .to('cuda') goes to the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dino_model.py
"""
import ast
import copy
import math
import os
import sys
from typing import List

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dino_model_inputs as MI  # noqa: E402
import uvhand_amd.modules.ms_deform_attn as msda_mod  # noqa: E402
from uvhand_amd.modules import DinoDeformableTransformer  # noqa: E402


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


def _cpu_only():
    """This process has no GPU: .cuda() is the identity and 'cuda' means the CPU."""
    real_to = torch.Tensor.to

    def to(self, *args, **kwargs):
        args = tuple("cpu" if a == "cuda" else a for a in args)
        if kwargs.get("device") == "cuda":
            kwargs["device"] = "cpu"
        return real_to(self, *args, **kwargs)

    torch.Tensor.to = to
    torch.Tensor.cuda = lambda self, *a, **k: self


def _reference():
    (inverse_sigmoid,) = _extract(REF + "/util/misc.py", ["inverse_sigmoid"], {"torch": torch})
    (MLP,) = _extract(REF + "/models/dino/utils.py", ["MLP"], {"torch": torch, "nn": nn, "F": F})
    prepare_for_cdn, dn_post_process = _extract(REF + "/models/dino/dn_components.py", ["prepare_for_cdn", "dn_post_process"],
                                                {"torch": torch, "inverse_sigmoid": inverse_sigmoid})
    ns = {"torch": torch, "nn": nn, "F": F, "math": math, "copy": copy, "List": List, "NestedTensor": MI.NestedTensor,
          "inverse_sigmoid": inverse_sigmoid, "MLP": MLP, "prepare_for_cdn": prepare_for_cdn, "dn_post_process": dn_post_process}
    (dino,) = _extract(REF + "/models/dino/dino.py", ["DINO"], ns)
    return dino


def run_case(case, dino_cls):
    out = {}
    torch.manual_seed(MI.INIT_SEED)
    bare = MI.construct(dino_cls, DinoDeformableTransformer, case)
    out[case + "/state_keys"] = np.array(list(bare.state_dict().keys()))
    out[case + "/init_sums"] = np.asarray([float(v.double().sum()) for v in bare.state_dict().values()], dtype=np.float64)

    model = MI.build(dino_cls, DinoDeformableTransformer, case)
    prep = MI.prepare(case)
    res, flat, srcs = MI.step(model, prep)
    out[case + "/key_order"] = np.array(MI.key_order(res))
    out[case + "/output_names"] = np.array([k for k, _ in flat])
    for j, (_, o) in enumerate(flat):
        out["%s/out%d" % (case, j)] = o.detach().numpy()
    out[case + "/grad_image"] = prep["samples"].tensors.grad.numpy()
    assert len(srcs) == MI.CFG["levels"]
    for lvl, s in enumerate(srcs):
        out["%s/grad_src%d" % (case, lvl)] = s.grad.numpy()
    params = sorted(model.named_parameters(), key=lambda kv: kv[0])
    out[case + "/param_names"] = np.array([k for k, _ in params])
    none, val, sums, abss = [], np.zeros((len(params), MI.PGRAD_SAMPLES), dtype=np.float32), [], []
    for j, (k, p) in enumerate(params):
        none.append(p.grad is None)
        g = (p.grad if p.grad is not None else torch.zeros_like(p)).flatten().double().numpy()
        ix = MI.pgrad_index(case, j, g.size)
        val[j, :ix.size] = g[ix]
        sums.append(g.sum())
        abss.append(np.abs(g).sum())
    out[case + "/pgrad_none"] = np.asarray(none)
    out[case + "/pgrad_val"] = val
    out[case + "/pgrad_sum"] = np.asarray(sums, dtype=np.float64)
    out[case + "/pgrad_abssum"] = np.asarray(abss, dtype=np.float64)
    if MI.CASES[case]["train"]:
        assert res["dn_meta"]["pad_size"] > 0 and "output_known_lbs_bboxes" in res["dn_meta"], case
    print(case, len(flat), "output tensors;", "None gradients:", [k for (k, _), n in zip(params, none) if n])
    return out


def main():
    _cpu_only()
    dino_cls = _reference()
    out = {}
    for case in MI.CASES:
        out.update(run_case(case, dino_cls))
    path = os.path.join(HERE, "dino_model.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
