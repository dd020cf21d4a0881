#!/usr/bin/env python3
"""DeformableDETR fixtures, made by RUNNING THE REFERENCE'S DeformableDETR (models/actic_detr.py, models/assembly_detr.py) with
its MLP, _get_clones and inverse_sigmoid (util/misc.py) on the CPU, over the stub transformer / backbones of detr_inputs.py:

  detr_<case>.npz   init/<key>   sha256 of the bytes of each state_dict entry as constructed under seed 0, and its shape
                                 as shape/<key> (the keys are the reference's)
                    out/<path>   every output of forward (train mode) with the seeded parameters of detr_inputs.perturb,
                                 in detr_inputs.flatten_outputs order
                    grad/hs, grad/<param>   gradients of detr_inputs.weighted_sum(out, seed) (None gradients absent);
                                 gradients over GRAD_FULL elements are kept as their sums over dim 0 and dim 1
                                 (gradsum0/<param>, gradsum1/<param>) to keep the files small

As gen_golden_r08.py does, the definitions are taken out of their files with `ast` and executed unchanged; NestedTensor is the
package's container (the reference's util/misc.py one holds the same two fields).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r10.py
"""
import ast
import copy
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import detr_inputs as DI   # noqa: E402
from uvhand_amd.modules.detr import NestedTensor, nested_tensor_from_tensor_list  # noqa: E402


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def reference_models():
    out = {}
    for key, path in (("arctic", "/models/actic_detr.py"), ("assembly", "/models/assembly_detr.py")):
        ns = {"torch": torch, "nn": nn, "F": F, "copy": copy, "math": math, "np": np, "NestedTensor": NestedTensor,
              "nested_tensor_from_tensor_list": nested_tensor_from_tensor_list}
        _extract(REF + "/util/misc.py", ["inverse_sigmoid"], ns)
        (out[key],) = _extract(REF + path, ["_get_clones", "MLP", "DeformableDETR"], ns)[2:]
    return out


GRAD_FULL = 16384


def run(name, model_cls):
    model = DI.build(name, model_cls, NestedTensor)
    z = {}
    for k, v in model.state_dict().items():
        z["init/" + k] = np.array(DI.digest(v))
        z["shape/" + k] = np.array(v.shape, dtype=np.int64)
    DI.perturb(model, DI.CASES[name][-1])
    model.train()
    out = model(DI.samples(name, NestedTensor))
    for path, t in DI.flatten_outputs(out):
        z["out" + path] = t.detach().numpy().copy()
    DI.weighted_sum(out, DI.CASES[name][-1] + 7).backward()
    z["grad/hs"] = model.transformer.hs.grad.numpy().copy()
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        if p.grad.numel() > GRAD_FULL:
            z["gradsum0/" + k] = p.grad.sum(0).numpy().copy()
            z["gradsum1/" + k] = p.grad.sum(1).numpy().copy()
        else:
            z["grad/" + k] = p.grad.numpy().copy()
    return z


def main():
    refs = reference_models()
    for name, case in DI.CASES.items():
        z = run(name, refs[case[0]])
        np.savez_compressed(os.path.join(HERE, "detr_%s.npz" % name), **z)
        print(name, len(z), "arrays")


if __name__ == "__main__":
    main()
