#!/usr/bin/env python3
"""SmoothNet fixtures, made by RUNNING THE REFERENCE'S SmootherResBlock / Smoother / MotionSmoother / ArcticSmoother
(models/smoothnet.py) and get_arctic_item (arctic_tools/process.py) on the CPU, over the seeded inputs of smoother_inputs.py:

  smoother_small.npz   <case>/init/<key>   sha256 of each state_dict entry as constructed under the case's seed
                       <case>/x, <case>/out, <case>/grad_x, <case>/grad/<param>
                                           eval-mode output and the gradients of smoother_inputs.weighted_sum(out, seed)
  smoother_arctic.npz  init/<key>, shape/<key>   sha256 and shape of each state_dict entry (default sizes, T 32, B 1)
                       x<i>, out<i>, grad_x<i>   the nine inputs, eval-mode outputs and input gradients
  arctic_item.npz      <case>/in/<name>, <case>/out<i>   selection inputs and the nine outputs

As gen_golden_r09.py does, the definitions are taken out of their files with `ast` and executed unchanged (importing the files
needs smplx).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r11.py
"""
import ast
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import smoother_inputs as SI   # noqa: E402


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def main():
    ns = {"torch": torch, "nn": nn}
    _, _, Motion, Arctic = _extract(REF + "/models/smoothnet.py",
                                    ["SmootherResBlock", "Smoother", "MotionSmoother", "ArcticSmoother"], ns)
    (get_item,) = _extract(REF + "/arctic_tools/process.py", ["get_arctic_item"], {"torch": torch})
    torch.use_deterministic_algorithms(True)

    out = {}
    for name in SI.SMALL_CASES:
        m = SI.build_motion(Motion, name)
        for k, v in m.state_dict().items():
            out["%s/init/%s" % (name, k)] = np.array(SI.digest(v))
        x = SI.motion_input(name).requires_grad_(True)
        y = m(x)
        SI.weighted_sum([y], 7).backward()
        out[name + "/x"] = x.detach().numpy()
        out[name + "/out"] = y.detach().contiguous().numpy()
        out[name + "/grad_x"] = x.grad.numpy()
        for k, p in m.named_parameters():
            out["%s/grad/%s" % (name, k)] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "smoother_small.npz"), **out)

    out = {}
    a = SI.build_arctic(Arctic)
    for k, v in a.state_dict().items():
        out["init/" + k] = np.array(SI.digest(v))
        out["shape/" + k] = np.array(v.shape, dtype=np.int64)
    xs = [t.requires_grad_(True) for t in SI.arctic_inputs()]
    ys = SI.flatten(a(SI.structure(xs)))
    SI.weighted_sum(ys, 8).backward()
    for i, (x, y) in enumerate(zip(xs, ys)):
        out["x%d" % i] = x.detach().numpy()
        out["out%d" % i] = y.detach().contiguous().numpy()
        out["grad_x%d" % i] = x.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "smoother_arctic.npz"), **out)

    out = {}
    for case in SI.ITEM_CASES:
        o = SI.item_outputs(case)
        out[case + "/in/pred_logits"] = o["pred_logits"].numpy()
        for key in ("pred_cams", "pred_mano_params", "pred_obj_params"):
            for j, t in enumerate(o[key]):
                out["%s/in/%s%d" % (case, key, j)] = t.numpy()
        res = SI.flatten(get_item(o, SI.Cfg(), device="cpu"))
        for i, t in enumerate(res):
            out["%s/out%d" % (case, i)] = t.numpy()
    np.savez_compressed(os.path.join(HERE, "arctic_item.npz"), **out)


if __name__ == "__main__":
    main()
