#!/usr/bin/env python3
"""ARCTIC small-loss fixtures, made by RUNNING THE REFERENCE'S compute_small_loss (src/callbacks/loss/loss_arctic_sf.py) and
ObjectTensors.forward_7d_batch (common/object_tensors.py) unchanged on the synthetic objects and seeded inputs of
small_loss_inputs.py:

  small_loss.npz   <case>/pred/<name>       the nine get_arctic_item inputs (small_loss_inputs.PRED_NAMES)
                   <case>/gt/<key>, <case>/K, <case>/obj_idx
                   <case>/loss/<key>         the 19 terms, in the reference's key order (<case>/keys)
                   <case>/grad/<name>        gradients of sum_k w_k * loss_k (w: small_loss_inputs.upstream) w.r.t. the inputs
                   object/<key>              forward_7d_batch of case all_valid (v, v_sub, bbox3d, kp3d, ...)

As gen_golden_r11.py / gen_golden_r13.py do, the definitions are taken out of their files with `ast` and executed unchanged
(importing them needs pytorch3d, trimesh and the ARCTIC meta files).  ObjectTensors is built without __init__ with the synthetic
obj_tensors installed; axis_angle_to_matrix is pytorch3d's, quaternion_to_matrix . axis_angle_to_quaternion of common/rot.py.
The MANO calls are served by the package's mano_reference (pinned to manopth by test_mano.py) on mano_inputs.py's models.
compute_small_loss casts to fp32 and project2d_batch asserts on fp32, so the reference runs in fp32 on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r14.py
"""
import ast
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference") + "/arctic_tools"

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mano_inputs as MI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd.mano import MANO  # noqa: E402


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


class _XDict(dict):
    """common/xdict.py's overwrite is plain dict assignment."""

    def overwrite(self, k, v):
        super().__setitem__(k, v)


def _reference():
    rot_ns = {"torch": torch}
    q2m, aa2q, qmul, qinv, qapply = _extract(REF + "/common/rot.py", ["quaternion_to_matrix", "axis_angle_to_quaternion",
                                                                     "quaternion_raw_multiply", "quaternion_invert",
                                                                     "quaternion_apply"], rot_ns)
    (nanmean,) = _extract(REF + "/common/torch_utils.py", ["nanmean"], {"torch": torch})
    torch_utils = types.SimpleNamespace(nanmean=nanmean)
    (wp2p,) = _extract(REF + "/common/camera.py", ["weak_perspective_to_perspective_torch"], {"torch": torch})
    tf_ns = {"torch": torch}
    to_xy, project2d = _extract(REF + "/common/transforms.py", ["to_xy_batch", "project2d_batch"], tf_ns)
    (normalize_kp2d,) = _extract(REF + "/common/data_utils.py", ["normalize_kp2d"], {"torch": torch})
    lm_ns = {"torch": torch, "np": np, "nn": nn, "nanmean": nanmean, "torch_utils": torch_utils,
             "l1_loss": nn.L1Loss(reduction="none"), "mse_loss": nn.MSELoss(reduction="none")}
    names = ["compute_contact_devi_loss", "contact_deviation", "subtract_root_batch", "keypoint_3d_loss", "object_kp3d_loss",
             "hand_kp3d_loss", "vector_loss", "joints_loss", "mano_loss", "obj_smt_loss"]
    lm = dict(zip(names, _extract(REF + "/src/utils/loss_modules.py", names, lm_ns)))
    ns = dict(lm, torch=torch, np=np, nn=nn, l1_loss=lm_ns["l1_loss"], mse_loss=lm_ns["mse_loss"],
              camera=types.SimpleNamespace(weak_perspective_to_perspective_torch=wp2p),
              tf=types.SimpleNamespace(project2d_batch=project2d, to_xy_batch=to_xy),
              data_utils=types.SimpleNamespace(normalize_kp2d=normalize_kp2d), torch_utils=torch_utils,
              axis_angle_to_matrix=lambda a: q2m(aa2q(a)))
    (compute_small_loss,) = _extract(REF + "/src/callbacks/loss/loss_arctic_sf.py", ["compute_small_loss"], ns)
    ot_ns = {"torch": torch, "np": np, "nn": nn, "xdict": _XDict, "axis_angle_to_quaternion": aa2q, "quaternion_apply": qapply}
    (ObjectTensors,) = _extract(REF + "/common/object_tensors.py", ["ObjectTensors"], ot_ns)
    return compute_small_loss, ObjectTensors


def models(ObjectTensors):
    obj = ObjectTensors.__new__(ObjectTensors)
    nn.Module.__init__(obj)
    obj.obj_tensors = SI.obj_arrays()
    obj.dev = None
    mano_l = MANO.from_arrays(**MI.model_arrays("left", dtype=torch.float32), is_rhand=False)
    mano_r = MANO.from_arrays(**MI.model_arrays("right", dtype=torch.float32))
    return {"mano_l": mano_l, "mano_r": mano_r, "arti_head": obj}


def main():
    compute_small_loss, ObjectTensors = _reference()
    m = models(ObjectTensors)
    out = {}
    for case, seed in SI.CASES.items():
        pred, gt, meta = SI.case_inputs(case)
        leaves = [t.clone().requires_grad_(True) for t in SI.flat_pred(pred)]
        d = compute_small_loss(SI.unflat_pred(leaves), gt, meta, m, SI.IMG_RES, device="cpu")
        keys = list(d.keys())
        w = SI.upstream(seed + 100)
        total = sum(w[i] * d[k].sum() for i, k in enumerate(keys))
        total.backward()
        out[case + "/keys"] = np.array(keys)
        for name, t, leaf in zip(SI.PRED_NAMES, SI.flat_pred(pred), leaves):
            out["%s/pred/%s" % (case, name)] = t.numpy()
            g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            out["%s/grad/%s" % (case, name)] = g.numpy()
        for k, v in gt.items():
            out["%s/gt/%s" % (case, k)] = v.numpy()
        out[case + "/K"] = meta["intrinsics"].numpy()
        out[case + "/obj_idx"] = np.array([SI.OBJECTS.index(n) for n in meta["query_names"]])
        for k in keys:
            out["%s/loss/%s" % (case, k)] = d[k].detach().numpy()
    pred, _, meta = SI.case_inputs("all_valid")
    o = m["arti_head"].forward(pred[3][1].view(-1, 1), pred[3][0], None, meta["query_names"])
    for k, v in o.items():
        out["object/" + k] = v.numpy()
    out["object/keys"] = np.array(list(o.keys()))
    np.savez_compressed(os.path.join(HERE, "small_loss.npz"), **out)


if __name__ == "__main__":
    main()
