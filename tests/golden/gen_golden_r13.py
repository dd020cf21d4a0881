#!/usr/bin/env python3
"""MANO fixtures, made by RUNNING THE REFERENCE'S manopth ManoLayer (manopth/manolayer.py, tensutils.py, rodrigues_layer.py:
the same linear blend skinning as smplx's lbs) in float64 on the synthetic models of mano_inputs.py:

  mano_mean.npz / mano_flat.npz   <side>/betas, <side>/global_orient, <side>/hand_pose   inputs (hand_pose without the mean)
                                  <side>/vertices [B, 778, 3], <side>/joints [B, 16, 3]    smplx conventions: metres, the 16
                                                                                           posed joints in native MANO order
                                  <side>/grad_betas, <side>/grad_global_orient, <side>/grad_hand_pose
                                      gradients of sum(vertices * w_v) + sum(joints * w_j), weights mano_inputs.upstream

As gen_golden_r11.py does, the definitions are taken out of their files with `ast` and executed unchanged (importing
manolayer.py needs mano.webuser / chumpy).  The instance is built without __init__ and the synthetic model is installed as
its th_* buffers; use_pca=False, axis-angle, center_idx=None, th_trans=None.  manopth's quaternion Rodrigues and smplx's
formula agree to rounding away from zero angles, which the inputs keep.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r13.py
"""
import ast
import os
import sys
import types

import numpy as np
import torch
from torch.nn import Module

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import mano_inputs as MI   # noqa: E402

REORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]   # manolayer.py's final permutation


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _manopth():
    rod_ns = {"torch": torch}
    quat2mat, batch_rodrigues = _extract(REF + "/manopth/rodrigues_layer.py", ["quat2mat", "batch_rodrigues"], rod_ns)
    rodrigues_layer = types.SimpleNamespace(batch_rodrigues=batch_rodrigues, quat2mat=quat2mat)
    tu_ns = {"torch": torch, "rodrigues_layer": rodrigues_layer}
    tu = _extract(REF + "/manopth/tensutils.py", ["th_posemap_axisang", "th_with_zeros", "th_pack", "subtract_flat_id",
                                                  "make_list"], tu_ns)
    ns = {"torch": torch, "np": np, "os": os, "Module": Module, "rodrigues_layer": rodrigues_layer,
          "th_posemap_axisang": tu[0], "th_with_zeros": tu[1], "th_pack": tu[2], "subtract_flat_id": tu[3], "make_list": tu[4]}
    (ManoLayer,) = _extract(REF + "/manopth/manolayer.py", ["ManoLayer"], ns)
    return ManoLayer


def _layer(ManoLayer, side, flat):
    m = MI.model_arrays(side, flat)
    lay = ManoLayer.__new__(ManoLayer)
    Module.__init__(lay)
    lay.center_idx, lay.use_pca, lay.rot, lay.ncomps, lay.side = None, False, 3, 45, side
    lay.joint_rot_mode, lay.root_rot_mode, lay.robust_rot, lay.flat_hand_mean = "axisang", "axisang", False, flat
    lay.register_buffer("th_betas", torch.zeros(1, MI.NB, dtype=torch.float64))
    lay.register_buffer("th_shapedirs", m["shapedirs"])
    lay.register_buffer("th_posedirs", m["posedirs"].t().reshape(MI.V, 3, MI.NPF).contiguous())
    lay.register_buffer("th_v_template", m["v_template"].unsqueeze(0))
    lay.register_buffer("th_J_regressor", m["J_regressor"])
    lay.register_buffer("th_weights", m["lbs_weights"])
    lay.register_buffer("th_faces", m["faces"].int())
    lay.register_buffer("th_hands_mean", m["pose_mean"][3:].unsqueeze(0))
    lay.kintree_parents = list(MI.PARENTS)
    return lay


def main():
    ManoLayer = _manopth()
    native = [REORDER.index(i) for i in range(MI.NJ)]       # position of native joint i after the permutation
    for flat, name in ((False, "mano_mean"), (True, "mano_flat")):
        out = {}
        for case, (side, f, seed) in MI.FIXTURE_CASES.items():
            if f != flat:
                continue
            lay = _layer(ManoLayer, side, flat)
            betas, go, hp = MI.pose_inputs(seed, MI.FIXTURE_B, mean=None if flat else MI.hand_mean(side))
            leaves = [t.clone().requires_grad_(True) for t in (betas, go, hp)]
            verts, jtr = lay(torch.cat([leaves[1], leaves[2]], 1), th_betas=leaves[0], th_trans=None)
            verts, joints = verts / 1000, jtr[:, native] / 1000
            wv, wj = MI.upstream(seed + 100, MI.FIXTURE_B)
            ((verts * wv).sum() + (joints * wj).sum()).backward()
            for key, t in (("betas", betas), ("global_orient", go), ("hand_pose", hp), ("vertices", verts), ("joints", joints)):
                out["%s/%s" % (side, key)] = t.detach().numpy()
            for key, t in zip(("grad_betas", "grad_global_orient", "grad_hand_pose"), leaves):
                out["%s/%s" % (side, key)] = t.grad.numpy()
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)


if __name__ == "__main__":
    main()
