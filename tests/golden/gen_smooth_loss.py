#!/usr/bin/env python3
"""SmoothNet-criterion fixtures, made by RUNNING THE REFERENCE'S OWN FUNCTIONS unchanged on the seeded inputs of
smooth_loss_inputs.py: compute_smoothnet_loss (arctic_tools/src/callbacks/loss/loss_arctic_sf.py), eval_acc_pose and
compute_error_accel (src/utils/eval_modules.py), compute_contact_devi_loss and contact_deviation (src/utils/loss_modules.py),
nanmean (common/torch_utils.py); common/xdict.py over common/thing.py carries eval_acc_pose's result.

  smooth_loss.npz  <case>/keys            compute_smoothnet_loss's keys in its order
                   <case>/loss/<key>      its three values (fp64 copies); <case>/dtype/<key> the dtype the reference returned
                   <case>/eval/<key>      eval_acc_pose's two arrays
                   <case>/raises          for N < 3: the exception eval_acc_pose ends in (its mask and its rows differ in
                                          length); the loss then holds loss/cd alone, from compute_contact_devi_loss
                   <case>/insum/<pred|gt>/<key>  fp64 (sum, sum of |.|) of the ten vertex and joint tensors the run read: a test
                                          that rebuilds bitwise the same inputs can hold the fixture to a tight bound
                   <case>/grad/<key>      d (10 loss/cd) / d pred[key], the first grad_rows(N) rows of every frame (file size: at
                                          most 3000 elements), and <case>/gradsum/<key> the fp64 sum of |.| over the whole tensor

As gen_arctic_eval.py does, the definitions are taken out of their files with `ast` and executed unchanged (importing them
needs pytorch3d).  Stand-ins, none of them arithmetic of the result: device='cpu' and a no-op Tensor.cuda while the reference
runs; compute_smoothnet_loss's four axis_angle_to_matrix calls (pytorch3d's; their results are never read) are served by
common/rot.py's copies.  The generator asserts in fp64 what the tests rely on: every case has at least one bottom row in
parts_ids[0], and the coherent case's per-frame acceleration errors lie in smooth_loss_inputs.ACC_RANGE.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_smooth_loss.py
"""
import ast
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference") + "/arctic_tools"

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import smooth_loss_inputs as MI  # noqa: E402


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _reference():
    S = types.SimpleNamespace
    rot_names = ["axis_angle_to_quaternion", "quaternion_to_matrix"]
    aa2q, q2m = _extract(REF + "/common/rot.py", rot_names, {"torch": torch, "F": F})
    thing_names = ["thing2dev", "thing2np", "thing2torch", "thing2list", "detach_thing"]
    thing = S(**dict(zip(thing_names, _extract(REF + "/common/thing.py", thing_names, {"torch": torch, "np": np}))))
    (xdict,) = _extract(REF + "/common/xdict.py", ["xdict"], {"torch": torch, "np": np, "thing": thing})
    (nanmean,) = _extract(REF + "/common/torch_utils.py", ["nanmean"], {"torch": torch})
    torch_utils = S(nanmean=nanmean)
    cdl, cd = _extract(REF + "/src/utils/loss_modules.py", ["compute_contact_devi_loss", "contact_deviation"],
                       {"torch": torch, "np": np, "nanmean": nanmean, "torch_utils": torch_utils})
    cea, eap = _extract(REF + "/src/utils/eval_modules.py", ["compute_error_accel", "eval_acc_pose"],
                        {"torch": torch, "np": np, "torch_utils": torch_utils, "xdict": xdict})
    (csl,) = _extract(REF + "/src/callbacks/loss/loss_arctic_sf.py", ["compute_smoothnet_loss"],
                      {"torch": torch, "np": np, "torch_utils": torch_utils, "axis_angle_to_matrix": lambda a: q2m(aa2q(a)),
                       "compute_contact_devi_loss": cdl, "eval_acc_pose": eap})
    return S(compute_smoothnet_loss=csl, eval_acc_pose=eap, compute_error_accel=cea, compute_contact_devi_loss=cdl,
             contact_deviation=cd, nanmean=nanmean, xdict=xdict)


class _NoCuda:
    """While the reference runs: Tensor.cuda() returns the tensor."""

    def __enter__(self):
        self.saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda t, *a, **k: t

    def __exit__(self, *exc):
        torch.Tensor.cuda = self.saved
        return False


def _check_inputs(case, pred, gt, ref):
    assert (gt["object.parts_ids"][0] == 2).any(), "no bottom row in parts_ids[0]"
    assert pred["object.v.cam"].shape == gt["object.v.cam"].shape
    if case != "coherent":
        return
    d = lambda t: t.double()  # noqa: E731
    bottom = gt["object.parts_ids"][0] == 2
    rows = []
    for k, rp, rg in (("mano.v3d.cam.r", d(pred["mano.j3d.cam.r"])[:, :1], d(gt["mano.j3d.cam.r"])[:, :1]),
                      ("mano.v3d.cam.l", d(pred["mano.j3d.cam.l"])[:, :1], d(gt["mano.j3d.cam.l"])[:, :1]),
                      ("object.v.cam", d(pred["object.v.cam"])[:, bottom].mean(dim=1)[:, None], d(gt["object.v.cam"])[:, bottom].mean(dim=1)[:, None])):
        rows.append(ref.compute_error_accel(d(gt[k]) - rg, d(pred[k]) - rp))
    acc = torch.cat(rows)
    print("coherent: per-frame acceleration errors %.2f .. %.2f m/s^2" % (float(acc.min()), float(acc.max())))
    assert float(acc.min()) >= MI.ACC_RANGE[0] and float(acc.max()) <= MI.ACC_RANGE[1]


def main():
    warnings.filterwarnings("ignore")
    ref = _reference()
    out = {}
    m = MI.models()
    for case in MI.CASES:
        pred, gt = MI.case_inputs(case, m)
        _check_inputs(case, pred, gt, ref)
        p, ls = MI.leaves(pred)
        p, g = ref.xdict(p), ref.xdict(gt)
        with _NoCuda():
            try:
                losses = ref.compute_smoothnet_loss(p, g, None, None, 224, device="cpu")
                ev = ref.eval_acc_pose(p, g, None)
            except (IndexError, RuntimeError, ValueError) as exc:
                assert gt["is_valid"].shape[0] < 3, (case, exc)
                out[case + "/raises"] = np.array(type(exc).__name__)
                cd_ro, cd_lo = ref.compute_contact_devi_loss(p, g)
                losses, ev = {"loss/cd": torch.tensor(0).to(torch.float32) + cd_ro + cd_lo}, {}
        for side, d in (("pred", pred), ("gt", gt)):
            for k in MI.PRED_LEAVES:
                out["%s/insum/%s/%s" % (case, side, k)] = MI.checksum(d[k])
        out[case + "/keys"] = np.array(list(losses.keys()))
        for k, v in losses.items():
            out["%s/loss/%s" % (case, k)] = np.float64(v.detach().double().item())
            out["%s/dtype/%s" % (case, k)] = np.array(str(v.dtype))
        for k, v in dict(ev).items():
            out["%s/eval/%s" % (case, k)] = np.asarray(v)
        (10 * losses["loss/cd"]).backward()
        for k, t in zip(MI.PRED_LEAVES, ls):
            grad = torch.zeros_like(t) if t.grad is None else t.grad
            out["%s/grad/%s" % (case, k)] = grad[:, :MI.grad_rows(grad.shape[0])].numpy()
            out["%s/gradsum/%s" % (case, k)] = np.float64(grad.double().abs().sum().item())
        print(case, {k: float(out["%s/loss/%s" % (case, k)]) for k in losses}, str(out.get(case + "/raises", "")))
    np.savez_compressed(os.path.join(HERE, "smooth_loss.npz"), **out)
    print("smooth_loss.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "smooth_loss.npz")))


if __name__ == "__main__":
    main()
