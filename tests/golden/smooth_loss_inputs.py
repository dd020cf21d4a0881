"""Seeded inputs of the SmoothNet-criterion fixtures (gen_smooth_loss.py) and of tests/test_smooth_loss*.py, built on
arctic_eval_inputs.case_inputs: the targets get ``mano.v3d.cam.{r,l}`` (the MANO restatement on the gt pose and betas plus the
gt cam_t), and the prediction is the package's CPU ``make_output`` + ``prepare_data(flag='device')`` on those inputs, so ``pred``
and ``gt`` are the two halves of the dict the criterion receives.

Cases: the five of arctic_eval_inputs.CASES at N = 6; ``coherent`` (N = 8): the gt is a smooth trajectory of rigid hand and
object clouds at z = 12 m and the prediction is the gt plus small smooth per-vertex jitter, so the acceleration errors are of
realistic size (1 to 50 m/s^2; the random cases' are hundreds); ``n1``, ``n2``, ``n3``: 1, 2 and 3 frames; ``no_centre``: a
validity pattern that leaves no valid centre frame while frames still count for the contact deviation.  Shared by the generator
and the tests: nothing at test time reads the reference."""
import math

import torch

import arctic_eval_inputs as EI
import small_loss_inputs as SI
from uvhand_amd import arctic_eval as AE
from uvhand_amd.object_tensors import ObjectTensors
from uvhand_amd.small_loss import weak_perspective_to_perspective

EDGE = {"coherent": ("all_valid", 8, 2101), "n1": ("all_valid", 1, 2102), "n2": ("all_valid", 2, 2103),
        "n3": ("all_valid", 3, 2104), "no_centre": ("all_valid", 6, 2105)}
CASES = list(EI.CASES) + list(EDGE)
ACC_RANGE = (1.0, 50.0)            # m/s^2, the coherent case's per-frame errors (asserted in fp64 by the generator)
PRED_LEAVES = ("mano.v3d.cam.r", "mano.v3d.cam.l", "mano.j3d.cam.r", "mano.j3d.cam.l", "object.v.cam")


def grad_rows(n):
    """Rows per frame of a stored gradient: n x rows x 3 <= 3000 elements (file size)."""
    return min(160, 1000 // n)


def checksum(t):
    """fp64 (sum, sum of |.|) of a tensor: equal for bitwise equal tensors, and different after a one-ulp change of a
    coordinate in all but contrived cases."""
    t = t.detach().double()
    return torch.stack((t.sum(), t.abs().sum())).numpy()


def models(device="cpu", lengths=None):
    return dict(EI.mano_models(device), arti_head=ObjectTensors.from_arrays(SI.obj_arrays(lengths=lengths)).to(device))


def raw_inputs(case, B=None, lengths=None, seed=None, margin=None):
    """(outputs, targets, meta_info) of arctic_eval_inputs with the gt hand vertices added."""
    base, n, sd = EDGE.get(case, (case, SI.FIXTURE_B, None))
    outputs, gt, meta = EI.case_inputs(base, B=n if B is None else B, lengths=lengths, seed=sd if seed is None else seed,
                                       margin=margin)
    K = meta["intrinsics"]
    focal = (K[:, 0, 0] + K[:, 1, 1]) / 2.0
    manos = EI.mano_models()
    for s in ("l", "r"):
        pose = gt["mano.pose." + s]
        out = manos["mano_" + s](betas=gt["mano.beta." + s], hand_pose=pose[:, 3:], global_orient=pose[:, :3])
        cam_t = weak_perspective_to_perspective(gt["mano.cam_t.wp." + s], focal, SI.IMG_RES)
        gt["mano.v3d.cam." + s] = out.vertices.detach() + cam_t[:, None, :]
    if case == "no_centre":
        gt["is_valid"] = torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 0.0])
    return outputs, gt, meta


def _smooth(g, n, shape, amp, w0):
    """amp * sin(phase + w t) with per-element phase and frequency w in [w0, 1.5 w0]: [n, *shape]."""
    phase = 2 * math.pi * torch.rand(shape, generator=g, dtype=torch.float64)
    w = w0 * (1.0 + 0.5 * torch.rand(shape, generator=g, dtype=torch.float64))
    t = torch.arange(n, dtype=torch.float64).view(-1, *([1] * len(shape)))
    return amp * torch.sin(phase + w * t)


def _coherent(pred, gt, seed):
    """Overwrite the vertex and root tensors: rigid clouds (frame 0's) on a smooth trajectory for the gt, the gt plus smooth
    jitter of 5 mm for the prediction.  (pred - gt) has second differences of about 7 mm, times fps^2 = 900: a few m/s^2."""
    g = torch.Generator().manual_seed(seed)
    n = gt["is_valid"].shape[0]
    for k in ("mano.v3d.cam.r", "mano.v3d.cam.l", "object.v.cam"):
        cloud = gt[k][0].double()
        cloud = cloud - cloud.mean(dim=0, keepdim=True)
        centre = torch.tensor([0.1, -0.05, 12.0], dtype=torch.float64) + _smooth(g, n, (1, 3), 0.05, 0.4)
        gt.overwrite(k, (cloud[None] + centre).float())
        pred.overwrite(k, (gt[k].double() + _smooth(g, n, tuple(cloud.shape), 5e-3, 1.0)).float())
    for s in ("r", "l"):
        root = gt["mano.v3d.cam." + s][:, :1]
        k = "mano.j3d.cam." + s
        gt.overwrite(k, (root + 0.05 * torch.randn(gt[k].shape[1], 3, generator=g)).float())
        pred.overwrite(k, (gt[k].double() + _smooth(g, n, tuple(gt[k].shape[1:]), 2e-3, 1.0)).float())


def case_inputs(case, m=None, **kw):
    """(pred, gt) as XDicts of fp32 / int64 CPU tensors: the ``pred.`` and ``targets.`` halves of prepare_data's dict."""
    outputs, gt, meta = raw_inputs(case, **kw)
    with torch.no_grad():
        data = AE.prepare_data(EI.args(), outputs, gt, meta, EI.CFG, flag="device", models=models() if m is None else m)
    pred, gt = data.search("pred.", ""), data.search("targets.", "")
    pred = AE.XDict({k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in pred.items()})
    gt = AE.XDict({k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in gt.items()})
    if case == "coherent":
        _coherent(pred, gt, EDGE[case][2])
    return pred, gt


def leaves(pred, dtype=None, device=None):
    """A copy of ``pred`` whose five differentiable tensors are fresh leaves; returns (pred, [leaves])."""
    out = AE.XDict(pred)
    ls = []
    for k in PRED_LEAVES:
        t = pred[k].detach().clone()
        t = t.to(dtype=dtype or t.dtype, device=device or t.device).requires_grad_(True)
        out.overwrite(k, t)
        ls.append(t)
    return out, ls
