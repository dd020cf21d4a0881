"""The SmoothNet criterion's losses: a drop-in for arctic_tools/src/callbacks/loss/loss_arctic_sf.py ``compute_smoothnet_loss``
(402-548) and for src/utils/eval_modules.py ``eval_acc_pose`` / ``compute_error_accel`` (254-368) without host
synchronisation.

``compute_smoothnet_loss(pred, gt, meta_info, pre_process_models, img_res, device=None, acc_grad=False)`` keeps the reference's
signature and returns its three keys in its order, ``("loss/cd", "acc/h", "acc/o")``, all 0-d fp32.  ``pred`` / ``gt`` are the
``pred.`` / ``targets.`` halves of ``prepare_data``'s dict.  On CUDA fp32 data it is one autograd node of three forward launches
and one backward launch (``csrc/msda_smooth_loss.hip``): every Python gate of the reference (the ``.nonzero()`` rows of the
contact deviation, ``np.convolve``'s validity, the "any non-NaN" test) is a device predicate, so the step makes no host sync
and captures in a graph.  No float atomics and fixed summation orders: two runs are bitwise equal, values and gradients.
The kernels are fp32 except for the object root, a mean of coordinates at the camera's depth, which they sum, keep and
subtract in fp64, so ``acc/o`` is closer to the exact value than the reference's fp32 run.

``acc_grad``.  In the reference ``acc/h`` and ``acc/o`` pass through numpy: they are constants, and the smoother trains on
``loss/cd`` alone whatever ``weight_dict`` says.  ``acc_grad=False`` (the default) reproduces that: the two terms are detached.
``acc_grad=True`` returns the same values with gradients into ``pred["mano.v3d.cam.{r,l}"]``, ``pred["mano.j3d.cam.{r,l}"]``
(row 0, the root) and ``pred["object.v.cam"]``.

``smooth_loss_reference`` restates the reference's control flow in torch (its syncs included; no pytorch3d, no numpy round
trip), in fp32 as the reference runs it or in fp64 as the tests' yardstick.  It runs for CPU tensors, non-fp32 or mismatched
dtypes, autocast, geometries over ``msda_smooth_loss_supported``, a prediction and a gt object of different padded length and
``MSDA_SMOOTH_LOSS_FUSED=0``; device data of a wrong dtype warns once, naming the key.

What the reference does and this keeps: accelerations run along the flat frame axis N = B * T, across window boundaries,
stencil ``[1, -2, 1] * fps ** 2``; a centre frame counts iff the validity product at t - 1, t, t + 1 sums to 3 after truncation
to int64 (a 0.5 flag invalidates; the contact deviation keeps ``(1 - valid) != 0``); the object root of every frame is the mean
over the columns where ``parts_ids[0] == 2`` (frame 0's ids, over the whole padded length); the per-frame error is the mean
over all padded columns.  Deviations: with no valid centre frame, or N < 3, the reference returns an int64 ``torch.tensor(0)``
(N < 3: it raises on its index mismatch) where this returns an fp32 0-d zero with a zero gradient."""
import os
import warnings

import numpy as np
import torch

from . import _native
from .small_loss import _nanmean, contact_deviation

KEYS = ("loss/cd", "acc/h", "acc/o")
_PRED_KEYS = ("mano.v3d.cam.r", "mano.v3d.cam.l", "mano.j3d.cam.r", "mano.j3d.cam.l", "object.v.cam")
_GT_FLOAT_KEYS = _PRED_KEYS + ("dist.ro", "dist.lo", "is_valid", "left_valid", "right_valid")
_GT_LONG_KEYS = ("idx.ro", "idx.lo", "object.parts_ids")


# ---- torch restatement ----------------------------------------------------------------------------------------------------------
def compute_error_accel(joints_gt, joints_pred, fps=30.0):
    """eval_modules.py:254-280: the mean over columns of |accel_pred - accel_gt|, [N - 2], in m/s^2."""
    step2 = (1 / fps) ** 2                               # the reference divides by h^2, h = 1 / fps: kept for its rounding

    def stencil(x):
        return (x[:-2] - 2 * x[1:-1] + x[2:]) / step2
    return (stencil(joints_pred) - stencil(joints_gt)).norm(dim=2).mean(dim=1)


def _convolve_valid(v):
    """np.convolve(v, np.ones(3), mode='valid').astype(np.int64) == 3 on the host, as the reference (fp64 sums)."""
    v = v.detach().cpu().double()
    return (v[:-2] + v[1:-1] + v[2:]).long() == 3


def _acc_rows(pred, targets, dtype):
    """eval_acc_pose up to its padding: (acc_h [N], acc_o [N - 2]) with NaN where a frame does not count; None for N < 3."""
    f = lambda t: t.to(dtype)  # noqa: E731
    gt_vo, gt_vr, gt_vl = f(targets["object.v.cam"]), f(targets["mano.v3d.cam.r"]), f(targets["mano.v3d.cam.l"])
    pred_vo, pred_vr, pred_vl = f(pred["object.v.cam"]), f(pred["mano.v3d.cam.r"]), f(pred["mano.v3d.cam.l"])
    if gt_vo.shape[0] < 3:
        return None
    pred_root_r, pred_root_l = f(pred["mano.j3d.cam.r"])[:, :1], f(pred["mano.j3d.cam.l"])[:, :1]
    gt_root_r, gt_root_l = f(targets["mano.j3d.cam.r"])[:, :1], f(targets["mano.j3d.cam.l"])[:, :1]
    bottom_idx = targets["object.parts_ids"][0] == 2
    gt_root_o = gt_vo[:, bottom_idx].mean(dim=1)[:, None, :]
    pred_root_o = pred_vo[:, bottom_idx].mean(dim=1)[:, None, :]
    acc_r = compute_error_accel(gt_vr - gt_root_r, pred_vr - pred_root_r)
    acc_l = compute_error_accel(gt_vl - gt_root_l, pred_vl - pred_root_l)
    acc_o = compute_error_accel(gt_vo - gt_root_o, pred_vo - pred_root_o)
    is_valid = f(targets["is_valid"])
    left_valid, right_valid = f(targets["left_valid"]) * is_valid, f(targets["right_valid"]) * is_valid
    dev = acc_r.device
    nan = torch.full_like(acc_r, float("nan"))
    acc_r = torch.where(_convolve_valid(right_valid).to(dev), acc_r, nan)
    acc_l = torch.where(_convolve_valid(left_valid).to(dev), acc_l, nan)
    acc_o = torch.where(_convolve_valid(is_valid).to(dev), acc_o, nan)
    acc_h = _nanmean(torch.stack((acc_r, acc_l), dim=1), dim=1)
    pad = torch.full((1,), float("nan"), dtype=dtype, device=dev)
    return torch.cat((pad, acc_h, pad)), acc_o


def smooth_loss_reference(pred, gt, dtype=torch.float32, acc_grad=False):
    """compute_smoothnet_loss restated with the reference's control flow, in ``dtype`` (the reference: fp32)."""
    f = lambda t: t.to(dtype)  # noqa: E731
    dev = gt["is_valid"].device
    zero = lambda: torch.tensor(0, dtype=dtype, device=dev)  # noqa: E731
    loss_cd = zero()
    for side, key, valid in (("r", "ro", "right_valid"), ("l", "lo", "left_valid")):
        if "mano.v3d.cam." + side in pred.keys():
            cd = contact_deviation(f(pred["object.v.cam"]), f(pred["mano.v3d.cam." + side]), f(gt["dist." + key]), gt["idx." + key],
                                   f(gt["is_valid"]), f(gt[valid]))
            loss_cd = loss_cd + torch.nan_to_num(_nanmean(cd))
    d = {"loss/cd": loss_cd}
    rows = _acc_rows(pred, gt, dtype)
    for k, v in zip(("acc/h", "acc/o"), rows if rows is not None else (None, None)):
        if v is None or not bool((~torch.isnan(v)).sum() != 0):
            d[k] = zero()
        else:
            d[k] = _nanmean(v) if acc_grad else _nanmean(v.detach())
    return {k: d[k] for k in KEYS}


# ---- the HIP node ---------------------------------------------------------------------------------------------------------------
def _fused_enabled():
    return os.environ.get("MSDA_SMOOTH_LOSS_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatement


_WARNED = set()


def _warn_restatement(what, why):
    """Once per cause: device data that the kernels could have served runs the (syncing) torch restatement."""
    if (what, why) not in _WARNED:
        _WARNED.add((what, why))
        warnings.warn("uvhand_amd.smooth_loss.%s: %s; running the torch restatement instead of the HIP kernel" % (what, why))


def _plan(what, pred, gt):
    """(dims, floats, longs) for the kernels, or None where the restatement runs (with a warning, once per cause, when the
    data is on the device and the kernels are not switched off)."""
    iv = gt["is_valid"]
    if not _fused_enabled() or not torch.is_tensor(iv) or iv.device.type != "cuda":
        return None
    dev = iv.device
    no = lambda why: _warn_restatement(what, why)  # noqa: E731
    if torch.is_autocast_enabled():
        return no("autocast is on")
    named = [("pred." + k, pred[k], torch.float32) for k in _PRED_KEYS] + [("targets." + k, gt[k], torch.float32) for k in _GT_FLOAT_KEYS] \
        + [("targets." + k, gt[k], torch.int64) for k in _GT_LONG_KEYS]
    for k, t, want in named:
        if not torch.is_tensor(t) or t.device != dev or t.dtype != want:
            return no("%r must be a %s tensor on %s (got %s)" % (k, want, dev, "%s on %s" % (t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    ts = [t for _, t, _ in named]
    vr, jr, vo = ts[0], ts[2], ts[4]
    if vr.dim() != 3 or jr.dim() != 3 or vo.dim() != 3:
        return no("unexpected tensor ranks")
    N, NV, J, L = vo.shape[0], vr.shape[1], jr.shape[1], vo.shape[1]
    dims = [N, NV, J, L]
    shapes = [(N, NV, 3), (N, NV, 3), (N, J, 3), (N, J, 3), (N, L, 3)] * 2 + [(N, NV), (N, NV), (N,), (N,), (N,), (N, NV), (N, NV), (N, L)]
    ts = [t.reshape(-1) if s == (N,) and t.numel() == N else t for t, s in zip(ts, shapes)]
    if any(tuple(t.shape) != s for t, s in zip(ts, shapes)):
        return no("shapes are inconsistent (a prediction and a gt object of different padded length among them)")
    if N == 0 or not _native.smooth_loss_supported(*dims):
        return no("N = %d, NV = %d, J = %d, L = %d is outside msda_smooth_loss_supported" % tuple(dims))
    pred_ts = [t.contiguous() for t in ts[:5]]
    rest = [t.detach().contiguous() for t in ts[5:]]
    return dims, pred_ts, rest[:10], rest[10:]


class _SmoothLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *pred_ts):
        dims, gt_floats, longs, acc_grad = meta
        losses, _, ws = _native.smooth_loss_forward(dims, 30.0, list(pred_ts) + gt_floats, longs)
        ctx.meta, ctx.ws = meta, ws
        ctx.save_for_backward(*pred_ts)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        dims, gt_floats, longs, acc_grad = ctx.meta
        grads = _native.smooth_loss_backward(dims, 30.0, list(ctx.saved_tensors) + gt_floats, longs, grad_losses.contiguous(),
                                             ctx.ws, acc_grad)
        return (None,) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[1:]))


def compute_smoothnet_loss(pred, gt, meta_info, pre_process_models, img_res, device=None, acc_grad=False):
    """Drop-in for loss_arctic_sf.compute_smoothnet_loss (``meta_info``, ``pre_process_models``, ``img_res`` and ``device`` are
    accepted for the signature: the live terms read none of them; results live with the inputs)."""
    plan = _plan("compute_smoothnet_loss", pred, gt)
    if plan is None:
        return smooth_loss_reference(pred, gt, dtype=torch.float32, acc_grad=acc_grad)
    dims, pred_ts, gt_floats, longs = plan
    if torch.is_grad_enabled() and any(t.requires_grad for t in pred_ts):
        L = _SmoothLossFunction.apply((dims, gt_floats, longs, bool(acc_grad)), *pred_ts)
    else:
        L = _native.smooth_loss_forward(dims, 30.0, [t.detach() for t in pred_ts] + gt_floats, longs)[0]
    return {"loss/cd": L[0], "acc/h": L[1] if acc_grad else L[1].detach(), "acc/o": L[2] if acc_grad else L[2].detach()}


def eval_acc_pose(pred, targets, meta_info):
    """Drop-in for eval_modules.eval_acc_pose: ``{"acc/h": [N] with NaN at both ends, "acc/o": [N - 2]}`` as numpy arrays in
    m/s^2.  On device data: the forward launches and one copy.  N < 3 (the reference raises): all NaN / empty."""
    from .arctic_eval import XDict
    plan = _plan("eval_acc_pose", pred, targets)
    N = targets["object.v.cam"].shape[0]
    out = XDict()
    if plan is not None:
        dims, pred_ts, gt_floats, longs = plan
        frames = _native.smooth_loss_forward(dims, 30.0, [t.detach() for t in pred_ts] + gt_floats, longs, want_frames=True)[1]
        frames = frames.cpu().numpy()
        out["acc/h"], out["acc/o"] = frames[0].copy(), frames[1, :max(N - 2, 0)].copy()
        return out
    with torch.no_grad():
        rows = _acc_rows(pred, targets, torch.float32)
    if rows is None:
        out["acc/h"], out["acc/o"] = np.full(N, np.nan, dtype=np.float32), np.zeros(0, dtype=np.float32)
    else:
        out["acc/h"], out["acc/o"] = rows[0].cpu().numpy(), rows[1].cpu().numpy()
    return out
