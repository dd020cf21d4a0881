"""The ARCTIC small losses: a drop-in for arctic_tools/src/callbacks/loss/loss_arctic_sf.py ``compute_small_loss`` without host
synchronisation.

``compute_small_loss(pred, gt, meta_info, pre_process_models, img_res)`` keeps the reference's signature and its 19 keys in
their insertion order (the l-hand block, the r-hand block ending with ``loss/object/transl``, ``loss/mano/transl/l``, the
object block ending with ``loss/object/v3d_smoothing``, ``loss/cd``).  ``pre_process_models`` may hold the package's ``MANO``
/ ``ObjectTensors`` or the reference's smplx MANO and ``ObjectTensors``; reference modules are converted once
(``MANO.from_smplx`` / ``ObjectTensors.from_reference``) and cached.

``ArcticSmallLoss(pre_process_models, cfg)`` has ``SetArcticCriterion``'s ``small_loss`` signature ``(outputs, targets,
meta_info, args, suffix)``: ``get_arctic_item`` then the loss, ``img_res`` from ``args``.  Its ``many(sets, targets,
meta_info, args, suffixes)`` computes every set in one pass: one ``mano_many`` call (two groups per set), one
``objects_many`` call and one loss node of two forward launches and one backward launch (``csrc/msda_small_loss.hip``) that
covers the camera conversion, projection and normalisation, the axis-angle to matrix conversion of the pose terms (pytorch3d's
quaternion route), every masked mean, the contact deviation and the smoothing term.  Gradients reach the nine
``get_arctic_item`` tensors through the MANO and object backward passes.  The reference's Python gates become device
predicates: every term is computed and selected on the device, so the step makes no host sync and captures in a graph.
Object indices come from ``meta_info["query_names"]`` (a pinned, non-blocking upload) or, for graph capture, from
``meta_info["obj_idx"]`` (int64 device tensor) with a host ``meta_info["max_len"]``.  No float atomics and fixed summation
orders: two runs, and grouped against per-set calls, are bitwise equal.

``small_loss_reference`` restates the reference's control flow in torch (its syncs included, none of its dependencies: no
pytorch3d, cv2 or loguru), in fp32 as the reference or in fp64 as the tests' yardstick.  It runs for CPU tensors, non-fp32
inputs, autocast, geometries over the kernel limits, more than ``SMALL_LOSS_MAX_SETS`` sets and ``MSDA_SMALL_LOSS_FUSED=0``.

``MSDA_SMALL_LOSS_BF16=1`` (read at call time, off by default) keeps an amp step on the kernels.  Under bf16 autocast ARCTIC's
``pred_cams`` / ``pred_mano_params`` / ``pred_obj_params`` are bf16 and its logits fp32: ``ArcticSmallLoss.many`` then selects
for every set with ``get_arctic_item_many`` (one launch instead of one per set; fp32 outputs, the bf16 values widened exactly),
and bf16 autocast alone no longer sends ``mano_many``, ``objects_many`` and the loss node to their restatements.  They call the
C ABI on fp32 tensors, and the Python glue between them runs with autocast disabled, so values are those of the same step
outside autocast on ``.float()`` predictions, bit for bit, and the bf16 leaves' gradients are that step's rounded once.  fp16
autocast and bf16 inputs to the MANO / object / loss nodes themselves keep the restatement.

The first deviation: a skipped hand block (no frame with ``is_valid * hand_valid``) returns shape ``[1]`` zeros where the
reference returns 0-d zeros, since a data-dependent shape would need a sync.  ``loss/cd`` and ``loss/object/v3d_smoothing``
are 0-d as in the reference.  A second one: with a single frame the reference's ``obj_smt_loss`` raises (it reads ``v[1]``);
the kernel path returns ``loss/object/v3d_smoothing`` = 0 with a zero gradient, as there is no consecutive pair."""
import os

import torch

from . import _native
from ._autocast import autocast_refuses, no_autocast, small_loss_bf16_enabled
from .arctic_item import get_arctic_item, get_arctic_item_many
from .mano import MANO, mano_many
from .object_tensors import ObjectTensors, axis_angle_to_matrix, objects_many

SMALL_LOSS_MAX_SETS = _native.SMALL_LOSS_MAX_SETS
KEYS = ("loss/mano/kp2d/l", "loss/mano/pose/l", "loss/mano/beta/l", "loss/mano/cam_t/l", "loss/mano/kp3d/l",
        "loss/mano/kp2d/r", "loss/mano/pose/r", "loss/mano/beta/r", "loss/mano/cam_t/r", "loss/mano/kp3d/r",
        "loss/object/transl", "loss/mano/transl/l",
        "loss/object/kp2d", "loss/object/cam_t", "loss/object/kp3d", "loss/object/radian", "loss/object/rot",
        "loss/object/v3d_smoothing", "loss/cd")
_SCALAR_KEYS = ("loss/object/v3d_smoothing", "loss/cd")          # 0-d, as the reference's


# ---- torch restatement ----------------------------------------------------------------------------------------------------------
def _mse(a, b):
    return (a - b) ** 2


def vector_loss(pred, gt, is_valid):
    dist = _mse(pred, gt)
    if is_valid.sum() == 0:
        return torch.zeros(1, dtype=dist.dtype, device=dist.device)
    return dist[is_valid.long().bool()].mean().view(-1)


def joints_loss(pred, gt, jts_valid):
    return (_mse(pred, gt) * jts_valid[:, :, None]).mean().view(-1)


def _subtract_root(x, root):
    return x - x[:, root:root + 1]


def hand_kp3d_loss(pred, gt, jts_valid):
    p, g = _subtract_root(pred, 0), _subtract_root(gt, 0)
    return joints_loss(_subtract_root(p, 0), _subtract_root(g, 0), jts_valid)


def object_kp3d_loss(pred, gt, is_valid):
    n = pred.shape[1] // 2
    return vector_loss(_subtract_root(pred, n), _subtract_root(gt, n), is_valid)


def weak_perspective_to_perspective(cam, focal_length, img_res, min_s=0.1):
    s = torch.clamp(cam[:, 0], min_s)
    return torch.stack([cam[:, 1], cam[:, 2], 2 * focal_length / (img_res * s + 1e-9)], dim=-1)


def project_normalise(K, pts, img_res):
    """K p, then x / z and y / z, normalised to 2 u / img_res - 1."""
    h = torch.bmm(K, pts.permute(0, 2, 1)).permute(0, 2, 1)
    xy = h[:, :, :2] / h[:, :, 2:3]
    return 2.0 * xy / img_res - 1.0


def _nanmean(v, *args, **kwargs):
    is_nan = torch.isnan(v)
    v = v.masked_fill(is_nan, 0)
    return v.sum(*args, **kwargs) / (~is_nan).to(v.dtype).sum(*args, **kwargs)


def contact_deviation(v_o, v_h, dist, idx, is_valid, hand_valid):
    valid = hand_valid * is_valid
    corres = torch.gather(v_o, 1, idx[:, :, None].repeat(1, 1, 3))
    disp = corres - v_h
    nan = torch.full_like(disp, float("nan"))
    disp = torch.where(((1 - valid) != 0)[:, None, None], nan, disp)
    disp = torch.where((dist > 3e-3)[:, :, None], nan, disp)
    return _nanmean(torch.sqrt((disp ** 2).sum(dim=2)), 1)


def obj_smt_loss(v):
    loss = (v[0] - v[1]).abs().sum()
    for i in range(1, v.shape[0] - 1):
        loss = loss + (v[i] - v[i + 1]).abs().sum()
    return loss


def small_loss_reference(pred, gt, meta_info, pre_process_models, img_res, dtype=torch.float32):
    """compute_small_loss restated with the reference's control flow, in ``dtype`` (the reference: fp32)."""
    root, mano_pose, mano_shape, obj_angle = pred
    root_l, root_r, root_o = [t.to(dtype) for t in root]
    betas_l, betas_r = [t.to(dtype) for t in mano_shape]
    pose_l, pose_r = [t.to(dtype) for t in mano_pose]
    rot = obj_angle[0].reshape(-1, 3).to(dtype)
    radian = obj_angle[1].reshape(-1).to(dtype)
    g = lambda k: gt[k].to(dtype)  # noqa: E731
    gt_kp2d_o = torch.cat((gt["object.kp2d.norm.t"], gt["object.kp2d.norm.b"]), dim=1).to(dtype)
    is_valid, right_valid, left_valid = g("is_valid"), g("right_valid"), g("left_valid")
    device = is_valid.device
    K = meta_info["intrinsics"].to(dtype)
    focal = (K[:, 0, 0] + K[:, 1, 1]) / 2.0
    cam_t_l, cam_t_r, cam_t_o = [weak_perspective_to_perspective(r, focal, img_res) for r in (root_l, root_r, root_o)]
    zero = lambda: torch.tensor(0, dtype=dtype, device=device)  # noqa: E731
    tmp, d = {}, {}
    for side, cam_t, rr, betas, pose, valid in (("l", cam_t_l, root_l, betas_l, pose_l, left_valid),
                                               ("r", cam_t_r, root_r, betas_r, pose_r, right_valid)):
        if sum(is_valid * valid) != 0:
            out = pre_process_models["mano_" + side](betas=betas, hand_pose=pose[:, 3:], global_orient=pose[:, :3])
            j3d = out.joints.to(dtype) + cam_t[:, None, :]
            tmp["mano.v3d.cam." + side] = out.vertices.to(dtype) + cam_t[:, None, :]
            kp2d = project_normalise(K, j3d, img_res)
            rot_gt = axis_angle_to_matrix(g("mano.pose." + side).reshape(-1, 3)).reshape(-1, 16, 3, 3)
            rot_p = axis_angle_to_matrix(pose.reshape(-1, 3)).reshape(-1, 16, 3, 3)
            jv = g("joints_valid_" + side)
            d["loss/mano/kp2d/" + side] = joints_loss(kp2d, g("mano.j2d.norm." + side), jv)
            d["loss/mano/pose/" + side] = vector_loss(rot_p, rot_gt, valid)
            d["loss/mano/beta/" + side] = vector_loss(betas, g("mano.beta." + side), valid)
            d["loss/mano/cam_t/" + side] = vector_loss(rr, g("mano.cam_t.wp." + side), valid)
            d["loss/mano/kp3d/" + side] = hand_kp3d_loss(j3d, g("mano.j3d.cam." + side), jv)
            if side == "r":
                d["loss/object/transl"] = vector_loss(root_o - root_r, g("object.cam_t.wp") - g("mano.cam_t.wp.r"),
                                                      right_valid * is_valid)
        else:
            for k in ("kp2d", "pose", "beta", "cam_t", "kp3d"):
                d["loss/mano/%s/%s" % (k, side)] = zero()
            if side == "r":
                d["loss/object/transl"] = zero()
    if sum(is_valid * left_valid) != 0 and sum(is_valid * right_valid) != 0:
        d["loss/mano/transl/l"] = vector_loss(root_l - root_r, g("mano.cam_t.wp.l") - g("mano.cam_t.wp.r"),
                                              right_valid * left_valid)
    else:
        d["loss/mano/transl/l"] = zero()
    head = pre_process_models["arti_head"]
    if isinstance(head, ObjectTensors) and meta_info.get("obj_idx") is not None:
        obj = head.forward(radian.view(-1, 1), rot, None, None, obj_idx=meta_info["obj_idx"], max_len=meta_info["max_len"])
    else:
        obj = head.forward(radian.view(-1, 1), rot, None, meta_info["query_names"])
    kp3d_o = obj["kp3d"].to(dtype) + cam_t_o[:, None, :]
    v3d_o = obj["v"].to(dtype) + cam_t_o[:, None, :]
    d["loss/object/kp2d"] = vector_loss(project_normalise(K, kp3d_o, img_res), gt_kp2d_o, is_valid)
    d["loss/object/cam_t"] = vector_loss(root_o, g("object.cam_t.wp"), is_valid)
    d["loss/object/kp3d"] = object_kp3d_loss(kp3d_o, g("object.kp3d.cam"), is_valid)
    d["loss/object/radian"] = vector_loss(radian, g("object.radian").reshape(-1), is_valid)
    d["loss/object/rot"] = vector_loss(rot, g("object.rot").reshape(-1, 3), is_valid)
    d["loss/object/v3d_smoothing"] = obj_smt_loss(v3d_o)
    loss_cd = zero()
    for side, key in (("r", "ro"), ("l", "lo")):
        if "mano.v3d.cam." + side in tmp:
            cd = contact_deviation(v3d_o, tmp["mano.v3d.cam." + side], gt["dist." + key].to(dtype), gt["idx." + key],
                                   gt["is_valid"].to(dtype), gt[("right" if side == "r" else "left") + "_valid"].to(dtype))
            loss_cd = loss_cd + torch.nan_to_num(_nanmean(cd))
    d["loss/cd"] = loss_cd
    return {k: d[k] for k in KEYS}


# ---- model conversion -----------------------------------------------------------------------------------------------------------
_CONVERTED = {}


def _convert(models):
    """The package's MANO / ObjectTensors for pre_process_models (reference modules converted once, cached by identity)."""
    key = tuple(id(models[k]) for k in ("mano_l", "mano_r", "arti_head"))
    hit = _CONVERTED.get(key)
    if hit is not None and all(hit[0][k] is models[k] for k in ("mano_l", "mano_r", "arti_head")):
        return hit[1]
    out = {}
    for k in ("mano_l", "mano_r"):
        out[k] = models[k] if isinstance(models[k], MANO) else MANO.from_smplx(models[k])
    m = models["arti_head"]
    out["arti_head"] = m if isinstance(m, ObjectTensors) else ObjectTensors.from_reference(m)
    _CONVERTED[key] = ({k: models[k] for k in ("mano_l", "mano_r", "arti_head")}, out)
    return out


# ---- the HIP node ---------------------------------------------------------------------------------------------------------------
def _fused_enabled():
    return os.environ.get("MSDA_SMALL_LOSS_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatement


def _targets(gt, meta_info, dev):
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    B = gt["is_valid"].shape[0]
    kp2d_o = torch.cat((gt["object.kp2d.norm.t"], gt["object.kp2d.norm.b"]), dim=1)
    ts = [f(gt["mano.pose.l"].reshape(B, -1)), f(gt["mano.pose.r"].reshape(B, -1)), f(gt["mano.beta.l"]),
          f(gt["mano.beta.r"]), f(gt["mano.j3d.cam.l"]), f(gt["mano.j3d.cam.r"]), f(gt["object.kp3d.cam"]),
          f(gt["mano.j2d.norm.l"]), f(gt["mano.j2d.norm.r"]), f(kp2d_o), f(gt["object.rot"].reshape(B, 3)),
          f(gt["object.radian"].reshape(B)), f(gt["mano.cam_t.wp.l"]), f(gt["mano.cam_t.wp.r"]), f(gt["object.cam_t.wp"]),
          f(gt["is_valid"]), f(gt["left_valid"]), f(gt["right_valid"]), f(gt["joints_valid_l"]), f(gt["joints_valid_r"]),
          f(gt["dist.ro"]), f(gt["dist.lo"]), f(meta_info["intrinsics"])]
    idx = [gt["idx.ro"].to(device=dev, dtype=torch.int64).contiguous(), gt["idx.lo"].to(device=dev, dtype=torch.int64).contiguous()]
    return ts + idx


class _SmallLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *flat):
        dims, img_res, targets = meta
        n = _native.SMALL_LOSS_INPUTS
        inputs = [list(flat[n * i:n * i + n]) for i in range(dims[0])]
        losses, ws = _native.small_loss_forward(dims, img_res, targets, inputs)
        ctx.meta, ctx.ws = meta, ws
        ctx.save_for_backward(*flat)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        dims, img_res, targets = ctx.meta
        flat = ctx.saved_tensors
        n = _native.SMALL_LOSS_INPUTS
        inputs = [list(flat[n * i:n * i + n]) for i in range(dims[0])]
        grads = _native.small_loss_backward(dims, img_res, targets, inputs, grad_losses.contiguous(), ctx.ws)
        res = [g for grp in grads for g in grp]
        return (None,) + tuple(r if need else None for r, need in zip(res, ctx.needs_input_grad[1:]))


def _flat_pred(pred):
    root, pose, shape, obj = pred
    return list(root) + list(pose) + list(shape) + [obj[0], obj[1]]


def _fused_ok(preds, gt, models):
    if not (_fused_enabled() and preds) or autocast_refuses() or len(preds) > SMALL_LOSS_MAX_SETS:
        return False
    ts = [t for p in preds for t in _flat_pred(p)]
    dev = ts[0].device
    if dev.type != "cuda" or any(not torch.is_tensor(t) or t.device != dev or t.dtype != torch.float32 for t in ts):
        return False
    return all(k in models for k in ("mano_l", "mano_r", "arti_head"))


def _object_index(obj, meta_info):
    if meta_info.get("obj_idx") is not None:
        if meta_info.get("max_len") is None:
            raise ValueError("meta_info['obj_idx'] needs a host meta_info['max_len']")
        return meta_info["obj_idx"], int(meta_info["max_len"])
    return obj.obj_index(meta_info["query_names"])


def _fused(preds, gt, meta_info, models, img_res):
    """Per set the 19-key dict through one mano_many, one objects_many and one loss node; None where the restatement runs."""
    models = _convert(models)
    mano_l, mano_r, obj = models["mano_l"], models["mano_r"], models["arti_head"]
    dev = preds[0][0][0].device
    B = preds[0][0][0].shape[0]
    if B == 0 or any(p[0][0].shape[0] != B for p in preds) or obj.obj_tensors["v"].device != dev:
        return None
    obj_idx, max_len = _object_index(obj, meta_info)
    J = 16 + len(mano_l._extra)
    dims = [len(preds), B, J, mano_l.v_template.shape[0], obj.obj_tensors["kp_top"].shape[1] + obj.obj_tensors["kp_bottom"].shape[1],
            mano_l.num_betas, max_len]
    if mano_r._dims() != mano_l._dims() or not _native.small_loss_supported(*dims):
        return None
    calls = []
    for (_, pose, shape, _) in preds:
        calls.append((mano_l, shape[0], pose[0][:, :3], pose[0][:, 3:]))
        calls.append((mano_r, shape[1], pose[1][:, :3], pose[1][:, 3:]))
    hands = mano_many(calls)
    objs = objects_many([(obj, p[3][1].view(-1, 1), p[3][0].reshape(-1, 3), None, obj_idx, max_len) for p in preds])
    flat = []
    for i, p in enumerate(preds):
        (rl, rr, ro), (pl, pr), (bl, br), (rot, rad) = p
        hl, hr, o = hands[2 * i], hands[2 * i + 1], objs[i]
        flat += [rl, rr, ro, pl, pr, bl, br, rot.reshape(-1, 3), rad.reshape(-1), hl.vertices, hr.vertices, hl.joints,
                 hr.joints, o["v"], o["kp3d"]]
    flat = [t.contiguous() for t in flat]
    targets = _targets(gt, meta_info, dev)
    if torch.is_grad_enabled() and any(t.requires_grad for t in flat):
        L = _SmallLossFunction.apply((dims, float(img_res), targets), *flat)
    else:
        L = _native.small_loss_forward(dims, float(img_res), targets,
                                       [flat[15 * i:15 * i + 15] for i in range(len(preds))])[0]
    return [{k: (L[s, c] if k in _SCALAR_KEYS else L[s, c:c + 1]) for c, k in enumerate(KEYS)} for s in range(len(preds))]


def small_loss_many(preds, gt, meta_info, pre_process_models, img_res):
    """One 19-key dict per set of ``preds`` (each in get_arctic_item's structure)."""
    if _fused_ok(preds, gt, pre_process_models):
        with no_autocast():          # the nodes call the C ABI; no torch op of the glue between them is autocast
            out = _fused(preds, gt, meta_info, pre_process_models, img_res)
        if out is not None:
            return out
    return [small_loss_reference(p, gt, meta_info, pre_process_models, img_res) for p in preds]


def compute_small_loss(pred, gt, meta_info, pre_process_models, img_res, device=None):
    """Drop-in for loss_arctic_sf.compute_small_loss (``device`` accepted for the signature; results live with the inputs)."""
    return small_loss_many([pred], gt, meta_info, pre_process_models, img_res)[0]


class ArcticSmallLoss:
    """``SetArcticCriterion(..., small_loss=ArcticSmallLoss(pre_process_models, cfg))``: get_arctic_item + the small losses
    per set, and ``many`` for all sets in one pass."""

    def __init__(self, pre_process_models, cfg):
        self.pre_process_models = pre_process_models
        self.cfg = cfg

    def __call__(self, outputs, targets, meta_info, args, suffix):
        return self.many([outputs], targets, meta_info, args, [suffix])[0]

    def many(self, sets, targets, meta_info, args, suffixes):
        if small_loss_bf16_enabled():
            preds = get_arctic_item_many(sets, self.cfg, getattr(args, "device", None))
        else:
            preds = [get_arctic_item(o, self.cfg, getattr(args, "device", None)) for o in sets]
        dicts = small_loss_many(preds, targets, meta_info, self.pre_process_models, args.img_res)
        return [{k + sfx: v for k, v in d.items()} for d, sfx in zip(dicts, suffixes)]
