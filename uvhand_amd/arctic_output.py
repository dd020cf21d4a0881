"""The pose, camera and projection glue of ``make_output`` / ``prepare_data`` (arctic_tools/process.py:107-149, :249-299) as
three HIP operations (``csrc/msda_arctic_output.hip``), each one launch forward and one launch backward, without host
synchronisation:

``pose_heads(poses, roots, K, img_res)``  per pose [B, 48]: the rotation matrices [B, 16, 3, 3] of ``axis_angle_to_matrix`` and
    the axis-angle [B, 48] of ``matrix_to_axis_angle`` of those; per weak-perspective root [B, 3]: ``cam_t`` [B, 3].
``matrix_to_axis_angle_many(mats)``       the second half alone, for given matrices [B, 16, 3, 3] of up to two hands.
``place_many(segments, cam_ts, K, img_res)``  per segment ``(points [B, n, 3], camera index, project?)``: ``points + cam_t`` and,
    for projected segments, ``project_normalise`` of that and its pixel form ``0.5 img_res (x + 1)``.

Each is an autograd node over the C ABI (include/msda.h).  ``*_reference`` are the torch compositions the kernels restate
(any dtype, any device); they run for CPU tensors, non-fp32 inputs, under autocast, for a ``K`` that requires grad, for sizes
over ``msda_arctic_pose_supported`` / ``msda_arctic_place_supported`` and with ``MSDA_ARCTIC_OUTPUT_FUSED=0``.  Whenever device data
misses a kernel for a reason other than that knob, a warning names the cause once."""
import os
import warnings

import torch

from . import _native
from .object_tensors import axis_angle_to_matrix
from .small_loss import project_normalise, weak_perspective_to_perspective

PLACE_MAX_SEGMENTS = _native.ARCTIC_PLACE_MAX_SEGMENTS
PLACE_MAX_ROWS = _native.ARCTIC_PLACE_MAX_ROWS


def fused_enabled():
    return os.environ.get("MSDA_ARCTIC_OUTPUT_FUSED", "1") != "0"     # A/B knob: 0 = the torch compositions


_WARNED = set()


def _warn_restatement(what, why):
    if (what, why) not in _WARNED:
        _WARNED.add((what, why))
        warnings.warn("uvhand_amd.arctic_output.%s: %s; running the torch restatement instead of the HIP kernel" % (what, why))


# ---- the torch compositions (common/rot.py restated without boolean indexing, so without a sync) ---------------------------------
def matrix_to_quaternion(matrix):
    batch = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(batch + (9,)), dim=-1)
    x = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    pos = x > 0
    q_abs = torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))
    by_rijk = torch.stack([torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
                           torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
                           torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
                           torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    cand = by_rijk / (2.0 * q_abs[..., None].clamp(min=0.1))
    pick = q_abs.argmax(dim=-1)[..., None, None].expand(batch + (1, 4))
    return torch.gather(cand, -2, pick).squeeze(-2)


def quaternion_to_axis_angle(quaternions):
    norms = torch.norm(quaternions[..., 1:], p=2, dim=-1, keepdim=True)
    half = torch.atan2(norms, quaternions[..., :1])
    angles = 2 * half
    small = angles.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angles), angles)
    s = torch.where(small, 0.5 - (angles * angles) / 48, torch.sin(half) / safe)
    return quaternions[..., 1:] / s


def matrix_to_axis_angle(matrix):
    return quaternion_to_axis_angle(matrix_to_quaternion(matrix))


def unnormalise(kp2d, img_res):
    return 0.5 * img_res * (kp2d + 1)


def pose_heads_reference(poses, roots, K, img_res):
    mats = [axis_angle_to_matrix(p.reshape(-1, 3)).reshape(-1, 16, 3, 3) for p in poses]
    aas = [matrix_to_axis_angle(m.reshape(-1, 3, 3)).reshape(-1, 48) for m in mats]
    focal = (K[:, 0, 0] + K[:, 1, 1]) / 2.0
    return mats, aas, [weak_perspective_to_perspective(r, focal, img_res) for r in roots]


def place_many_reference(segments, cam_ts, K, img_res, pixels=True):
    out = []
    for pts, cam, proj in segments:
        placed = pts + cam_ts[cam][:, None, :]
        n2 = project_normalise(K, placed, img_res) if proj else None
        out.append((placed, n2, unnormalise(n2, img_res) if proj and pixels else None))
    return out


# ---- eligibility ----------------------------------------------------------------------------------------------------------------
def _why_not(tensors, K, B):
    """None when fp32 CUDA tensors on one device can take the kernels, "" for the two silent causes, else the reason."""
    first = K if K is not None else tensors[0]
    dev = first.device
    if dev.type != "cuda" or not fused_enabled():
        return ""
    if torch.is_autocast_enabled():
        return "autocast is on"
    for t in list(tensors) + ([K] if K is not None else []):
        if t.device != dev or t.dtype != torch.float32:
            return "inputs are not all fp32 on one device (got %s on %s)" % (t.dtype, t.device)
    if K is not None and K.requires_grad and torch.is_grad_enabled():
        return "K requires grad"
    if B == 0:
        return "empty batch"
    return None


def _route(what, why):
    if why is None:
        return True
    if why:
        _warn_restatement(what, why)
    return False


# ---- pose heads -----------------------------------------------------------------------------------------------------------------
class _PoseFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n_poses, img_res, K, *flat):
        poses, roots = list(flat[:n_poses]), list(flat[n_poses:])
        ctx.set_materialize_grads(False)
        ctx.n_poses, ctx.img_res = n_poses, img_res
        ctx.save_for_backward(K, *flat)
        mats, aas, cts = _native.arctic_pose_forward(poses, roots, K, img_res)
        return tuple(mats) + tuple(aas) + tuple(cts)

    @staticmethod
    def backward(ctx, *grads):
        K, flat = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        n = ctx.n_poses
        poses, roots = list(flat[:n]), list(flat[n:])
        g = [None if x is None else x.contiguous() for x in grads]
        want = ctx.needs_input_grad[3:]
        gp, gr = _native.arctic_pose_backward(poses, roots, K, ctx.img_res, g[:n], g[n:2 * n], g[2 * n:], want[:n], want[n:])
        return (None, None, None) + tuple(gp) + tuple(gr)


def pose_heads(poses, roots, K, img_res):
    """``(mats, aas, cam_ts)``: per pose [B, 48] of ``poses`` (up to two) the matrices [B, 16, 3, 3] and the round-tripped
    axis-angle [B, 48]; per root [B, 3] of ``roots`` (up to three) ``weak_perspective_to_perspective(root, (K00 + K11) / 2,
    img_res)``.  One launch."""
    poses, roots = list(poses), list(roots)
    B = K.shape[0]
    why = _why_not(poses + roots, K, B)
    if why is None:
        if any(p.dim() != 2 or tuple(p.shape) != (B, 48) for p in poses) or any(tuple(r.shape) != (B, 3) for r in roots) \
                or tuple(K.shape) != (B, 3, 3):
            why = "expected poses [B, 48], roots [B, 3] and K [B, 3, 3]"
        elif not poses and not roots:
            return [], [], []
        elif not _native.arctic_pose_supported(len(poses), len(roots), B):
            why = "%d poses, %d roots, B = %d is outside msda_arctic_pose_supported" % (len(poses), len(roots), B)
    if not _route("pose_heads", why):
        return pose_heads_reference(poses, roots, K, img_res)
    flat = [t.contiguous() for t in poses + roots]
    Kc = K.detach().contiguous()
    if torch.is_grad_enabled() and any(t.requires_grad for t in flat):
        out = _PoseFunction.apply(len(poses), float(img_res), Kc, *flat)
    else:
        mats, aas, cts = _native.arctic_pose_forward([t.detach() for t in flat[:len(poses)]], [t.detach() for t in flat[len(poses):]],
                                                     Kc, img_res)
        out = tuple(mats) + tuple(aas) + tuple(cts)
    n = len(poses)
    return list(out[:n]), list(out[n:2 * n]), list(out[2 * n:])


# ---- matrix to axis-angle -------------------------------------------------------------------------------------------------------
class _M2AAFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *mats):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*mats)
        return tuple(_native.arctic_m2aa_forward(list(mats)))

    @staticmethod
    def backward(ctx, *grads):
        g = [None if x is None else x.contiguous() for x in grads]
        return tuple(_native.arctic_m2aa_backward(list(ctx.saved_tensors), g, ctx.needs_input_grad))


def matrix_to_axis_angle_many(mats):
    """``[matrix_to_axis_angle(m)]`` for up to two ``m [B, 16, 3, 3]`` sharing B: aa [B, 16, 3] each.  One launch."""
    mats = list(mats)
    if not mats:
        return []
    B = mats[0].shape[0] if mats[0].dim() else 0
    why = _why_not(mats, None, B)
    if why is None:
        if any(tuple(m.shape) != (B, 16, 3, 3) for m in mats):
            why = "expected matrices [B, 16, 3, 3] sharing B"
        elif len(mats) > 2 or not _native.arctic_pose_supported(len(mats), 0, B):
            why = "%d hands, B = %d is outside msda_arctic_pose_supported" % (len(mats), B)
    if not _route("matrix_to_axis_angle_many", why):
        return [matrix_to_axis_angle(m) for m in mats]
    flat = [m.contiguous() for m in mats]
    if torch.is_grad_enabled() and any(m.requires_grad for m in flat):
        return list(_M2AAFunction.apply(*flat))
    return _native.arctic_m2aa_forward([m.detach() for m in flat])


# ---- place and project ----------------------------------------------------------------------------------------------------------
class _PlaceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cameras, projects, img_res, K, c0, c1, c2, *points):
        ctx.set_materialize_grads(False)
        ctx.geo = (cameras, projects, img_res)
        cams = [c0, c1, c2]
        ctx.has_cam = [c is not None for c in cams]
        ctx.save_for_backward(K, *[c for c in cams if c is not None], *points)
        res = _native.arctic_place_forward(list(points), cameras, projects, cams, K, img_res)
        return tuple(t for r in res for t in r if t is not None)

    @staticmethod
    def backward(ctx, *grads):
        cameras, projects, img_res = ctx.geo
        saved = list(ctx.saved_tensors)
        K = saved.pop(0)
        cams = [saved.pop(0) if has else None for has in ctx.has_cam]
        points = saved
        g = iter(None if x is None else x.contiguous() for x in grads)
        gy, gn, gpx = [], [], []
        for proj in projects:
            gy.append(next(g))
            gn.append(next(g) if proj else None)
            gpx.append(next(g) if proj else None)
        want_cams = [bool(w) and c is not None for w, c in zip(ctx.needs_input_grad[4:7], cams)]
        gp, gc = _native.arctic_place_backward(points, cameras, projects, cams, K, img_res, gy, gn, gpx, ctx.needs_input_grad[7:],
                                               want_cams)
        return (None, None, None, None) + tuple(gc) + tuple(gp)


def place_many(segments, cam_ts, K, img_res, pixels=True):
    """``[(placed, norm2d, pix2d)]`` for segments ``(points [B, n, 3], camera index into cam_ts, project?)``: ``placed = points +
    cam_ts[camera][:, None]``; for projected segments ``norm2d = project_normalise(K, placed, img_res)`` and ``pix2d = 0.5 img_res
    (norm2d + 1)``, else None.  ``cam_ts``: up to three [B, 3].  At most PLACE_MAX_SEGMENTS segments of at most PLACE_MAX_ROWS
    rows share one launch.  ``pixels=False`` lets the torch composition skip ``pix2d`` (the kernel writes it anyway)."""
    segments = [(p, int(c), bool(pr)) for p, c, pr in segments]
    cam_ts = list(cam_ts)
    if not segments:
        return []
    B = K.shape[0]
    used = sorted({c for _, c, _ in segments})
    why = _why_not([p for p, _, _ in segments] + [cam_ts[c] for c in used if 0 <= c < len(cam_ts)], K, B)
    if why is None:
        if len(cam_ts) > 3 or any(c < 0 or c >= len(cam_ts) for c in used):
            why = "camera indices must address at most three cam_ts"
        elif any(p.dim() != 3 or p.shape[0] != B or p.shape[2] != 3 or p.shape[1] < 1 for p, _, _ in segments) \
                or any(tuple(cam_ts[c].shape) != (B, 3) for c in used) or tuple(K.shape) != (B, 3, 3):
            why = "expected points [B, n, 3], cam_ts [B, 3] and K [B, 3, 3]"
        else:
            rows = max(p.shape[1] for p, _, _ in segments)
            if not _native.arctic_place_supported(len(segments), B, rows):
                why = "%d segments of up to %d rows, B = %d is outside msda_arctic_place_supported" % (len(segments), rows, B)
    if not _route("place_many", why):
        return place_many_reference(segments, cam_ts, K, img_res, pixels)
    points = [p.contiguous() for p, _, _ in segments]
    cameras, projects = tuple(c for _, c, _ in segments), tuple(pr for _, _, pr in segments)
    cams = [cam_ts[c].contiguous() if c in used else None for c in range(3)]
    Kc = K.detach().contiguous()
    if torch.is_grad_enabled() and any(t.requires_grad for t in points + [c for c in cams if c is not None]):
        flat = iter(_PlaceFunction.apply(cameras, projects, float(img_res), Kc, *cams, *points))
        return [(next(flat), next(flat) if pr else None, next(flat) if pr else None) for pr in projects]
    return _native.arctic_place_forward([p.detach() for p in points], cameras, projects,
                                        [None if c is None else c.detach() for c in cams], Kc, img_res)
