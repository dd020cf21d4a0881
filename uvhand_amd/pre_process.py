"""The first call of every ARCTIC step: a drop-in for arctic_tools/process.py ``arctic_pre_process`` (72-93) over
src/callbacks/process/process_arctic.py ``process_data`` and process_generic.py ``prepare_interfield``, without host
synchronisation.  The reference builds two MANO layers and an ``ArtiHead`` from disk per call, poses the object twice, goes to
the host for the rigid fit (``batch_solve_rigid_tf``) and for a per-frame loop of ``np.linalg.solve``
(``estimate_translation_k``), and ends in pytorch3d's ``knn_points``, which does not exist on ROCm.

``fit_targets(kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l, img_res=224)``  one launch for the batch
    (``csrc/msda_pre_process.hip``): ``R0, T0`` of Arun's method between ``object.kp3d.full.b`` and the posed object's bottom
    keypoints, both hands' joints moved by it, the ``Tr0`` / ``Tl0`` means, the camera translation of
    ``estimate_translation_k_np`` with unit weights, and the weak-perspective cameras.  Returns ``(outputs, status)``: a dict
    with the keys ``FIT_OUTPUTS`` and an int32 ``[B]`` of bits: 1 the fit had a negative determinant (the reference raises
    there; the corrected rotation is returned), 2 the rotation is not unique (second singular value of H below 1e-6 of the
    first), 4 a non-finite input (the frame's outputs are NaN and no other bit is set), 8 a singular normal matrix (``transl``
    and what depends on it are NaN).  A rank-deficient H (planar keypoints) has no orientation and never sets bit 1.
``distance_fields(hand_r, hand_l, obj, v_len, dist_min=0.0, dist_max=inf)``  one launch for the four contact fields of
    ``prepare_interfield``.  Returns a dict ``dist.ro, dist.lo, dist.or, dist.ol, idx.ro, idx.lo, idx.or, idx.ol``.  Object rows at
    or beyond ``v_len`` are never candidates; as sources they get distance 0 (before the clamp) and index 0, which is what
    ``knn_points`` leaves in its zero-initialised outputs; ``v_len`` is clamped to ``[0, L]`` and a frame with ``v_len = 0``
    gives every hand vertex 0 and 0 as well.
``fit_targets_reference`` / ``distance_fields_reference`` restate both in torch (``torch.linalg.svd``, ``torch.linalg.solve``,
    chunked brute force) in the inputs' dtype with the same outputs and status bits; in fp64 they are the yardstick.  They run
    for CPU tensors, non-fp32 inputs, sizes outside ``msda_pre_fit_supported`` / ``msda_dist_fields_supported`` and with
    ``MSDA_PRE_PROCESS_FUSED=0`` (read at call time).  Whenever device data misses a kernel for a reason other than that
    knob, a warning names the cause once.

``pre_process(targets, meta_info, models=None, obj_idx=None, max_len=None)`` is the device API: under ``no_grad``, one
``objects_many`` (the reference's second, identical object forward is not repeated), one ``mano_many`` for both hands, ``fit_targets``,
one ``place_many`` (the cameras are the two vertex offsets and ``transl``), ``distance_fields``: five library launches, no sync,
and with ``obj_idx`` / ``max_len`` capturable in a graph.  It writes ``process_data``'s keys into ``targets`` in its order and
returns ``(targets, meta_info)`` with ``meta_info`` an ``XDict`` holding ``part_ids``, ``diameter``, ``object.v_len``,
``mano.faces.r``, ``mano.faces.l`` and ``fit_status``.  ``arctic_pre_process(args, targets, meta_info, models=None,
check=False)`` has the reference's signature; ``check=True`` reads ``fit_status`` once (one sync) and raises as the reference
does on a negative determinant."""
import math
import os
import warnings

import torch

from . import _native
from .arctic_eval import XDict, _models
from .arctic_output import place_many
from .mano import mano_many
from .object_tensors import objects_many

IMG_RES = 224                                   # process_data's constant, not args.img_res
FIT_OUTPUTS = _native.PRE_FIT_OUTPUTS
FIELD_KEYS = ("dist.ro", "dist.lo", "dist.or", "dist.ol", "idx.ro", "idx.lo", "idx.or", "idx.ol")
STATUS_DET_NEGATIVE, STATUS_NOT_UNIQUE, STATUS_NON_FINITE, STATUS_SINGULAR = 1, 2, 4, 8
_RANK_TOL, _UNIQUE_TOL, _SINGULAR_TOL = 1e-12, 1e-6, 1e-12      # msda_pre_fit.h


def _fused_enabled():
    return os.environ.get("MSDA_PRE_PROCESS_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatements


_WARNED = set()


def _warn_restatement(what, why):
    if (what, why) not in _WARNED:
        _WARNED.add((what, why))
        warnings.warn("uvhand_amd.pre_process.%s: %s; running the torch restatement instead of the HIP kernel" % (what, why))


# ---- the torch restatements -----------------------------------------------------------------------------------------------------
def _safe_frame(NK, J, dtype, dev):
    """A well-conditioned frame that stands in for one with non-finite inputs (its results are overwritten with NaN)."""
    k = torch.arange(NK, dtype=dtype, device=dev)
    kp = torch.stack([torch.cos(k), torch.sin(2 * k + 1), 0.5 * torch.cos(3 * k + 2)], dim=1) * 0.1
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]], dtype=dtype, device=dev)
    return [kp, kp, 4.0 * kp[:, :2], K] + [torch.zeros(J, 3, dtype=dtype, device=dev)] * 4


def fit_targets_reference(kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l, img_res=IMG_RES):
    """``fit_targets`` in torch, in the inputs' dtype: ``(outputs, status)``."""
    ins = [kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l]
    dtype, dev = kp_full.dtype, kp_full.device
    B, NK, _ = kp_full.shape
    J = j_full_r.shape[1]
    bad = torch.zeros(B, dtype=torch.bool, device=dev)
    for t in ins:
        bad = bad | ~torch.isfinite(t).flatten(1).all(dim=1)
    ins = [torch.where(bad.view(-1, 1, 1), s.to(dtype)[None], t.to(dtype)) for t, s in zip(ins, _safe_frame(NK, J, dtype, dev))]
    kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l = ins
    # batch_solve_rigid_tf
    cA, cB = kp_full.mean(dim=1), kp_cano.mean(dim=1)
    H = (kp_full - cA[:, None]).transpose(1, 2) @ (kp_cano - cB[:, None])
    U, S, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    neg = torch.linalg.det(V @ U.transpose(1, 2)) < 0
    one = torch.ones_like(S[:, 0])
    V = V * torch.stack([one, one, torch.where(neg, -one, one)], dim=1)[:, None, :]
    R0 = V @ U.transpose(1, 2)
    T0 = cB - (R0 @ cA[:, :, None])[:, :, 0]
    rank_tol = max(_RANK_TOL, 64 * torch.finfo(dtype).eps)
    status = (neg & (S[:, 2] > rank_tol * S[:, 0])).to(torch.int32) * STATUS_DET_NEGATIVE
    status = status + (~(S[:, 1] >= _UNIQUE_TOL * S[:, 0]) | ~(S[:, 0] > 0)).to(torch.int32) * STATUS_NOT_UNIQUE
    # estimate_translation_k_np with unit weights
    fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    px = 0.5 * img_res * (kp2d_norm + 1)
    F, O = torch.stack([fx, fy], dim=1)[:, None, :], torch.stack([cx, cy], dim=1)[:, None, :]
    c = ((px - O) * kp_cano[:, :, 2:3] - F * kp_cano[:, :, :2]).reshape(B, 2 * NK)
    Q = torch.zeros(B, NK, 2, 3, dtype=dtype, device=dev)
    Q[:, :, 0, 0] = fx[:, None]
    Q[:, :, 1, 1] = fy[:, None]
    Q[:, :, :, 2] = O - px
    Q = Q.reshape(B, 2 * NK, 3)
    A = Q.transpose(1, 2) @ Q
    rhs = (Q.transpose(1, 2) @ c[:, :, None])[:, :, 0]
    singular_tol = max(_SINGULAR_TOL, 64 * torch.finfo(dtype).eps)
    singular = ~(torch.linalg.det(A).abs() > singular_tol * (A[:, 0, 0] * A[:, 1, 1] * A[:, 2, 2]))
    eye = torch.eye(3, dtype=dtype, device=dev)
    t = torch.linalg.solve(torch.where(singular.view(-1, 1, 1), eye[None], A), rhs)
    t = torch.where(singular[:, None], torch.full_like(t, float("nan")), t)
    status = status + singular.to(torch.int32) * STATUS_SINGULAR
    focal = (fx + fy) / 2.0
    out = {"R0": R0, "T0": T0, "transl": t}
    wp = lambda ct: torch.stack([2 * focal / (img_res * ct[:, 2] + 1e-9), ct[:, 0], ct[:, 1]], dim=-1)  # noqa: E731
    offs = {}
    for s, jf, jc in (("r", j_full_r, j_cano_r), ("l", j_full_l, j_cano_l)):
        j0 = (R0 @ jf.transpose(1, 2)).transpose(1, 2) + T0[:, None, :]           # rigid_tf_torch_batch
        offs[s] = (j0 - jc).mean(dim=1) + t
        out["j3d_cam_" + s] = j0 + t[:, None, :]
        out["cam_t_" + s] = out["j3d_cam_" + s][:, 0] - jc[:, 0]
    for s in ("r", "l"):
        out["cam_t_wp_" + s] = wp(out["cam_t_" + s])
    out["cam_t_wp_o"] = wp(t)
    out["off_r"], out["off_l"] = offs["r"], offs["l"]
    out = {k: out[k] for k in FIT_OUTPUTS}
    nan = float("nan")
    out = {k: torch.where(bad.view([-1] + [1] * (v.dim() - 1)), torch.full_like(v, nan), v) for k, v in out.items()}
    status = torch.where(bad, torch.full_like(status, STATUS_NON_FINITE), status)
    return out, status


def _nearest(src, trg, n_trg):
    """Brute force, lowest index on a tie, NaN never wins, candidates below ``n_trg [B]`` only: (squared distance, index)."""
    B, N1, _ = src.shape
    N2 = trg.shape[1]
    chunk = max(1, (1 << 22) // max(1, B * N2))
    ar = torch.arange(N2, device=src.device)
    out_of_reach = (ar[None, :] >= n_trg[:, None])[:, None, :]
    dists, idxs = [], []
    for i0 in range(0, N1, chunk):
        diff = src[:, i0:i0 + chunk, None, :] - trg[:, None, :, :]
        d = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
        d = torch.where(torch.isnan(d) | out_of_reach, torch.full_like(d, float("inf")), d)
        m = d.min(dim=2, keepdim=True).values
        idx = torch.where(d == m, ar, N2).min(dim=2).values
        dists.append(torch.gather(d, 2, idx[..., None])[..., 0])
        idxs.append(idx)
    return torch.cat(dists, 1), torch.cat(idxs, 1)


def distance_fields_reference(hand_r, hand_l, obj, v_len, dist_min=0.0, dist_max=math.inf):
    """``distance_fields`` in torch, in the inputs' dtype."""
    B, L, _ = obj.shape
    NV = hand_r.shape[1]
    vl = v_len.to(obj.device).clamp(0, L)
    full = torch.full_like(vl, NV)
    padded = torch.arange(L, device=obj.device)[None, :] >= vl[:, None]
    empty = (vl == 0)[:, None]
    out = {}
    for s, hand in (("r", hand_r), ("l", hand_l)):
        d, i = _nearest(hand, obj, vl)
        out["dist.%so" % s] = torch.where(empty, torch.zeros_like(d), d.sqrt()).clamp(dist_min, dist_max)
        out["idx.%so" % s] = torch.where(empty, torch.zeros_like(i), i)
        d, i = _nearest(obj, hand, full)
        out["dist.o" + s] = torch.where(padded, torch.zeros_like(d), d.sqrt()).clamp(dist_min, dist_max)
        out["idx.o" + s] = torch.where(padded, torch.zeros_like(i), i)
    return {k: out[k] for k in FIELD_KEYS}


# ---- routing --------------------------------------------------------------------------------------------------------------------
def _why_not(tensors, longs=()):
    """None when these tensors can take a kernel, "" for the two silent causes (CPU data, the knob), else the reason."""
    dev = tensors[0].device
    if dev.type != "cuda" or not _fused_enabled():
        return ""
    if torch.is_autocast_enabled():
        return "autocast is on"
    for t in tensors:
        if t.device != dev or t.dtype != torch.float32:
            return "inputs are not all fp32 on one device (got %s on %s)" % (t.dtype, t.device)
    for t in longs:
        if t.device != dev or t.dtype != torch.int64:
            return "v_len is not int64 on the inputs' device (got %s on %s)" % (t.dtype, t.device)
    return None


def _route(what, why):
    if why is None:
        return True
    if why:
        _warn_restatement(what, why)
    return False


def fit_targets(kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l, img_res=IMG_RES):
    """``(outputs, status)``: see the module's head.  One launch for fp32 CUDA inputs inside ``msda_pre_fit_supported``."""
    ins = [kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l]
    B, NK = kp_full.shape[0], kp_full.shape[1]
    J = j_full_r.shape[1]
    want = [(B, NK, 3), (B, NK, 3), (B, NK, 2), (B, 3, 3)] + [(B, J, 3)] * 4
    if any(tuple(t.shape) != s for t, s in zip(ins, want)):
        raise ValueError("fit_targets: expected keypoints [B, NK, 3], kp2d_norm [B, NK, 2], K [B, 3, 3] and joints [B, J, 3]")
    why = _why_not(ins)
    if why is None and not _native.pre_fit_supported(B, NK, J):
        why = "B = %d, NK = %d, J = %d is outside msda_pre_fit_supported" % (B, NK, J)
    if not _route("fit_targets", why):
        return fit_targets_reference(*ins, img_res=img_res)
    return _native.pre_fit(*[t.detach().contiguous() for t in ins], img_res)


def distance_fields(hand_r, hand_l, obj, v_len, dist_min=0.0, dist_max=math.inf):
    """The four contact fields as a dict with ``FIELD_KEYS``: see the module's head.  One launch for fp32 CUDA inputs inside
    ``msda_dist_fields_supported``."""
    B, NV = hand_r.shape[0], hand_r.shape[1]
    L = obj.shape[1]
    if tuple(hand_r.shape) != (B, NV, 3) or tuple(hand_l.shape) != (B, NV, 3) or tuple(obj.shape) != (B, L, 3) \
            or tuple(v_len.shape) != (B,):
        raise ValueError("distance_fields: expected hands [B, NV, 3], obj [B, L, 3] and v_len [B]")
    if not dist_min <= dist_max:
        raise ValueError("distance_fields: dist_min must not exceed dist_max")
    why = _why_not([hand_r, hand_l, obj], [v_len])
    if why is None and not _native.dist_fields_supported(B, NV, L):
        why = "B = %d, NV = %d, L = %d is outside msda_dist_fields_supported" % (B, NV, L)
    if not _route("distance_fields", why):
        return distance_fields_reference(hand_r, hand_l, obj, v_len, dist_min, dist_max)
    dists, idx = _native.dist_fields(hand_r.detach().contiguous(), hand_l.detach().contiguous(), obj.detach().contiguous(),
                                     v_len.contiguous(), dist_min, dist_max)
    return dict(zip(FIELD_KEYS, dists + idx))


# ---- the step -------------------------------------------------------------------------------------------------------------------
def pre_process(targets, meta_info, models=None, obj_idx=None, max_len=None, field_max=math.inf):
    """``process_data`` + ``arctic_pre_process``'s bookkeeping on the tensors' device: ``(targets, meta_info)``.  ``targets`` is
    written in place, in ``process_data``'s key order.  ``obj_idx`` (int64 device tensor) with a host ``max_len`` replaces
    ``meta_info['query_names']`` for graph capture; both may also travel in ``meta_info`` as they do for ``make_output``."""
    m = _models(models)
    obj = m["arti_head"]
    obj_idx = meta_info.get("obj_idx") if obj_idx is None else obj_idx
    max_len = meta_info.get("max_len") if max_len is None else max_len
    if obj_idx is None:
        obj_idx, max_len = obj.obj_index(meta_info["query_names"])
    elif max_len is None:
        raise ValueError("obj_idx needs a host max_len")
    with torch.no_grad():
        K = meta_info["intrinsics"]
        pose_r, pose_l = targets["mano.pose.r"], targets["mano.pose.l"]
        out = objects_many([(obj, targets["object.radian"].view(-1, 1), targets["object.rot"].view(-1, 3), None, obj_idx,
                             int(max_len))])[0]
        hand_r, hand_l = mano_many([(m["mano_r"], targets["mano.beta.r"], pose_r[:, :3], pose_r[:, 3:]),
                                    (m["mano_l"], targets["mano.beta.l"], pose_l[:, :3], pose_l[:, 3:])])
        nk = out["kp3d"].shape[1] // 2
        fit, status = fit_targets(targets["object.kp3d.full.b"], out["kp3d"][:, nk:], targets["object.kp2d.norm.b"], K,
                                  targets["mano.j3d.full.r"], targets["mano.j3d.full.l"], hand_r.joints, hand_l.joints, IMG_RES)
        placed = place_many([(hand_r.vertices, 0, False), (hand_l.vertices, 1, False), (out["v"], 2, False), (out["kp3d"], 2, False),
                             (out["bbox3d"], 2, False)], [fit["off_r"], fit["off_l"], fit["transl"]], K, IMG_RES, pixels=False)
        v_r, v_l, v_o, kp3d, bbox3d = [p[0] for p in placed]
        fields = distance_fields(v_r, v_l, v_o, out["v_len"], 0.0, field_max)
    meta_info = dict(meta_info)                 # the caller's dict is left as it was
    meta_info["part_ids"] = out["parts_ids"]
    meta_info["diameter"] = out["diameter"]
    for k, v in (("mano.cam_t.r", fit["cam_t_r"]), ("mano.cam_t.l", fit["cam_t_l"]), ("object.cam_t", fit["transl"]),
                 ("mano.cam_t.wp.r", fit["cam_t_wp_r"]), ("mano.cam_t.wp.l", fit["cam_t_wp_l"]), ("object.cam_t.wp", fit["cam_t_wp_o"]),
                 ("object.cam_t.kp3d.b", fit["transl"]), ("mano.v3d.cam.r", v_r), ("mano.v3d.cam.l", v_l),
                 ("mano.j3d.cam.r", fit["j3d_cam_r"]), ("mano.j3d.cam.l", fit["j3d_cam_l"]), ("object.kp3d.cam", kp3d),
                 ("object.bbox3d.cam", bbox3d), ("object.v.cam", v_o), ("object.v_len", out["v_len"]), ("object.f", out["f"]),
                 ("object.f_len", out["f_len"]), ("object.diameter", out["diameter"]), ("object.parts_ids", out["parts_ids"])):
        targets[k] = v
    for k in FIELD_KEYS:
        targets[k] = fields[k]
    meta_info["object.v_len"] = targets["object.v_len"]
    meta_info["mano.faces.r"] = m["mano_r"].faces
    meta_info["mano.faces.l"] = m["mano_l"].faces
    meta_info = XDict(meta_info)
    meta_info.overwrite("part_ids", targets["object.parts_ids"])
    meta_info.overwrite("diameter", targets["object.diameter"])
    meta_info.overwrite("fit_status", status)
    return targets, meta_info


def arctic_pre_process(args, targets, meta_info, models=None, check=False):
    """Drop-in for process.py:72-93 (``args`` is accepted for the signature; the results live with the inputs).  ``models``: the
    ``pre_process_models``-shaped dict, or ``set_default_models`` once.  ``check=True`` reads the fit's status (one sync) and
    raises as ``batch_solve_rigid_tf`` does when a frame's rotation had a negative determinant."""
    targets, meta_info = pre_process(targets, meta_info, models=models)
    if check:
        neg_idx = ((meta_info["fit_status"] & STATUS_DET_NEGATIVE) != 0).cpu()
        if bool(neg_idx.any()):
            raise Exception("some rotation matrices are not orthogonal; make sure implementation is correct for such case: %s"
                            % (neg_idx.numpy(),))
    return targets, meta_info
