"""ARCTIC object layer: a drop-in for arctic_tools/common/object_tensors.py ``ObjectTensors`` on one HIP launch.

``ObjectTensors`` keeps the reference's ``obj_tensors`` dict (the keys ``construct_obj_tensors`` returns, metres) and its
interface: ``forward(angles [B, 1], global_orient [B, 3], transl, query_names)``, ``forward_7d_batch(..., fwd_template)``,
``forward_template(query_names)`` and ``to(dev)``.  The result is a plain dict with the reference's keys in its order
(``diameter``, ``f``, ``f_len``, ``v_len``, ``v``, ``mask``, ``v_sub``, ``parts_ids``, ``parts_sub_ids``, ``bbox3d``, ``kp3d``),
padded to ``max(v_len[obj_idx])`` rows.  ``ObjectTensors.from_reference(m)`` copies a built reference module's ``obj_tensors``,
``ObjectTensors.from_arrays(d)`` builds one from such a dict; neither reads meshes or JSON.

Object indices: ``query_names`` map to indices on the host (``v_len`` is kept on the host too, so the padding needs no sync)
and go up with a pinned ``non_blocking`` copy.  For graph capture, ``obj_idx=`` (an int64 device tensor) with an explicit host
``max_len=`` replaces the names; ``max_len`` has no default because the padded rows change ``v3d_smoothing``.

``objects_many(calls)`` runs several calls as one autograd node: one forward launch writes ``v``, ``v_sub``, ``bbox3d`` and
``kp3d`` of every call and one backward launch gives the ``angles``, ``global_orient`` (and ``transl``) gradients with
fixed-order reductions (``csrc/msda_small_loss.hip``).  The kernels need fp32 CUDA inputs and model tensors that do not
require grad, at most ``OBJECT_MAX_GROUPS`` calls and the model sizes of ``msda_object_supported``; everything else (CPU
tensors, other dtypes, autocast, ``MSDA_OBJECT_FUSED=0``) runs ``object_tensors_reference``, a torch restatement.  With
``MSDA_SMALL_LOSS_BF16=1`` (read at call time, off by default) bf16 autocast alone no longer does: the node calls the C ABI on
its fp32 inputs and returns the bits it returns outside the region; fp16 autocast keeps the restatement.

Kept from the reference: ``transl`` is added in metres (its ``*1000`` in ``_sanity_check`` changes only a local variable);
articulation is ``q p q*`` about -z with ``q`` from pytorch3d's ``axis_angle_to_quaternion`` (the ``|theta| < 1e-6`` series),
not renormalised; an unknown name raises ``ValueError`` (the reference's ``list.index``).  An out-of-range ``obj_idx`` gives NaN
rows on the kernel path (the reference would raise; checking would need a sync); the template entries of such a frame are those
of the nearest valid index."""
import os

import numpy as np
import torch
from torch import nn

from . import _native
from ._autocast import autocast_refuses

OBJECT_MAX_GROUPS = _native.OBJECT_MAX_GROUPS
OUTPUT_KEYS = ("diameter", "f", "f_len", "v_len", "v", "mask", "v_sub", "parts_ids", "parts_sub_ids", "bbox3d", "kp3d")
TEMPLATE_KEYS = OUTPUT_KEYS[:9]
_MODEL_KEYS = ("v", "parts_ids", "v_sub", "parts_sub_ids", "bbox_top", "bbox_bottom", "kp_top", "kp_bottom")


# ---- torch restatement ----------------------------------------------------------------------------------------------------------
def axis_angle_to_quaternion(axis_angle):
    """pytorch3d's conversion: (cos(theta/2), a sin(theta/2)/theta), with 1/2 - theta^2/48 for theta < 1e-6."""
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    half = angles * 0.5
    small = angles.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angles), angles)
    s = torch.where(small, 0.5 - angles * angles / 48, torch.sin(half) / safe)
    return torch.cat([torch.cos(half), axis_angle * s], dim=-1)


def quaternion_raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def quaternion_apply(q, p):
    """Im(q (0, p) q*)."""
    pq = torch.cat((p.new_zeros(p.shape[:-1] + (1,)), p), -1)
    conj = q * q.new_tensor([1, -1, -1, -1])
    return quaternion_raw_multiply(quaternion_raw_multiply(q, pq), conj)[..., 1:]


def quaternion_to_matrix(q):
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def axis_angle_to_matrix(axis_angle):
    """pytorch3d's axis_angle_to_matrix: quaternion_to_matrix . axis_angle_to_quaternion."""
    return quaternion_to_matrix(axis_angle_to_quaternion(axis_angle))


def _template(ot, obj_idx, max_len):
    out = {}
    out["diameter"] = ot["diameter"][obj_idx]
    out["f"] = ot["f"][obj_idx]
    out["f_len"] = ot["f_len"][obj_idx]
    out["v_len"] = ot["v_len"][obj_idx]
    out["v"] = ot["v"][obj_idx][:, :max_len]
    out["mask"] = ot["mask"][obj_idx][:, :max_len]
    out["v_sub"] = ot["v_sub"][obj_idx]
    out["parts_ids"] = ot["parts_ids"][obj_idx][:, :max_len]
    out["parts_sub_ids"] = ot["parts_sub_ids"][obj_idx]
    return out


def object_tensors_reference(ot, angles, global_orient, transl, obj_idx, max_len):
    """forward_7d_batch (fwd_template=False) restated in torch, any dtype: the output dict."""
    out = _template(ot, obj_idx, max_len)
    dtype = global_orient.dtype
    z_axis = ot["z_axis"].to(dtype)
    quat_arti = axis_angle_to_quaternion(z_axis * angles)
    quat_global = axis_angle_to_quaternion(global_orient.view(-1, 3))
    cast = lambda t: t.to(dtype)  # noqa: E731
    tf = {"v_top": cast(out["v"]), "v_sub_top": cast(out["v_sub"]), "v_bottom": cast(out["v"]),
          "v_sub_bottom": cast(out["v_sub"]), "bbox_top": cast(ot["bbox_top"][obj_idx]),
          "bbox_bottom": cast(ot["bbox_bottom"][obj_idx]), "kp_top": cast(ot["kp_top"][obj_idx]),
          "kp_bottom": cast(ot["kp_bottom"][obj_idx])}
    for key in tf:
        if "top" in key:
            tf[key] = quaternion_apply(quat_arti[:, None, :], tf[key])
    for key in tf:
        val = quaternion_apply(quat_global[:, None, :], tf[key])
        tf[key] = val + transl[:, None, :] if transl is not None else val
    top = (out["parts_ids"] == 1).unsqueeze(-1)
    out["v"] = torch.where(top, tf["v_top"], tf["v_bottom"])
    top = (out["parts_sub_ids"] == 1).unsqueeze(-1)
    out["v_sub"] = torch.where(top, tf["v_sub_top"], tf["v_sub_bottom"])
    out["bbox3d"] = torch.cat((tf["bbox_top"], tf["bbox_bottom"]), dim=1)
    out["kp3d"] = torch.cat((tf["kp_top"], tf["kp_bottom"]), dim=1)
    return out


# ---- the HIP node ---------------------------------------------------------------------------------------------------------------
def _fused_enabled():
    return os.environ.get("MSDA_OBJECT_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatement


class _ObjectFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *flat):
        ctx.set_materialize_grads(False)
        dims, model, lens = meta
        inputs = [tuple(flat[4 * i:4 * i + 4]) for i in range(len(lens))]
        outs = _native.object_forward(dims, model, inputs, lens)
        ctx.meta = meta
        ctx.has_transl = [grp[3] is not None for grp in inputs]
        ctx.save_for_backward(*[t for grp in inputs for t in grp if t is not None])
        return tuple(t for grp in outs for t in grp)

    @staticmethod
    def backward(ctx, *grads):
        dims, model, lens = ctx.meta
        saved = list(ctx.saved_tensors)
        inputs = []
        for has_t in ctx.has_transl:
            grp, saved = saved[:3 + has_t], saved[3 + has_t:]
            inputs.append(tuple(grp) + ((None,) if not has_t else ()))
        gouts = [tuple(None if g is None else g.contiguous() for g in grads[4 * i:4 * i + 4]) for i in range(len(inputs))]
        gin = _native.object_backward(dims, model, inputs, lens, gouts, ctx.has_transl)
        res = []
        for ga, ggo, gtr in gin:
            res += [None, ga, ggo, gtr]
        return (None,) + tuple(r if need else None for r, need in zip(res, ctx.needs_input_grad[1:]))


def _fused_plan(calls):
    """(dims, model, lens, inputs) for the kernels, or None where the restatement runs."""
    if not (_fused_enabled() and calls) or autocast_refuses() or len(calls) > OBJECT_MAX_GROUPS:
        return None
    layer = calls[0][0]
    if any(c[0] is not layer for c in calls):
        return None
    dev = calls[0][2].device
    model = layer._kernel_model()
    if dev.type != "cuda" or model is None or any(t.device != dev for t in model):
        return None
    dims = layer._dims()
    if not _native.object_supported(*dims):
        return None
    inputs, lens = [], []
    for _, angles, go, transl, idx, max_len in calls:
        B = go.shape[0]
        ts = [t for t in (angles, go, transl) if t is not None]
        if any(t.device != dev or t.dtype != torch.float32 for t in ts) or idx.device != dev or max_len > dims[1]:
            return None
        if angles.numel() != B or go.shape != (B, 3) or (transl is not None and transl.shape != (B, 3)) or idx.numel() != B:
            return None
        inputs.append((idx.reshape(-1).contiguous(), angles.reshape(-1).contiguous(), go.contiguous(),
                       None if transl is None else transl.contiguous()))
        lens.append(int(max_len))
    return dims, model, lens, inputs


def objects_many(calls):
    """Every call ``(layer, angles [B, 1], global_orient [B, 3], transl or None, obj_idx [B] int64, max_len)`` as one node;
    returns one output dict per call."""
    plan = _fused_plan(calls)
    if plan is None:
        return [object_tensors_reference(c[0].obj_tensors, c[1], c[2], c[3], c[4], c[5]) for c in calls]
    dims, model, lens, inputs = plan
    flat = [t for grp in inputs for t in grp]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in flat):
        outs = _ObjectFunction.apply((dims, model, lens), *flat)
        outs = [tuple(outs[4 * i:4 * i + 4]) for i in range(len(inputs))]
    else:
        outs = _native.object_forward(dims, model, inputs, lens)
    res = []
    for (layer, _, _, _, idx, max_len), (v, v_sub, bbox, kp) in zip(calls, outs):
        # an out-of-range index has NaN rows from the kernel; the template gather must not read outside the model for it
        out = _template(layer.obj_tensors, idx.clamp(0, dims[0] - 1), max_len)
        out["v"], out["v_sub"], out["bbox3d"], out["kp3d"] = v, v_sub, bbox, kp
        res.append(out)
    return res


class ObjectTensors(nn.Module):
    """Drop-in for arctic_tools ``ObjectTensors``; ``obj_tensors`` is the reference's dict (``names`` a list of str)."""

    def __init__(self, obj_tensors):
        super().__init__()
        ot = {}
        for k, v in obj_tensors.items():
            ot[k] = list(v) if k == "names" else (v.detach().clone() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)))
        self.obj_tensors = ot
        self.dev = None
        self._names = {n: i for i, n in enumerate(ot["names"])}
        self._v_len = [int(x) for x in ot["v_len"].cpu().tolist()]
        self._kmodel = None

    @classmethod
    def from_arrays(cls, obj_tensors):
        """From tensors with ``construct_obj_tensors``'s keys and units (metres)."""
        return cls(obj_tensors)

    @classmethod
    def from_reference(cls, module):
        """Copy a built reference module's ``obj_tensors`` (on its current device)."""
        layer = cls(module.obj_tensors)
        layer.dev = getattr(module, "dev", None)
        return layer

    def to(self, dev):
        self.obj_tensors = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in self.obj_tensors.items()}
        self.dev = dev
        self._kmodel = None
        return self

    def _dims(self):
        ot = self.obj_tensors
        return (ot["v"].shape[0], ot["v"].shape[1], ot["v_sub"].shape[1], ot["bbox_top"].shape[1],
                ot["bbox_bottom"].shape[1], ot["kp_top"].shape[1], ot["kp_bottom"].shape[1])

    def _kernel_model(self):
        """The 8 model tensors in msda.h's order (fp32 / int64 contiguous), or None when the kernels cannot take them."""
        ot = self.obj_tensors
        ts = [ot[k] for k in _MODEL_KEYS]
        if not all(t.is_cuda for t in ts) or any(t.requires_grad for t in ts):
            return None
        if self._kmodel is None or self._kmodel[0].device != ts[0].device:
            self._kmodel = [t.to(torch.int64 if "parts" in k else torch.float32).contiguous() for k, t in zip(_MODEL_KEYS, ts)]
        return self._kmodel

    def obj_index(self, query_names):
        """(obj_idx int64 tensor on the model's device, host max_len) for host names, without a sync."""
        try:
            idx = [self._names[n] for n in query_names]
        except KeyError as e:
            raise ValueError("%r is not in list" % e.args[0]) from None
        host = torch.tensor(idx, dtype=torch.int64)
        dev = self.obj_tensors["v"].device
        if dev.type == "cuda":
            host = host.pin_memory().to(dev, non_blocking=True)
        return host, max(self._v_len[i] for i in idx)

    def _resolve(self, query_names, obj_idx, max_len):
        if obj_idx is None:
            return self.obj_index(query_names)
        if max_len is None:
            raise ValueError("obj_idx needs an explicit host max_len (the padded rows change v3d_smoothing)")
        return obj_idx, int(max_len)

    def forward_7d_batch(self, angles, global_orient, transl, query_names, fwd_template, obj_idx=None, max_len=None):
        obj_idx, max_len = self._resolve(query_names, obj_idx, max_len)
        if fwd_template:
            return _template(self.obj_tensors, obj_idx, max_len)
        B = angles.shape[0]
        assert angles.shape == (B, 1) and global_orient.shape == (B, 3)
        assert transl is None or (torch.is_tensor(transl) and transl.shape == (B, 3))
        assert query_names is None or len(query_names) == B
        return objects_many([(self, angles, global_orient, transl, obj_idx, max_len)])[0]

    def forward(self, angles, global_orient, transl, query_names, obj_idx=None, max_len=None):
        return self.forward_7d_batch(angles, global_orient, transl, query_names, fwd_template=False, obj_idx=obj_idx,
                                     max_len=max_len)

    def forward_template(self, query_names, obj_idx=None, max_len=None):
        return self.forward_7d_batch(None, None, None, query_names, fwd_template=True, obj_idx=obj_idx, max_len=max_len)
