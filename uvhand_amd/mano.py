"""MANO hand layer: a drop-in for smplx's ``MANO(use_pca=False)`` as ARCTIC builds it (``build_mano_aa``), on one HIP launch.

``MANO`` keeps smplx's model tensors under their names (``v_template``, ``shapedirs``, ``posedirs``, ``J_regressor``,
``lbs_weights``, ``parents``, ``pose_mean``, ``faces_tensor``, ``extra_joints_idxs``) and its forward signature; absent arguments
fall back to the module's own ``betas`` / ``global_orient`` / ``hand_pose`` / ``transl`` parameters.  ``MANO.from_smplx(m)``
copies a constructed smplx module, ``MANO.from_arrays(...)`` builds one from plain tensors.

``mano_many(calls)`` runs several ``(layer, betas, global_orient, hand_pose[, transl])`` calls as one autograd node: one
forward launch and two backward launches (``csrc/msda_mano.hip``) for all of them, mixed layers and batch sizes included, with
no host synchronisation; the node captures in a graph.  The kernels need fp32 CUDA tensors, model tensors that do not require
grad, at most ``MANO_MAX_GROUPS`` calls over at most ``MANO_MAX_LAYERS`` layers.  Everything else runs ``mano_reference``, a
torch restatement of smplx's MANO forward and ``lbs`` in any dtype: CPU tensors, non-fp32 inputs, autocast, model tensors
that require grad, anything over the limits, and ``MSDA_MANO_FUSED=0`` (A/B knob).  With ``MSDA_SMALL_LOSS_BF16=1`` (read at
call time, off by default) bf16 autocast alone no longer does: the node calls the C ABI on its fp32 inputs, so it returns the
bits it returns outside the region.  fp16 autocast keeps the restatement."""
import os

import numpy as np
import torch
from torch import nn

from . import _native
from ._autocast import autocast_refuses

MANO_MAX_GROUPS = _native.MANO_MAX_GROUPS       # calls per mano_many node; more run the restatement
MANO_MAX_LAYERS = _native.MANO_MAX_LAYERS       # distinct layers per node
NUM_JOINTS = 16


class ManoOutput:
    """smplx's MANOOutput fields: vertices, joints, betas, global_orient, hand_pose, full_pose (and transl)."""
    _fields = ("vertices", "joints", "betas", "global_orient", "hand_pose", "full_pose", "transl")

    def __init__(self, **kw):
        for k in self._fields:
            setattr(self, k, kw.get(k))

    def __getitem__(self, key):
        return getattr(self, key)

    def keys(self):
        return [k for k in self._fields if getattr(self, k) is not None]

    def items(self):
        return [(k, getattr(self, k)) for k in self.keys()]


# ---- torch restatement of smplx's lbs ------------------------------------------------------------------------------------------
def batch_rodrigues_reference(rot_vecs):
    """[N, 3] axis-angles -> [N, 3, 3]: angle = |r + 1e-8|, R = I + sin K + (1 - cos) K^2 with K the cross matrix of r / angle."""
    angle = torch.norm(rot_vecs + 1e-8, dim=1, keepdim=True)
    x, y, z = (rot_vecs / angle).unbind(1)
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], dim=1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device)
    s = torch.sin(angle).unsqueeze(-1)
    c = torch.cos(angle).unsqueeze(-1)
    return eye + s * K + (1 - c) * torch.bmm(K, K)


def lbs_reference(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights):
    """Linear blend skinning as smplx's ``lbs`` (pose as axis-angles [B, 3 J]).  Returns (vertices [B, V, 3], posed joints
    [B, J, 3]).  ``parents``: a sequence of ints (parents[0] = -1); ``betas`` with batch 1 is broadcast over the pose batch."""
    B = max(betas.shape[0], pose.shape[0])
    dtype = pose.dtype
    v_shaped = v_template + torch.einsum("bl,vcl->bvc", betas, shapedirs)
    J = torch.einsum("jv,bvc->bjc", J_regressor, v_shaped)
    if v_shaped.shape[0] != B:
        v_shaped, J = v_shaped.expand(B, -1, -1), J.expand(B, -1, -1)
    nj = J.shape[1]
    R = batch_rodrigues_reference(pose.reshape(-1, 3)).view(B, nj, 3, 3)
    eye = torch.eye(3, dtype=dtype, device=pose.device)
    pose_feature = (R[:, 1:] - eye).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, posedirs).view(B, -1, 3)
    parents = [int(p) for p in parents]
    rel = torch.cat([J[:, :1], J[:, 1:] - J[:, parents[1:]]], dim=1)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=dtype, device=pose.device).expand(B, nj, 1, 4)
    local = torch.cat([torch.cat([R, rel.unsqueeze(-1)], dim=-1), bottom], dim=-2)          # [B, J, 4, 4]
    chain = [local[:, 0]]
    for i in range(1, nj):
        chain.append(torch.matmul(chain[parents[i]], local[:, i]))
    G = torch.stack(chain, dim=1)
    posed_joints = G[:, :, :3, 3]
    rot = G[:, :, :3, :3]
    A = torch.cat([rot, (posed_joints - torch.matmul(rot, J.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1)], dim=-1)   # [B, J, 3, 4]
    T = torch.einsum("vj,bjrc->bvrc", lbs_weights, A)
    verts = torch.matmul(T[..., :3], v_posed.unsqueeze(-1)).squeeze(-1) + T[..., 3]
    return verts, posed_joints


def _batch(*tensors):
    return max(t.shape[0] for t in tensors if t is not None)


def _expand(t, B):
    return t if t is None or t.shape[0] == B else t.expand(B, -1)


def mano_reference(layer, betas, global_orient, hand_pose, transl=None):
    """smplx's MANO forward (use_pca=False) in torch: (vertices [B, V, 3], joints [B, 16 + E, 3], full_pose [B, 48])."""
    B = _batch(betas, global_orient, hand_pose, transl)
    dtype = hand_pose.dtype
    full_pose = torch.cat([_expand(global_orient, B), _expand(hand_pose, B)], dim=1) + layer.pose_mean.to(dtype)
    cast = [t.to(dtype) for t in (layer.v_template, layer.shapedirs, layer.posedirs, layer.J_regressor)]
    verts, joints = lbs_reference(betas.to(dtype), full_pose, *cast, layer._parents, layer.lbs_weights.to(dtype))
    joints = torch.cat([joints, verts[:, layer._extra]], dim=1)
    if transl is not None:
        t = _expand(transl, B).unsqueeze(1)
        joints, verts = joints + t, verts + t
    return verts, joints, full_pose


# ---- the HIP node ---------------------------------------------------------------------------------------------------------------
def _fused_enabled():
    return os.environ.get("MSDA_MANO_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatement


def _layer_ok(layer, dev):
    ts = layer._kernel_tensors()
    return all(t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in ts) \
        and not any(t.requires_grad for t in (layer.v_template, layer.shapedirs, layer.posedirs, layer.J_regressor))


def _fused_plan(calls):
    """(dims, layers, group_layer, group_bcast, inputs) for the kernels, or None where the restatement runs."""
    if not (_fused_enabled() and calls) or autocast_refuses() or len(calls) > MANO_MAX_GROUPS:
        return None
    layers = []
    for c in calls:
        if not any(c[0] is l for l in layers):
            layers.append(c[0])
    if len(layers) > MANO_MAX_LAYERS:
        return None
    dev = calls[0][3].device
    if not dev.type == "cuda" or not all(_layer_ok(l, dev) for l in layers):
        return None
    dims = layers[0]._dims()
    if any(l._dims() != dims for l in layers) or not _native.mano_supported(*dims):
        return None
    group_layer, group_bcast, inputs = [], [], []
    for layer, betas, go, hp, transl in calls:
        ts = [t for t in (betas, go, hp, transl) if t is not None]
        if any(not t.is_cuda or t.device != dev or t.dtype != torch.float32 or t.dim() != 2 for t in ts):
            return None
        if betas.shape[1] != dims[1] or go.shape[1] != 3 or hp.shape[1] != 45 or (transl is not None and transl.shape[1] != 3):
            return None
        B = _batch(betas, go, hp, transl)
        if any(t.shape[0] not in (1, B) for t in ts):
            return None
        group_layer.append(next(i for i, l in enumerate(layers) if l is layer))
        group_bcast.append(int(betas.shape[0] != B))
        inputs.append((betas.contiguous(), _expand(go, B).contiguous(), _expand(hp, B).contiguous(),
                       None if transl is None else _expand(transl, B).contiguous()))
    return dims, layers, group_layer, group_bcast, inputs


def _kernel_layers(layers):
    return [(l._kernel_tensors(), l._index) for l in layers]


class _ManoFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *flat):
        ctx.set_materialize_grads(False)
        dims, layers, group_layer, group_bcast = meta
        inputs = [tuple(flat[4 * i:4 * i + 4]) for i in range(len(group_layer))]
        outs = _native.mano_forward(dims, _kernel_layers(layers), group_layer, group_bcast, inputs)
        ctx.meta = meta
        ctx.has_transl = [grp[3] is not None for grp in inputs]
        ctx.save_for_backward(*[t for grp in inputs for t in grp if t is not None])
        return tuple(t for pair in outs for t in pair)

    @staticmethod
    def backward(ctx, *grads):
        dims, layers, group_layer, group_bcast = ctx.meta
        saved = list(ctx.saved_tensors)
        inputs = []
        for has_t in ctx.has_transl:
            grp, saved = saved[:3 + has_t], saved[3 + has_t:]
            inputs.append(tuple(grp) + ((None,) if not has_t else ()))
        gouts = [tuple(None if g is None else g.contiguous() for g in grads[2 * i:2 * i + 2]) for i in range(len(inputs))]
        gin = _native.mano_backward(dims, _kernel_layers(layers), group_layer, group_bcast, inputs, gouts)
        res = []
        for (gb, ggo, ghp, gtr), bc in zip(gin, group_bcast):
            res += [gb.sum(0, keepdim=True) if bc else gb, ggo, ghp, gtr]
        return (None,) + tuple(r if need else None for r, need in zip(res, ctx.needs_input_grad[1:]))


def _resolve(call):
    layer, betas, go, hp = call[:4]
    transl = call[4] if len(call) > 4 else None
    betas = layer.betas if betas is None else betas
    go = layer.global_orient if go is None else go
    hp = layer.hand_pose if hp is None else hp
    if transl is None and getattr(layer, "transl", None) is not None:
        transl = layer.transl
    return layer, betas, go, hp, transl


def _run(calls):
    """[(vertices, joints, full_pose or None)] per resolved call."""
    plan = _fused_plan(calls)
    if plan is None:
        return [mano_reference(*c) for c in calls]
    dims, layers, group_layer, group_bcast, inputs = plan
    meta = (dims, layers, group_layer, group_bcast)
    flat = [t for grp in inputs for t in grp]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in flat):
        outs = _ManoFunction.apply(meta, *flat)
        outs = [(outs[2 * i], outs[2 * i + 1]) for i in range(len(inputs))]
    else:
        outs = _native.mano_forward(dims, _kernel_layers(layers), group_layer, group_bcast, inputs)
    return [(v, j, None) for v, j in outs]


def mano_many(calls, return_full_pose=False):
    """Every call ``(layer, betas, global_orient, hand_pose[, transl])`` (None: the layer's own parameter) as one node; returns
    one ``ManoOutput`` per call."""
    calls = [_resolve(c) for c in calls]
    res = []
    for (layer, betas, go, hp, transl), (v, j, fp) in zip(calls, _run(calls)):
        if fp is None and return_full_pose:
            B = _batch(betas, go, hp, transl)
            fp = torch.cat([_expand(go, B), _expand(hp, B)], dim=1) + layer.pose_mean.to(hp.dtype)
        res.append(ManoOutput(vertices=v, joints=j, betas=betas, global_orient=go, hand_pose=hp,
                              full_pose=fp if return_full_pose else None, transl=transl))
    return res


def _fold(J_regressor, v_template, shapedirs):
    """J_regressor folded into the template and the shape directions (fp64, then the model dtype)."""
    Jr = J_regressor.double()
    jt = (Jr @ v_template.double()).to(v_template.dtype)
    jsd = torch.einsum("jv,vcl->jcl", Jr, shapedirs.double()).to(shapedirs.dtype)
    return jt.contiguous(), jsd.contiguous()


class MANO(nn.Module):
    """Drop-in for smplx's ``MANO(use_pca=False)``.  Model tensors are fixed once the layer is built (``J_regressor`` is folded
    into ``J_template`` / ``J_shapedirs`` then; call ``refold()`` after changing any of them in place)."""

    NUM_HAND_JOINTS = 15

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, lbs_weights, parents, pose_mean, faces, extra_joints_idxs,
                 betas=None, global_orient=None, hand_pose=None, transl=None, is_rhand=True, flat_hand_mean=False):
        super().__init__()
        f32 = dict(dtype=torch.float32)
        as_t = lambda t, **kw: torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t, **kw).detach().clone()  # noqa: E731
        self.register_buffer("v_template", as_t(v_template, **f32).contiguous())
        self.register_buffer("shapedirs", as_t(shapedirs, **f32).contiguous())
        self.register_buffer("posedirs", as_t(posedirs, **f32).contiguous())
        self.register_buffer("J_regressor", as_t(J_regressor, **f32).contiguous())
        self.register_buffer("lbs_weights", as_t(lbs_weights, **f32).contiguous())
        self.register_buffer("parents", as_t(parents, dtype=torch.long))
        self.register_buffer("pose_mean", as_t(pose_mean, **f32).reshape(-1).contiguous())
        self.register_buffer("faces_tensor", as_t(faces, dtype=torch.long))
        self.register_buffer("extra_joints_idxs", as_t(extra_joints_idxs, dtype=torch.long).reshape(-1))
        self.faces = self.faces_tensor.cpu().numpy()
        self._parents = [int(p) for p in self.parents.cpu().tolist()]
        self._extra = [int(i) for i in self.extra_joints_idxs.cpu().tolist()]
        self._index = self._parents + self._extra
        self.num_betas = self.shapedirs.shape[-1]
        self.is_rhand = bool(is_rhand)
        self.flat_hand_mean = bool(flat_hand_mean)
        self.use_pca = False
        nb = self.num_betas

        def param(t, shape):
            return nn.Parameter(torch.zeros(*shape) if t is None else as_t(t, **f32).reshape(-1, shape[1]))
        self.betas = param(betas, (1, nb))
        self.global_orient = param(global_orient, (1, 3))
        self.hand_pose = param(hand_pose, (1, 45))
        if transl is not None:
            self.transl = param(transl, (1, 3))
        else:
            self.transl = None
        jt, jsd = _fold(self.J_regressor, self.v_template, self.shapedirs)
        self.register_buffer("J_template", jt, persistent=False)
        self.register_buffer("J_shapedirs", jsd, persistent=False)

    @property
    def hand_mean(self):
        return self.pose_mean[3:]

    def refold(self):
        jt, jsd = _fold(self.J_regressor, self.v_template, self.shapedirs)
        self.J_template.data = jt.to(self.J_template.device)
        self.J_shapedirs.data = jsd.to(self.J_shapedirs.device)

    def _dims(self):
        return (self.v_template.shape[0], self.num_betas, len(self._extra))

    def _kernel_tensors(self):
        return (self.v_template, self.shapedirs, self.posedirs, self.J_template, self.J_shapedirs, self.lbs_weights,
                self.pose_mean)

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, J_regressor, lbs_weights, parents, pose_mean, faces,
                    extra_joints_idxs, **kw):
        """Build from plain tensors in smplx's layouts: posedirs [135, 3 V], pose_mean [48] (zeros for the global orient, then
        hand_mean)."""
        return cls(v_template, shapedirs, posedirs, J_regressor, lbs_weights, parents, pose_mean, faces, extra_joints_idxs, **kw)

    @classmethod
    def from_smplx(cls, module):
        """Copy a constructed smplx MANO module by attribute name (its parameters' current values included)."""
        g = lambda name: getattr(module, name, None)  # noqa: E731
        transl = g("transl")
        layer = cls(module.v_template, module.shapedirs, module.posedirs, module.J_regressor, module.lbs_weights,
                    module.parents, module.pose_mean, module.faces_tensor, module.vertex_joint_selector.extra_joints_idxs,
                    betas=g("betas"), global_orient=g("global_orient"), hand_pose=g("hand_pose"), transl=transl,
                    is_rhand=bool(g("is_rhand") if g("is_rhand") is not None else True),
                    flat_hand_mean=bool(g("flat_hand_mean") or False))
        return layer.to(module.v_template.device)

    def name(self):
        return "MANO"

    def forward(self, betas=None, global_orient=None, hand_pose=None, transl=None, return_verts=True, return_full_pose=False,
                **kwargs):
        out = mano_many([(self, betas, global_orient, hand_pose, transl)], return_full_pose=return_full_pose)[0]
        if not return_verts:
            out.vertices = None
        return out
