"""The DeformableDETR prediction heads (models/actic_detr.py:245-287, models/assembly_detr.py:172-210) as one autograd node.

``detr_heads`` evaluates, for every decoder level of ``hs [L, B, Q, C]``, the class Linear, the 3-layer keypoint MLPs with
their reference epilogue and (ARCTIC) the six shared pose / shape / camera Linears, and returns the reference's
``torch.stack``-ed tensors.  On CUDA fp32 it is ``_DetrHeadsFunction``: three forward launches and five backward launches
(``csrc/msda_heads.hip``) over every head of every level, with no host synchronisation.  Everything else runs
``detr_heads_reference``, a torch restatement of the reference's composition: CPU tensors, autocast (the reference
under ``--amp``: logits go ``.to(float32)`` for ARCTIC, the rest stays bf16), hidden sizes the kernels do not take,
references that require grad, heads whose levels share some modules but not all, and ``MSDA_HEADS_FUSED=0`` (A/B knob).

``MSDA_HEADS_BF16=1`` (read at call time, off by default) sends bf16 autocast over fp32 ``hs``, parameters and references
to the same node on the bf16 MFMA (``csrc/msda_heads_bf16.hip``): the same launch counts, the composition's output dtypes and
forward roundings, hidden activations saved as bf16, ``hs`` and the weights rounded in the kernels' own loads (no cast
kernels), and fp32 ``grad_hs`` / parameter gradients that are not rounded to bf16 on the way.  fp16 autocast, bf16 ``hs``
and hidden sizes with ``C % 8 != 0`` keep the composition."""
import os

import torch

from .. import _native
from .linear_func import _autocast_dtype

ARCTIC, ASSEMBLY = "arctic", "assembly"
_KIND = {ARCTIC: _native.HEADS_ARCTIC, ASSEMBLY: _native.HEADS_ASSEMBLY}
MAX_LEVELS = 8


def inverse_sigmoid(x, eps=1e-5):
    """util/misc.py:614-618."""
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


def _mlp(mlp, x):
    """MLP.forward (models/actic_detr.py:580-583): ReLU after every layer but the last."""
    n = len(mlp.layers)
    for i, layer in enumerate(mlp.layers):
        x = torch.relu(layer(x)) if i < n - 1 else layer(x)
    return x


def _reference(kind, lvl, init_reference, inter_references):
    if lvl == 0:
        return inverse_sigmoid(init_reference)
    ref = inter_references[lvl - 1]
    return inverse_sigmoid(ref) if kind == ARCTIC else inverse_sigmoid((ref + 0.5) / 2)


def detr_heads_reference(kind, hs, init_reference, inter_references, cls_embed, mlps, shared=None):
    """The reference's per-level composition and stacks; same arguments and results as ``detr_heads``."""
    levels = hs.shape[0]
    classes, keys, outs = [], [[] for _ in mlps], [[] for _ in (shared or ())]
    for lvl in range(levels):
        hs_lvl = hs[lvl]
        if mlps:
            reference = _reference(kind, lvl, init_reference, inter_references)
        if kind == ARCTIC:
            for h, mlp in enumerate(mlps):
                keys[h].append((_mlp(mlp[lvl], hs_lvl) + reference).sigmoid() * 2 - 1)
            classes.append(cls_embed[lvl](hs_lvl).to(torch.float32))
            for g, lin in enumerate(shared or ()):
                outs[g].append(lin(hs_lvl))
        else:
            classes.append(cls_embed[lvl](hs_lvl))
            key = _mlp(mlps[0][lvl], hs_lvl)
            if reference.shape[-1] == 42:
                ref_x = reference[..., 0::2].mean(-1).unsqueeze(-1)
                ref_y = reference[..., 1::2].mean(-1).unsqueeze(-1)
                key = key.reshape(key.shape[0], key.shape[1], 21, 3)
                key[..., :2] += torch.cat([ref_x, ref_y], dim=-1)[:, :, None, :]
            else:
                assert reference.shape[-1] == 2
                key = key.reshape(key.shape[0], key.shape[1], 21, 3)
                key[..., :2] += reference[:, :, None, :]
            key = key.reshape(key.shape[0], key.shape[1], -1)
            keys[0].append(key.sigmoid() * 2 - 0.5)
    return torch.stack(classes), [torch.stack(k) for k in keys], [torch.stack(o) for o in outs]


def _fused_enabled():
    return os.environ.get("MSDA_HEADS_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatement


def _bf16_enabled():
    return os.environ.get("MSDA_HEADS_BF16", "0") not in ("", "0")     # opt-in: the node under bf16 autocast


def _levels(mods, L):
    """([modules], shared) for levels < L: one module repeated, or L distinct ones; None for anything in between."""
    mods = list(mods)[:L]
    if all(m is mods[0] for m in mods):
        return mods[:1], True
    if len({id(m) for m in mods}) == L:
        return mods, False
    return None


def _fused_plan(kind, hs, init_reference, inter_references, cls_embed, mlps, shared):
    """The kernels' operands, or None where the composition runs."""
    if not (_fused_enabled() and hs.is_cuda and hs.dtype == torch.float32 and hs.dim() == 4):
        return None
    bf16 = torch.is_autocast_enabled()
    if bf16 and not (_bf16_enabled() and _autocast_dtype() == torch.bfloat16):
        return None
    if not (_native.heads_bf16_supported(hs.shape[-1]) if bf16 else _native.heads_supported(hs.shape[-1])):
        return None
    L = hs.shape[0]
    if not 1 <= L <= MAX_LEVELS or (kind == ARCTIC and len(mlps) not in (0, 2)) or (kind == ASSEMBLY and len(mlps) != 1):
        return None
    if kind == ARCTIC and (shared is None or len(shared) != 6):
        return None
    refs = [t for t in (init_reference, inter_references if L > 1 else None) if t is not None] if mlps else []
    if mlps and (init_reference is None or (L > 1 and inter_references is None)):
        return None
    if any(r.requires_grad or not r.is_cuda or r.dtype != torch.float32 for r in refs):
        return None
    cls = _levels(cls_embed, L)
    heads = [_levels(m, L) for m in mlps]
    if cls is None or any(h is None for h in heads) or len({h[1] for h in heads}) > 1:
        return None
    flags = (_native.HEADS_SHARED_CLS if cls[1] else 0) | (_native.HEADS_SHARED_MLP if heads and heads[0][1] else 0)
    cls_w = [m.weight for m in cls[0]]
    cls_b = [m.bias for m in cls[0]]
    mlp_w, mlp_b = [], []
    for mods, _ in heads:
        for layer in range(3):
            for m in mods:
                if len(m.layers) != 3:
                    return None
                mlp_w.append(m.layers[layer].weight)
                mlp_b.append(m.layers[layer].bias)
    sh_w = [m.weight for m in shared] if kind == ARCTIC else []
    sh_b = [m.bias for m in shared] if kind == ARCTIC else []
    params = cls_w + cls_b + mlp_w + mlp_b + sh_w + sh_b
    if any(p is None or not p.is_cuda or p.dtype != torch.float32 or p.device != hs.device for p in params):
        return None
    if mlps:
        B, Q = hs.shape[1:3]
        R = init_reference.shape[-1]
        if tuple(init_reference.shape) != (B, Q, R) or (L > 1 and (inter_references.shape[0] < L - 1
                                                                    or tuple(inter_references.shape[1:]) != (B, Q, R))):
            return None
        if R not in ((42,) if kind == ARCTIC else (2, 42)):
            return None
    meta = (_KIND[kind], flags, len(cls_w), len(mlp_w), len(sh_w), bf16)
    return meta, params


class _DetrHeadsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, hs, init_ref, inter_ref, *params):
        kind, flags, n_cls, n_mlp, n_sh, bf16 = meta
        L, B, Q, C = hs.shape
        hs3 = hs.contiguous().view(L, B * Q, C)
        init3 = init_ref.contiguous() if init_ref is not None else None
        inter3 = inter_ref[:L - 1].contiguous() if inter_ref is not None and L > 1 else None
        groups = _split(params, n_cls, n_mlp, n_sh)
        run = _native.heads_forward_bf16 if bf16 else _native.heads_forward
        logits, kp, sh, hidden, sig = run(kind, hs3, init3, inter3, *groups, flags)
        ctx.meta = meta
        ctx.save_for_backward(hs3, init3, inter3, hidden, sig, *params)
        ctx.shape = (L, B, Q)
        ctx.n_kp, ctx.n_sh_out = len(kp), len(sh)
        outs = [logits] + kp + sh
        return tuple(o.view(L, B, Q, o.shape[-1]) for o in outs)

    @staticmethod
    def backward(ctx, *grads):
        kind, flags, n_cls, n_mlp, n_sh, bf16 = ctx.meta
        hs3, init3, inter3, hidden, sig, *params = ctx.saved_tensors
        L, B, Q = ctx.shape
        g = [x.contiguous().view(L, B * Q, x.shape[-1]) for x in grads]
        grad_logits, grad_kp, grad_sh = g[0], g[1:1 + ctx.n_kp], g[1 + ctx.n_kp:]
        groups = _split(params, n_cls, n_mlp, n_sh)
        run = _native.heads_backward_bf16 if bf16 else _native.heads_backward
        grad_hs, g_cls, g_mlp, g_sh = run(kind, hs3, init3, inter3, *groups, flags, hidden, sig, grad_logits, grad_kp, grad_sh)
        pgrads = g_cls[0] + g_cls[1] + g_mlp[0] + g_mlp[1] + g_sh[0] + g_sh[1]
        return (None, grad_hs.view(L, B, Q, -1), None, None) + tuple(pgrads)


def _split(params, n_cls, n_mlp, n_sh):
    p = list(params)
    cls = (p[:n_cls], p[n_cls:2 * n_cls])
    o = 2 * n_cls
    mlp = (p[o:o + n_mlp], p[o + n_mlp:o + 2 * n_mlp])
    o += 2 * n_mlp
    return cls, mlp, (p[o:o + n_sh], p[o + n_sh:o + 2 * n_sh])


def detr_heads(kind, hs, init_reference, inter_references, cls_embed, mlps, shared=None):
    """Every level's prediction heads over ``hs [L, B, Q, C]``.

    kind: ``"arctic"`` or ``"assembly"``.  cls_embed: per-level Linears (index l used for level l; a ModuleList that repeats
    one module means shared weights).  mlps: the keypoint MLPs, each a per-level sequence of 3-layer MLPs (ARCTIC two-stage:
    key_embed and obj_key_embed; ARCTIC one-stage: none; AssemblyHands: keypoint_embed).  init_reference [B, Q, R] and
    inter_references [>= L - 1, B, Q, R] feed the keypoint epilogues.  shared: ARCTIC's six Linears (mano_pose, mano_beta,
    hand_cam, obj_cam, obj_rot, obj_rad), None for AssemblyHands.

    Returns (logits [L, B, Q, K], [keypoints [L, B, Q, D] per MLP], [shared outputs [L, B, Q, n]])."""
    if kind not in _KIND:
        raise ValueError("detr_heads: kind must be 'arctic' or 'assembly'")
    mlps = list(mlps or ())
    plan = _fused_plan(kind, hs, init_reference, inter_references, cls_embed, mlps, shared)
    if plan is None:
        return detr_heads_reference(kind, hs, init_reference, inter_references, cls_embed, mlps, shared)
    meta, params = plan
    outs = _DetrHeadsFunction.apply(meta, hs, init_reference if mlps else None,
                                    inter_references if mlps and hs.shape[0] > 1 else None, *params)
    n_kp = len(mlps)
    return outs[0], list(outs[1:1 + n_kp]), list(outs[1 + n_kp:])


# ---- DINO (models/dino/dino.py:323-347): the ARCTIC heads over references that carry a gradient ---------------------------
def dino_heads_reference(hs, references, class_embed, key_embed, obj_key_embed, shared):
    """The reference's per-layer composition and stacks (dino.py:329-347); same arguments and results as ``dino_heads``.
    Unlike ARCTIC's, DINO's logits keep the dtype autocast gives them (no ``.to(float32)``)."""
    levels = len(hs)
    classes, keys, outs = [], [[], []], [[] for _ in shared]
    for lvl in range(levels):
        hs_lvl, ref = hs[lvl], references[lvl]
        keys[0].append((key_embed[lvl](hs_lvl) + inverse_sigmoid(ref)).sigmoid() * 2 - 1)
        keys[1].append((obj_key_embed[lvl](hs_lvl) + inverse_sigmoid(ref)).sigmoid() * 2 - 1)
        classes.append(class_embed[lvl](hs_lvl))
        for g, lin in enumerate(shared):
            outs[g].append(lin(hs_lvl))
    return torch.stack(classes), [torch.stack(k) for k in keys], [torch.stack(o) for o in outs]


class _DinoHeadsFunction(torch.autograd.Function):
    """``_DetrHeadsFunction``'s fp32 ARCTIC node whose references may require grad: the same three forward and five backward
    launches, and one more (``msda_heads_ref_backward_f32``) when ``init_ref`` or ``inter_ref`` needs a gradient."""

    @staticmethod
    def forward(ctx, meta, hs, init_ref, inter_ref, *params):
        return _DetrHeadsFunction.forward(ctx, meta, hs, init_ref, inter_ref, *params)

    @staticmethod
    def backward(ctx, *grads):
        kind, flags, n_cls, n_mlp, n_sh, _ = ctx.meta
        hs3, init3, inter3, hidden, sig, *params = ctx.saved_tensors
        L, B, Q = ctx.shape
        g = [x.contiguous().view(L, B * Q, x.shape[-1]) for x in grads]
        grad_logits, grad_kp, grad_sh = g[0], g[1:1 + ctx.n_kp], g[1 + ctx.n_kp:]
        groups = _split(params, n_cls, n_mlp, n_sh)
        grad_hs, g_cls, g_mlp, g_sh = _native.heads_backward(kind, hs3, init3, inter3, *groups, flags, hidden, sig, grad_logits,
                                                             grad_kp, grad_sh)
        need_init, need_inter = ctx.needs_input_grad[2], ctx.needs_input_grad[3] and L > 1
        g_init = g_inter = None
        if need_init or need_inter:
            R = init3.shape[-1]
            g_init, g_inter = _native.heads_ref_backward(init3.view(B * Q, R), inter3.view(L - 1, B * Q, R) if L > 1 else None,
                                                         sig, grad_kp, need_init, need_inter)
            g_init = g_init.view(B, Q, R) if need_init else None
            g_inter = g_inter.view(L - 1, B, Q, R) if need_inter else None
        pgrads = g_cls[0] + g_cls[1] + g_mlp[0] + g_mlp[1] + g_sh[0] + g_sh[1]
        return (None, grad_hs.view(L, B, Q, -1), g_init, g_inter) + tuple(pgrads)


def _dino_fused_operands(hs, references, class_embed, key_embed, obj_key_embed, shared):
    """(meta, params, hs [L, N, Lq, C], init_ref, inter_ref) where the node runs, None where the composition does.  The
    module and shape conditions are ``_fused_plan``'s, asked with the references detached: whether they require grad is the one
    condition this node lifts."""
    L = len(hs)
    first = hs[0]
    if not (_fused_enabled() and 1 <= L <= MAX_LEVELS and len(references) >= L and first.is_cuda
            and first.dtype == torch.float32 and not torch.is_autocast_enabled()):
        return None
    refs = [references[lvl] for lvl in range(L)]
    if any(t.shape != first.shape or t.dtype != first.dtype or t.device != first.device for t in hs) \
            or any(r.shape != refs[0].shape or r.dtype != torch.float32 or r.device != first.device for r in refs):
        return None
    hs4 = hs if torch.is_tensor(hs) else torch.stack(list(hs))
    init_ref = refs[0]
    inter_ref = None if L == 1 else references[1:L] if torch.is_tensor(references) else torch.stack(refs[1:])
    plan = _fused_plan(ARCTIC, hs4, init_ref.detach(), inter_ref.detach() if L > 1 else None, class_embed,
                       [key_embed, obj_key_embed], shared)
    if plan is None:
        return None
    return plan + (hs4, init_ref, inter_ref)


def dino_heads(hs, references, class_embed, key_embed, obj_key_embed, shared):
    """Every decoder layer's prediction heads of the DINO model (models/dino/dino.py:323-347).

    hs: the decoder's list of L tensors [N, Lq, C], or one stacked [L, N, Lq, C].  references: ``reference[:-1]``, L tensors
    [N, Lq, 42] (a stacked tensor is taken too); in DINO all but the first carry a gradient back into the decoder ("look
    forward twice").  class_embed, key_embed, obj_key_embed: per-layer modules (one module repeated means shared weights).
    shared: the six Linears (mano_pose, mano_beta, hand_cam, obj_cam, obj_rot, obj_rad).

    On CUDA fp32 without autocast (and ``MSDA_HEADS_FUSED`` not ``0``, a hidden size the kernels take, L <= 8, module lists that
    are one module repeated or L distinct ones) it is one autograd node: three forward launches, five backward ones and one
    more for the references' gradients, which go to each reference that requires one.  Everything else runs
    ``dino_heads_reference``.  Returns what ``detr_heads("arctic", ...)`` returns:
    (logits [L, N, Lq, K], [hand keypoints, object keypoints] [L, N, Lq, 42], [six shared outputs [L, N, Lq, n]])."""
    shared = list(shared)
    ops = _dino_fused_operands(hs, references, class_embed, key_embed, obj_key_embed, shared)
    if ops is None:
        return dino_heads_reference(hs, references, class_embed, key_embed, obj_key_embed, shared)
    meta, params, hs4, init_ref, inter_ref = ops
    outs = _DinoHeadsFunction.apply(meta, hs4, init_ref, inter_ref, *params)
    return outs[0], list(outs[1:3]), list(outs[3:])
