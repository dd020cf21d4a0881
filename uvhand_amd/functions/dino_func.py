"""The DINO decoder's query positions and refinement (UVHand models/dino/deformable_transformer.py:730-746, :781-817;
models/dino/utils.py:138-165) on HIP (csrc/msda_dino.hip, include/msda.h):

  * ``sine_embed_for_position``  gen_sineembed_for_position: the [L, N, 256] sin / cos table of the (x, y) means of the reference
    points, optionally scaled by the level-0 valid ratios first (what the decoder feeds it), one launch instead of about a
    dozen element-wise torch kernels;
  * ``query_pos``  ``ref_point_head(gen_sineembed_for_position((reference_points * valid_ratios)[level 0]))`` as ONE autograd
    node.  Two forwards: ``fused`` — one launch, the table generated in the A operand of the first product and the hidden
    activations kept on chip as the A operand of the second (written once, for the backward) — and ``table`` — the table
    kernel, then the FFN node the layers use (``_FusedFFNFn``).  ``MSDA_DINO_QUERY_POS=table|fused`` selects; the default is
    the faster one at the training shape (README, "DINO decoder").  The fused node's backward is library launches only:
    both weight gradients on the split-M MFMA kernel, the input gradient of the second layer, the ReLU mask in place, and the
    table regenerated into a buffer that lives for that backward only;
  * ``refine``  the per-layer refinement: the reference adds the key / object head's output to the rows its class argmax
    selects with boolean-mask indexing (``outputs_unsig[obj_idx] += ...``, :796-797 — a ``nonzero`` and a host
    synchronisation each); here one launch per direction.  Unlike ARCTIC's refinement the result is not detached where the
    model reads it (dino.py:329-337, "look forward twice"), so the node has a backward: gradient to the two deltas;
  * ``select_queries_dino``  the transformer's two-stage selection (:348-387) for any number of encoder rows per frame
    (csrc/msda_dino_select.hip): the top ``num_queries`` rows by their largest class logit, the rows of ``output_memory`` and
    of the proposals they select and the class rule's code per row, as ONE autograd node — two launches forward, and a backward
    of one launch that writes every element of ``output_memory``'s gradient.

Every piece runs the reference's composition instead — the same torch ops the reference runs, boolean-index adds and their
synchronisations included — on CPU tensors, other dtypes, under autocast, with hooks on the MLP, for reference points that
require grad (``rm_detach=['dec']``) and with ``MSDA_DINO_FUSED=0`` (A/B knob)."""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as MSDA
from .linear_func import _FusedFFNFn
from .two_stage_func import _has_hooks, pe_dim_t

FUSED = os.environ.get("MSDA_DINO_FUSED", "1") != "0"               # A/B knob: 0 = the reference's composition for every piece
QUERY_POS_ROUTE = os.environ.get("MSDA_DINO_QUERY_POS", "fused")    # table | fused: the forward of the query_pos node
HAND_CLASSES = (12, 13)                                              # left / right hand in the ARCTIC label set (:787)


def _plain_cuda_f32(*ts):
    return (FUSED and not torch.is_autocast_enabled()
            and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in ts))


def inverse_sigmoid(x, eps=1e-5):
    """util/misc.py:614-618."""
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


# ---- the sine table -----------------------------------------------------------------------------------------------------------
def sine_embed_composition(pos_tensor, valid_xy=None):
    """gen_sineembed_for_position (utils.py:138-165) in torch ops: [L, N, 2 | 42] -> [L, N, 256], y half first.  With
    ``valid_xy`` [N, 2] the points are scaled first, as the decoder does for level 0 (:732-738)."""
    if valid_xy is not None:
        pos_tensor = pos_tensor * valid_xy.repeat(1, pos_tensor.shape[-1] // 2)[None]
    scale = 2 * math.pi
    dim_t = pe_dim_t(pos_tensor.device)
    x_embed = pos_tensor[:, :, 0::2].mean(-1) * scale
    y_embed = pos_tensor[:, :, 1::2].mean(-1) * scale
    pos_x = x_embed[:, :, None] / dim_t
    pos_y = y_embed[:, :, None] / dim_t
    pos_x = torch.stack((pos_x[:, :, 0::2].sin(), pos_x[:, :, 1::2].cos()), dim=3).flatten(2)
    pos_y = torch.stack((pos_y[:, :, 0::2].sin(), pos_y[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((pos_y, pos_x), dim=2)


def _rows_fusable(pos, valid_xy):
    return (_plain_cuda_f32(pos, valid_xy) and pos.dim() == 3 and pos.shape[-1] in (2, 42) and not pos.requires_grad
            and pos.shape[1] > 0 and pos.numel() > 0 and pos.shape[0] * pos.shape[1] * MSDA.DINO_PE_WIDTH < (1 << 31)
            and (valid_xy is None or (tuple(valid_xy.shape) == (pos.shape[1], 2) and not valid_xy.requires_grad)))


def _dim_t64(device):
    return pe_dim_t(device)[0::2].contiguous()


def sine_embed_for_position(pos, valid_xy=None):
    """Drop-in for gen_sineembed_for_position: pos [L, N, 2 | 42] (sequence-first) -> [L, N, 256]; ``valid_xy`` [N, 2] scales
    the (x, y) pairs first.  One HIP kernel for detached fp32 CUDA points (the reference feeds it detached)."""
    if _rows_fusable(pos, valid_xy):
        L, N, W = pos.shape
        pe = MSDA.dino_sine_embed(pos.contiguous().view(L * N, W), valid_xy.contiguous() if valid_xy is not None else None, N,
                                  _dim_t64(pos.device))
        return pe.view(L, N, MSDA.DINO_PE_WIDTH)
    return sine_embed_composition(pos, valid_xy)


# ---- query positions ----------------------------------------------------------------------------------------------------------
def query_pos_composition(ref, valid_ratios, ref_point_head):
    """The reference's lines :731-744: scale by every level's valid ratio, take level 0, the sine table, the MLP."""
    if ref.shape[-1] == 42:
        ref_input = ref[:, :, None] * valid_ratios.unsqueeze(0).repeat(1, 1, 1, 21)
    else:
        assert ref.shape[-1] == 2
        ref_input = ref[:, :, None] * valid_ratios[None, :]
    return ref_point_head(sine_embed_composition(ref_input[:, :, 0, :]))


class _QueryPosFn(Function):
    """ref_point_head(table(ref)) with the forward in one launch (msda_dino_query_pos_forward_f32).  Saved: ref, the valid
    ratios, h and the second weight — not the table.  Backward, existing kernels only: dW2 / db2 = wgrad(gy, h); gh =
    dgrad(gy, W2) masked by h > 0 in place; the table regenerated; dW1 / db1 = wgrad(gh, table).  Five launches, fewer when
    the head is frozen.  ref needs no gradient (detached on this route)."""

    @staticmethod
    def forward(ctx, ref2, valid_xy, n_frames, dim_t, w1, b1, w2, b2):
        h, y = MSDA.dino_query_pos_forward(ref2, valid_xy, n_frames, dim_t, w1, b1, w2, b2)
        ctx.save_for_backward(ref2, valid_xy, dim_t, h, w2)
        ctx.n_frames = n_frames
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        ref2, valid_xy, dim_t, h, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        gw1 = gb1 = gw2 = gb2 = None
        gy = grad_y.contiguous()
        if need[6] or need[7]:
            gw2, gb2 = MSDA.linear_wgrad(gy, h, want_bias=need[7])
            if not need[6]:
                gw2 = None
        if need[4] or need[5]:
            gh = MSDA.linear_dgrad(gy, w2)
            MSDA.relu_dropout_backward_(gh, h, 1.0)
            pe = MSDA.dino_sine_embed(ref2, valid_xy, ctx.n_frames, dim_t)
            gw1, gb1 = MSDA.linear_wgrad(gh, pe, want_bias=need[5])
            del pe
            if not need[4]:
                gw1 = None
        return None, None, None, None, gw1, gb1, gw2, gb2


def query_pos_fusable(ref, valid_ratios, ref_point_head):
    """The HIP routes apply: detached fp32 CUDA points [L, N, 2 | 42], valid ratios [N, levels, 2], and a head that is two plain
    fp32 256 -> 256 Linear layers with biases under ``.layers``, without hooks."""
    layers = getattr(ref_point_head, "layers", None)
    if not (isinstance(layers, nn.ModuleList) and len(layers) == 2 and getattr(ref_point_head, "num_layers", 2) == 2
            and all(type(l) is nn.Linear and l.bias is not None for l in layers)):
        return False
    l1, l2 = layers
    ps = [l1.weight, l1.bias, l2.weight, l2.bias]
    return (valid_ratios is not None and valid_ratios.dim() == 3 and valid_ratios.shape[-1] == 2 and valid_ratios.shape[1] > 0
            and not valid_ratios.requires_grad and _plain_cuda_f32(valid_ratios, *ps)
            and _rows_fusable(ref, valid_ratios[:, 0])
            and all(p.is_contiguous() and p.data_ptr() % 16 == 0 for p in ps) and not _has_hooks(ref_point_head)
            and MSDA.dino_query_pos_supported(ref.shape[-1], ref.shape[1], ref.shape[0] * ref.shape[1], l1.out_features,
                                              l2.out_features)
            and l1.in_features == MSDA.DINO_PE_WIDTH and l2.in_features == l1.out_features)


def query_pos(ref, valid_ratios, ref_point_head, route=None):
    """``ref_point_head(gen_sineembed_for_position((ref * valid_ratios)[level 0]))`` for sequence-first ref [L, N, 2 | 42] and
    valid_ratios [N, levels, 2]: [L, N, 256].  ``route``: 'fused' | 'table' (default: MSDA_DINO_QUERY_POS)."""
    if not query_pos_fusable(ref, valid_ratios, ref_point_head):
        return query_pos_composition(ref, valid_ratios, ref_point_head)
    L, N, W = ref.shape
    valid_xy = valid_ratios[:, 0].contiguous()
    l1, l2 = ref_point_head.layers
    route = route or QUERY_POS_ROUTE
    if route == "table":
        pe = MSDA.dino_sine_embed(ref.contiguous().view(L * N, W), valid_xy, N, _dim_t64(ref.device))
        y = _FusedFFNFn.apply(pe, l1.weight, l1.bias, l2.weight, l2.bias, 0.0, False)
    elif route == "fused":
        y = _QueryPosFn.apply(ref.contiguous().view(L * N, W), valid_xy, N, _dim_t64(ref.device), l1.weight, l1.bias, l2.weight,
                              l2.bias)
    else:
        raise ValueError("MSDA_DINO_QUERY_POS must be 'table' or 'fused', got %r" % (route,))
    return y.view(L, N, l2.out_features)


# ---- refinement ---------------------------------------------------------------------------------------------------------------
def refine_composition(reference_points, cls_out, delta_key, delta_obj, hand_classes=HAND_CLASSES):
    """The reference's refinement (:783-798) in its own torch ops, boolean-mask adds (and their host syncs) included."""
    class_indices = cls_out.argmax(dim=-1)
    obj_idx = torch.ones_like(class_indices, dtype=torch.bool)
    hand_idx = torch.zeros_like(class_indices, dtype=torch.bool)
    for idx in [0] + list(hand_classes):
        obj_idx &= (class_indices != idx)
        if idx != 0:
            hand_idx |= (class_indices == idx)
    outputs_unsig = inverse_sigmoid(reference_points)
    outputs_unsig[obj_idx] += delta_obj[obj_idx]
    outputs_unsig[hand_idx] += delta_key[hand_idx]
    return outputs_unsig.sigmoid() * 2 - 1


class _RefineFn(Function):
    """new_reference_points and the row codes in one launch; backward: g_u = g * (1 - out^2) / 2 (out = 2 sigmoid(u) - 1, so
    d out / d u = 2 s (1 - s) = (1 + out) (1 - out) / 2), to delta_key where the code is 2 and delta_obj where it is 1."""

    @staticmethod
    def forward(ctx, ref, cls_out, delta_key, delta_obj, hand_classes):
        out, code = MSDA.dino_refine_forward(ref, cls_out, delta_key, delta_obj, hand_classes)
        ctx.save_for_backward(out, code)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        out, code = ctx.saved_tensors
        need = ctx.needs_input_grad
        gk = go = None
        if need[2] or need[3]:
            gk, go = MSDA.dino_refine_backward(grad_out.contiguous(), out, code, need[2], need[3])
        return None, None, gk, go, None


def refine_fusable(reference_points, cls_out, delta_key, delta_obj):
    ts = (reference_points, cls_out, delta_key, delta_obj)
    return (_plain_cuda_f32(*ts) and reference_points.shape[-1] == 42 and reference_points.numel() > 0
            and not reference_points.requires_grad and cls_out.dim() == reference_points.dim() and cls_out.shape[-1] > 0
            and tuple(cls_out.shape[:-1]) == tuple(reference_points.shape[:-1])
            and tuple(delta_key.shape) == tuple(reference_points.shape) and tuple(delta_obj.shape) == tuple(reference_points.shape)
            and max(reference_points.numel(), cls_out.numel()) < (1 << 31))


def refine(reference_points, cls_out, delta_key, delta_obj, hand_classes=HAND_CLASSES):
    """new_reference_points [..., 42] = sigmoid(inverse_sigmoid(reference_points) + the selected head's delta) * 2 - 1, with
    gradient to the two deltas; the caller detaches for the next layer, as the reference does."""
    if refine_fusable(reference_points, cls_out, delta_key, delta_obj):
        return _RefineFn.apply(reference_points.contiguous(), cls_out.detach().contiguous(), delta_key.contiguous(),
                               delta_obj.contiguous(), tuple(hand_classes))
    if (_plain_cuda_f32(reference_points, cls_out, delta_key, delta_obj) and reference_points.shape[-1] != 42
            and not reference_points.requires_grad):
        # 2-wide points (heads of the same width): no kernel, but the same values without the nonzero of a boolean index
        classes = cls_out.argmax(dim=-1)
        hand = (classes == hand_classes[0]) | (classes == hand_classes[1])
        obj = ~hand & (classes != 0)
        unsig = inverse_sigmoid(reference_points)
        unsig = torch.where(obj[..., None], unsig + delta_obj, unsig)
        unsig = torch.where(hand[..., None], unsig + delta_key, unsig)
        return unsig.sigmoid() * 2 - 1
    return refine_composition(reference_points, cls_out, delta_key, delta_obj, hand_classes)


# ---- two-stage query selection ------------------------------------------------------------------------------------------------
def dino_select_composition(enc_class, output_memory, output_proposals, topk, hand_classes=HAND_CLASSES):
    """(topk_idx [N, Q] int64, tgt_undetach [N, Q, C], prop_sel [N, Q, 42], code [N, Q] uint8): the reference's selection
    (:348-355, :369, :387) in torch ops, on any device and without a host synchronisation.  The rule the kernels follow: per
    frame the Q rows with the largest row maximum, descending; ties: the lower row first; NaN above every number, -0 equal to
    +0.  ``torch.topk`` promises no order among equal values, so the order is a stable descending sort of the row maxima."""
    row_max = enc_class.max(-1)[0]
    if int(topk) > row_max.shape[1]:
        return torch.topk(row_max, int(topk), dim=1)                 # torch's own error ("selected index k out of range")
    topk_idx = torch.sort(row_max.detach(), dim=1, descending=True, stable=True)[1][:, :int(topk)]
    classes = torch.gather(enc_class.argmax(dim=-1), 1, topk_idx)
    hand = (classes == hand_classes[0]) | (classes == hand_classes[1])
    code = hand.to(torch.uint8) * 2 + (~hand & (classes != 0)).to(torch.uint8)
    tgt = torch.gather(output_memory, 1, topk_idx.unsqueeze(-1).expand(-1, -1, output_memory.shape[-1]))
    prop_sel = torch.gather(output_proposals.detach(), 1, topk_idx.unsqueeze(-1).expand(-1, -1, output_proposals.shape[-1]))
    return topk_idx, tgt, prop_sel, code


class _DinoSelectFn(Function):
    """The selection as one node (msda_dino_select_forward_f32): only the gathered rows of ``output_memory`` are
    differentiable, and only with respect to it; the inverse map ``slot`` is what the backward reads — one launch that writes
    every element of the gradient (selected rows copied, the others zero)."""

    @staticmethod
    def forward(ctx, enc_class, output_memory, output_proposals, topk, hand_classes):
        idx, slot, tgt, prop_sel, code = MSDA.dino_select_forward(enc_class, output_memory, output_proposals, topk, hand_classes)
        ctx.save_for_backward(slot)
        ctx.mark_non_differentiable(idx, prop_sel, code)
        return idx, tgt, prop_sel, code

    @staticmethod
    @once_differentiable
    def backward(ctx, g_idx, g_tgt, g_prop, g_code):
        (slot,) = ctx.saved_tensors
        gm = MSDA.dino_select_backward(slot, g_tgt.contiguous()) if ctx.needs_input_grad[1] else None
        return None, gm, None, None, None


def select_fusable(enc_class, output_memory, output_proposals, topk):
    ts = (enc_class, output_memory, output_proposals)
    return (_plain_cuda_f32(*ts) and all(t.dim() == 3 for t in ts) and output_proposals.shape[-1] == 42
            and tuple(output_memory.shape[:2]) == tuple(enc_class.shape[:2]) == tuple(output_proposals.shape[:2])
            and 0 < enc_class.shape[0] <= MSDA.DINO_SELECT_MAX_FRAMES and all(t.numel() < (1 << 31) for t in ts)
            and MSDA.dino_select_supported(enc_class.shape[1], enc_class.shape[2], int(topk), output_memory.shape[-1]))


def select_queries_dino(enc_class, output_memory, output_proposals, topk, hand_classes=HAND_CLASSES):
    """(topk_idx [N, Q] int64, tgt_undetach [N, Q, C], prop_sel [N, Q, 42], code [N, Q] uint8) for class logits [N, S, K],
    ``output_memory`` [N, S, C] and ``output_proposals`` [N, S, 42]: the top ``topk`` rows per frame by their largest class
    logit, the rows of the two tensors they select and the class rule's code per row (2 hand, 1 object, 0 neither).  Only
    ``tgt_undetach`` carries gradient, to ``output_memory``.  HIP kernels for fp32 CUDA tensors outside autocast within
    msda_dino_select_supported's envelope; ``dino_select_composition`` otherwise."""
    if select_fusable(enc_class, output_memory, output_proposals, topk):
        return _DinoSelectFn.apply(enc_class.detach().contiguous(), output_memory.contiguous(),
                                   output_proposals.detach().contiguous(), int(topk), tuple(hand_classes))
    return dino_select_composition(enc_class, output_memory, output_proposals, topk, hand_classes)
