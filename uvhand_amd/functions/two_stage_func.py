"""The two-stage block of ``DeformableTransformer`` (UVHand models/arctic_transformer.py:91-142, :196-232) on HIP
(csrc/msda_two_stage.hip, include/msda.h):

  * ``encoder_output_proposals``  gen_encoder_output_proposals (:106-142): the 42-d proposals, their logits with ``+inf`` at
    padded / out-of-range rows, and ``memory`` with those rows zeroed, in one pass (``_ProposalsFn``); the backward zeroes
    the same rows of the incoming gradient, and ``learnedxy`` receives a zero gradient — in the reference it reaches the
    graph only through columns that are sliced away, so its ``.grad`` is zeros, not None (AdamW's weight decay then applies);
  * ``select_queries``  the query selection (:208-232), detached: one launch per call, no ``nonzero`` and no host
    synchronisation, so the forward can be captured in a graph;
  * ``pos_trans_embed``  ``pos_trans(get_proposal_pos_embed(r))`` (:91-104, :235) where ``pos_trans[0:2]`` is ONE node
    (``_PosEmbedLinearReluFn``) whose GEMM builds its A operand — the [M, 5376] sin / cos table — from the 42 numbers per
    row in registers: the forward never writes the table, and the node saves r, W1 and the ReLU output only.
    ``pos_trans[2:6]`` is ``_FusedFFNFn`` (bias + ReLU epilogue, split-M weight gradients) plus a ReLU, the LayerNorm(512)
    ``add_layer_norm``.

Every piece runs the reference's composition instead — the same torch ops the reference runs — on CPU tensors, under
autocast (a bf16 form is out of scope), when a kernel's preconditions do not hold (more than 8192 rows per frame for the
selection, a ``pos_trans`` that is not the reference's plain fp32 Sequential or has hooks on it) and with
``MSDA_TWO_STAGE_FUSED=0`` (A/B knob)."""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as MSDA
from .layernorm_func import add_layer_norm
from .linear_func import _FusedFFNFn

FUSED = os.environ.get("MSDA_TWO_STAGE_FUSED", "1") != "0"      # A/B knob: 0 = the reference's composition for all three pieces
HAND_CLASSES = (12, 13)                                          # left / right hand in the ARCTIC label set (:216)


def _plain_cuda_f32(*ts):
    return (FUSED and not torch.is_autocast_enabled()
            and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in ts))


# ---- proposals --------------------------------------------------------------------------------------------------------------
def proposals_composition(memory, memory_padding_mask, level_hw, learnedxy):
    """(output_memory before enc_output, output_proposals): the reference's torch ops (:106-139)."""
    N_, S_, C_ = memory.shape
    proposals = []
    _cur = 0
    for lvl, (H_, W_) in enumerate(level_hw):
        mask_flatten_ = memory_padding_mask[:, _cur:(_cur + H_ * W_)].view(N_, H_, W_, 1)
        valid_H = torch.sum(~mask_flatten_[:, :, 0, 0], 1)
        valid_W = torch.sum(~mask_flatten_[:, 0, :, 0], 1)
        grid_y, grid_x = torch.meshgrid(torch.linspace(0, H_ - 1, H_, dtype=torch.float32, device=memory.device),
                                        torch.linspace(0, W_ - 1, W_, dtype=torch.float32, device=memory.device), indexing="ij")
        grid = torch.cat([grid_x.unsqueeze(-1), grid_y.unsqueeze(-1)], -1)
        scale = torch.cat([valid_W.unsqueeze(-1), valid_H.unsqueeze(-1)], 1).view(N_, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(N_, -1, -1, -1) + 0.5) / scale
        if learnedxy is not None:
            xy = torch.ones_like(grid).repeat(1, 1, 1, 20) * learnedxy.sigmoid() * (2.0 ** lvl)
        else:
            xy = (torch.ones_like(grid) * 0.05 * (2.0 ** lvl)).repeat(1, 1, 1, 20)
        proposals.append(torch.cat((grid, xy), -1).view(N_, -1, 42))
        _cur += H_ * W_
    output_proposals = torch.cat(proposals, 1)
    valid = ((output_proposals > 0.01) & (output_proposals < 0.99)).all(-1, keepdim=True)
    output_proposals = torch.log(output_proposals / (1 - output_proposals))
    output_proposals = output_proposals.masked_fill(memory_padding_mask.unsqueeze(-1), float("inf"))
    output_proposals = output_proposals.masked_fill(~valid, float("inf"))
    output_memory = memory.masked_fill(memory_padding_mask.unsqueeze(-1), float(0))
    output_memory = output_memory.masked_fill(~valid, float(0))
    return output_memory, output_proposals


class _ProposalsFn(Function):
    """(output_memory, output_proposals) in one kernel; the proposals carry no gradient (their only differentiable inputs
    are the learned offsets, whose columns the model slices away), the learned offsets get zeros."""

    @staticmethod
    def forward(ctx, memory, padding_mask, learnedxy, level_hw):
        props, mem_out, row_mask = MSDA.two_stage_proposals(memory, padding_mask, level_hw, learnedxy)
        ctx.save_for_backward(row_mask)
        ctx.mark_non_differentiable(props)
        ctx.xy_shape = tuple(learnedxy.shape) if learnedxy is not None else None
        return mem_out, props

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mem, grad_props):
        (row_mask,) = ctx.saved_tensors
        need = ctx.needs_input_grad
        gm = gxy = None
        if need[0]:
            gm = grad_mem.contiguous().clone()
            C = gm.shape[-1]
            if C % 4 == 0 and gm.data_ptr() % 16 == 0:
                MSDA.zero_masked_rows_(gm.view(-1, C), row_mask.view(-1))
            else:
                gm.masked_fill_(row_mask.unsqueeze(-1), 0.0)
        if need[2]:
            gxy = torch.zeros(ctx.xy_shape, dtype=grad_mem.dtype, device=grad_mem.device)
        return gm, None, gxy, None


def encoder_output_proposals(memory, memory_padding_mask, level_hw, learnedxy):
    """(memory with padded / out-of-range rows zeroed, output_proposals [N, S, 42]) — before ``enc_output``."""
    if (_plain_cuda_f32(memory, learnedxy) and memory.dim() == 3 and memory.shape[-1] % 4 == 0
            and memory_padding_mask.dtype == torch.bool and memory_padding_mask.is_cuda and 0 < len(level_hw) <= 16
            and sum(h * w for h, w in level_hw) == memory.shape[1] and memory.numel() < (1 << 31)):
        xy = learnedxy.contiguous() if learnedxy is not None else None
        return _ProposalsFn.apply(memory.contiguous(), memory_padding_mask.contiguous(), xy, list(level_hw))
    return proposals_composition(memory, memory_padding_mask, level_hw, learnedxy)


# ---- query selection --------------------------------------------------------------------------------------------------------
def select_composition(enc_outputs_class, hand_coord, obj_coord, output_proposals, topk, hand_classes=HAND_CLASSES):
    """(refpoint_unsig, reference_points): the reference's selection (:208-232) with its boolean-mask assignments written as
    torch.where (the same values, without the nonzero)."""
    topk_proposals = torch.topk(enc_outputs_class.max(-1)[0], topk, dim=1)[1]
    class_indices = torch.gather(enc_outputs_class.argmax(dim=-1), 1, topk_proposals)
    hand_idx = (class_indices == hand_classes[0]) | (class_indices == hand_classes[1])
    obj_idx = ~hand_idx & (class_indices != 0)
    index = topk_proposals.unsqueeze(-1).repeat(1, 1, 42)
    obj_kp = torch.gather(obj_coord, 1, index).detach()
    hand_kp = torch.gather(hand_coord, 1, index).detach()
    ref = torch.gather(output_proposals, 1, index).detach()
    ref = torch.where(obj_idx.unsqueeze(-1), obj_kp, ref)
    ref = torch.where(hand_idx.unsqueeze(-1), hand_kp, ref)
    return ref, ref.sigmoid() * 2 - 1


def select_queries(enc_outputs_class, hand_coord, obj_coord, output_proposals, topk, hand_classes=HAND_CLASSES,
                   return_indices=False):
    """(refpoint_unsig [N, Q, 42], reference_points [N, Q, 42]) (+ the selected rows [N, Q] with return_indices): the top
    ``topk`` rows per frame by the maximum class logit — descending; ties: the lower row first; NaN above every number —
    and their 42 coordinates from the hand / object / proposal source by the argmax class.  Detached."""
    N, S, K = enc_outputs_class.shape
    if int(topk) > S:
        raise RuntimeError("selected index k out of range")
    ts = (enc_outputs_class, hand_coord, obj_coord, output_proposals)
    if _plain_cuda_f32(*ts) and hand_coord.shape[-1] == 42 and MSDA.two_stage_select_supported(S, K, topk):
        idx, ref, refp = MSDA.two_stage_select(*(t.detach().contiguous() for t in ts), topk, hand_classes)
        return (ref, refp, idx) if return_indices else (ref, refp)
    ref, refp = select_composition(*ts, topk, hand_classes)
    if return_indices:
        return ref, refp, torch.topk(enc_outputs_class.max(-1)[0], topk, dim=1)[1]
    return ref, refp


# ---- proposal embedding and pos_trans ---------------------------------------------------------------------------------------
def pe_dim_t(device):
    """The 128-entry table of :96-97 (torch's own pow, so nothing can diverge from it)."""
    dim_t = torch.arange(128, dtype=torch.float32, device=device)
    return 10000 ** (2 * (dim_t // 2) / 128)


def pos_embed_composition(proposals):
    """get_proposal_pos_embed (:91-104) in torch ops: [..., 42] -> [..., 5376]."""
    dim_t = pe_dim_t(proposals.device)
    proposals = proposals.sigmoid() * (2 * math.pi)
    pos = proposals[..., None] / dim_t
    return torch.stack((pos[..., 0::2].sin(), pos[..., 1::2].cos()), dim=-1).flatten(-3)


def proposal_pos_embed(proposals):
    """[N, L, 42] -> [N, L, 5376]; one HIP kernel for fp32 CUDA tensors (no autograd: the reference feeds it detached)."""
    if _plain_cuda_f32(proposals) and proposals.shape[-1] == 42 and not proposals.requires_grad:
        r2 = proposals.reshape(-1, 42).contiguous()
        pe = MSDA.proposal_pos_embed(r2, pe_dim_t(proposals.device)[0::2].contiguous())
        return pe.view(*proposals.shape[:-1], MSDA.PE_WIDTH)
    return pos_embed_composition(proposals)


class _PosEmbedLinearReluFn(Function):
    """relu(PE(r) @ W1^T + b1): forward on the fused kernel (the PE table never in memory); backward: the ReLU mask from the
    saved output, then dW1 = dY1^T . PE(r) and db1 = sum dY1 on the split-M weight-gradient kernel (fixed order: bitwise
    reproducible) over PE regenerated by the same generator into a buffer that lives for this backward only.  r needs no
    gradient (detached in the reference)."""

    @staticmethod
    def forward(ctx, r2, dim_t, weight, bias):
        y = MSDA.proposal_pos_linear_relu(r2, dim_t, weight, bias)
        ctx.save_for_backward(r2, dim_t, y)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        r2, dim_t, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        gw = gb = None
        if need[2] or need[3]:
            gh = grad_y.contiguous().clone()
            MSDA.relu_dropout_backward_(gh, y, 1.0)
            pe = MSDA.proposal_pos_embed(r2, dim_t)
            gw, gb = MSDA.linear_wgrad(gh, pe, want_bias=ctx.has_bias and need[3])
            del pe
            if not need[2]:
                gw = None
        return None, None, gw, gb


def pos_embed_linear_relu(r2, linear):
    """relu(linear(PE(r2))) for r2 [M, 42] (detached, fp32 CUDA) and the 5376 -> out ``nn.Linear``: one autograd node."""
    dim_t = pe_dim_t(r2.device)[0::2].contiguous()
    return _PosEmbedLinearReluFn.apply(r2.contiguous(), dim_t, linear.weight, linear.bias)


def _has_hooks(module):
    from ..modules.deformable_layers import _has_listener
    return any(_has_listener(m) for m in module.modules())


def pos_trans_fusable(pos_trans, refpoints):
    """The fused route applies: ``pos_trans`` is exactly the reference's Sequential (Linear(5376, a), ReLU, Linear(a, b), ReLU,
    Linear(b, c), ReLU) of plain fp32 CUDA layers with biases, no hook on it or its children, fp32 CUDA detached refpoints."""
    if not (type(pos_trans) is nn.Sequential and len(pos_trans) == 6):
        return False
    mods = list(pos_trans)
    if not all(type(mods[i]) is nn.Linear and type(mods[i + 1]) is nn.ReLU and not mods[i + 1].inplace for i in (0, 2, 4)):
        return False
    l0, l2, l4 = mods[0], mods[2], mods[4]
    ps = [l0.weight, l0.bias, l2.weight, l2.bias, l4.weight, l4.bias]
    return (l0.in_features == MSDA.PE_WIDTH and all(p is not None for p in ps) and _plain_cuda_f32(refpoints, *ps)
            and refpoints.shape[-1] == 42 and not refpoints.requires_grad
            and all(lin.out_features % 4 == 0 and lin.in_features % 4 == 0 for lin in (l0, l2, l4))
            and l2.in_features == l0.out_features and l4.in_features == l2.out_features
            and not _has_hooks(pos_trans) and refpoints.numel() > 0)


def pos_trans_embed(pos_trans, pos_trans_norm, refpoints):
    """``pos_trans_norm(pos_trans(get_proposal_pos_embed(refpoints)))`` (:235)."""
    if pos_trans_fusable(pos_trans, refpoints):
        lead = refpoints.shape[:-1]
        y1 = pos_embed_linear_relu(refpoints.reshape(-1, 42), pos_trans[0])
        h = F.relu(_FusedFFNFn.apply(y1, pos_trans[2].weight, pos_trans[2].bias, pos_trans[4].weight, pos_trans[4].bias, 0.0,
                                     False))
        return add_layer_norm(h.view(*lead, h.shape[-1]), None, pos_trans_norm)
    return pos_trans_norm(pos_trans(pos_embed_composition(refpoints)))
