"""The AssemblyHands transformer's refinement and two-stage block (UVHand models/assembly_transformer.py:183-226, :407-465)
on HIP (csrc/msda_assembly.hip, include/msda.h):

  * ``refine``  the decoder's keypoint refinement (:416-462): the reference adds the keypoint head to the rows classified as a
    hand with boolean-mask indexing (``new_reference_points[hand_idx] += ...``, :442), i.e. a ``nonzero`` and a host
    synchronisation per use; here one launch per decoder layer writes the next reference points [N, Q, 42], detached as in
    the reference (the node has no backward);
  * ``encoder_output_proposals``  gen_encoder_output_proposals (:106-141) on the one level the forward passes (the last,
    :184): the 2-d proposal logits with ``+inf`` at padded / out-of-range rows, those rows of ``memory`` zeroed, in one pass
    over the level's rows read in place (``_LevelProposalsFn``); the backward zeroes the same rows of the incoming gradient;
  * ``select_queries``  the selection (:202-226): the object row by the reference's strict ``best < score`` loop over
    classes 1..8, the left / right hand rows by the argmax of classes 9 / 10, and the mean (x, y) of the sigmoid of their
    21 keypoints — one workgroup per frame, one launch, no host synchronisation (the reference's loop is 8 boolean-mask
    updates, each a sync).

Every piece runs the reference's composition instead — the same torch ops the reference runs, syncs included — on CPU
tensors, under autocast, for non-fp32 inputs, when a kernel's preconditions do not hold and with ``MSDA_ASSEMBLY_FUSED=0``
(A/B knob)."""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as MSDA

FUSED = os.environ.get("MSDA_ASSEMBLY_FUSED", "1") != "0"      # A/B knob: 0 = the reference's composition for all three pieces
OBJ_CLASSES = (1, 8)                                            # object classes of the H2O label layout (:204)
LEFT_CLASS, RIGHT_CLASS = 9, 10                                 # left / right hand (:209-210)
KEYPOINTS = 21


def _plain_cuda_f32(*ts):
    return (FUSED and not torch.is_autocast_enabled()
            and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in ts))


def inverse_sigmoid(x, eps=1e-5):
    """util/misc.py:614-618."""
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


# ---- refinement ---------------------------------------------------------------------------------------------------------------
def refine_composition(reference_points, cls_out, tmp):
    """The reference's refinement (:416-462) in its own torch ops, boolean-mask add (and its host sync) included."""
    hand_idx = cls_out.argmax(dim=-1) != 0
    if reference_points.shape[-1] == 2:
        ref = inverse_sigmoid(reference_points).unsqueeze(2)
        new_reference_points = ref.repeat(1, 1, KEYPOINTS, 1).clone()
    elif reference_points.shape[-1] == 42:
        ref_x = reference_points[..., 0::2].mean(-1).unsqueeze(-1)
        ref_y = reference_points[..., 1::2].mean(-1).unsqueeze(-1)
        new_reference_points = inverse_sigmoid((torch.cat([ref_x, ref_y], dim=-1) + 0.5) / 2).unsqueeze(2).repeat(
            1, 1, KEYPOINTS, 1).clone()
    else:
        raise ValueError("reference_points must have 2 or 42 coordinates per query, got %d" % reference_points.shape[-1])
    new_reference_points[hand_idx] += tmp.reshape(tmp.shape[0], tmp.shape[1], -1, 3)[hand_idx][..., :2]
    new_reference_points = new_reference_points.reshape(tmp.shape[0], tmp.shape[1], -1)
    return (new_reference_points.sigmoid() * 2 - 0.5).detach()


def refine_fusable(reference_points, cls_out, tmp):
    return (_plain_cuda_f32(reference_points, cls_out, tmp) and reference_points.dim() == 3
            and reference_points.shape[-1] in (2, 42) and tuple(cls_out.shape[:-1]) == tuple(reference_points.shape[:-1])
            and tuple(tmp.shape) == tuple(reference_points.shape[:-1]) + (3 * KEYPOINTS,) and cls_out.shape[-1] > 0)


def refine(reference_points, cls_out, tmp):
    """The next reference points [N, Q, 42] from reference_points [N, Q, 2 | 42], the layer's class logits [N, Q, K] and its
    keypoint head output [N, Q, 63]; detached."""
    if refine_fusable(reference_points, cls_out, tmp):
        return MSDA.assembly_refine(*(t.detach().contiguous() for t in (reference_points, cls_out, tmp)))
    return refine_composition(reference_points, cls_out, tmp)


# ---- proposals ----------------------------------------------------------------------------------------------------------------
def proposals_composition(memory, memory_padding_mask, level_hw):
    """(output_memory before enc_output, output_proposals [N, S, 2]): the reference's torch ops (:116-139)."""
    N, S, C = memory.shape
    proposals = []
    _cur = 0
    for lvl, (H, W) in enumerate(level_hw):
        mask_flatten_ = memory_padding_mask[:, _cur:(_cur + H * W)].view(N, H, W, 1)
        valid_H = torch.sum(~mask_flatten_[:, :, 0, 0], 1)
        valid_W = torch.sum(~mask_flatten_[:, 0, :, 0], 1)
        grid_y, grid_x = torch.meshgrid(torch.linspace(0, H - 1, H, dtype=torch.float32, device=memory.device),
                                        torch.linspace(0, W - 1, W, dtype=torch.float32, device=memory.device), indexing="ij")
        grid = torch.cat([grid_x.unsqueeze(-1), grid_y.unsqueeze(-1)], -1)
        scale = torch.cat([valid_W.unsqueeze(-1), valid_H.unsqueeze(-1)], 1).view(N, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(N, -1, -1, -1) + 0.5) / scale
        proposals.append(grid.view(N, -1, 2))
        _cur += H * W
    output_proposals = torch.cat(proposals, 1)
    valid = ((output_proposals > 0.01) & (output_proposals < 0.99)).all(-1, keepdim=True)
    output_proposals = torch.log(output_proposals / (1 - output_proposals))
    output_proposals = output_proposals.masked_fill(memory_padding_mask.unsqueeze(-1), float("inf"))
    output_proposals = output_proposals.masked_fill(~valid, float("inf"))
    output_memory = memory.masked_fill(memory_padding_mask.unsqueeze(-1), float(0))
    output_memory = output_memory.masked_fill(~valid, float(0))
    return output_memory, output_proposals


class _LevelProposalsFn(Function):
    """(output_memory, output_proposals) of one level in one kernel; the proposals carry no gradient (they depend on the mask
    only), the gradient of ``memory`` is the incoming one with the zeroed rows zeroed."""

    @staticmethod
    def forward(ctx, memory, padding_mask, hw):
        props, mem_out, row_mask = MSDA.assembly_proposals(memory, padding_mask, hw)
        ctx.save_for_backward(row_mask)
        ctx.mark_non_differentiable(props)
        return mem_out, props

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mem, grad_props):
        (row_mask,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        gm = grad_mem.contiguous().clone()
        C = gm.shape[-1]
        if C % 4 == 0 and gm.data_ptr() % 16 == 0:
            MSDA.zero_masked_rows_(gm.view(-1, C), row_mask.view(-1))
        else:
            gm.masked_fill_(row_mask.unsqueeze(-1), 0.0)
        return gm, None, None


def encoder_output_proposals(memory, memory_padding_mask, level_hw):
    """(memory with padded / out-of-range rows zeroed, output_proposals [N, S, 2]) — before ``enc_output``.  The kernel takes
    one level (what the forward passes); ``memory`` / the mask may be slices of the flattened pyramid."""
    level_hw = [(int(h), int(w)) for h, w in level_hw]
    if (_plain_cuda_f32(memory) and memory.dim() == 3 and len(level_hw) == 1 and memory.shape[1] == level_hw[0][0] * level_hw[0][1]
            and memory.shape[-1] % 4 == 0 and memory.stride(2) == 1 and memory.stride(1) == memory.shape[-1]
            and memory.stride(0) % 4 == 0 and memory.data_ptr() % 16 == 0 and memory.shape[0] * memory.stride(0) < (1 << 31)
            and memory_padding_mask.dtype == torch.bool and memory_padding_mask.is_cuda
            and tuple(memory_padding_mask.shape) == tuple(memory.shape[:2]) and memory_padding_mask.stride(1) == 1):
        return _LevelProposalsFn.apply(memory, memory_padding_mask, level_hw[0])
    return proposals_composition(memory, memory_padding_mask, level_hw)


# ---- selection ----------------------------------------------------------------------------------------------------------------
def select_composition(enc_outputs_class, hand_coord, obj_coord, obj_classes=OBJ_CLASSES, left=LEFT_CLASS, right=RIGHT_CLASS):
    """(indices [N, 3] (left, right, object), reference_points [N, 3, 2]): the reference's selection (:202-224) in its own
    torch ops, boolean-mask loop (and its host syncs) included."""
    bs = enc_outputs_class.shape[0]
    device = enc_outputs_class.device
    best_score = torch.zeros(bs).to(device)
    obj_idx = torch.zeros(bs).to(device).to(torch.long)
    for i in range(obj_classes[0], obj_classes[1] + 1):
        score, idx = torch.max(enc_outputs_class[:, :, i], dim=-1)
        obj_idx[best_score < score] = idx[best_score < score]
        best_score[best_score < score] = score[best_score < score]
    left_idx = torch.argmax(enc_outputs_class[:, :, left], dim=-1)
    right_idx = torch.argmax(enc_outputs_class[:, :, right], dim=-1)
    left_kp = torch.gather(hand_coord, 1, left_idx.unsqueeze(1).unsqueeze(1).repeat(1, 1, 63))
    right_kp = torch.gather(hand_coord, 1, right_idx.unsqueeze(1).unsqueeze(1).repeat(1, 1, 63))
    obj_kp = torch.gather(obj_coord, 1, obj_idx.unsqueeze(1).unsqueeze(1).repeat(1, 1, 63))
    topk_coords_unact = torch.cat([left_kp, right_kp, obj_kp], dim=1).detach()
    reference_points = topk_coords_unact.sigmoid()
    ref_x = reference_points[..., 0::3].mean(-1).unsqueeze(-1)
    ref_y = reference_points[..., 1::3].mean(-1).unsqueeze(-1)
    return torch.stack([left_idx, right_idx, obj_idx], 1), torch.cat([ref_x, ref_y], dim=-1)


def select_queries(enc_outputs_class, hand_coord, obj_coord, obj_classes=OBJ_CLASSES, left=LEFT_CLASS, right=RIGHT_CLASS,
                   return_indices=False):
    """reference_points [N, 3, 2] (+ the selected rows [N, 3] — left, right, object — with return_indices), detached.  Raises
    IndexError when a class index is not below the number of classes, as the reference does."""
    ts = (enc_outputs_class, hand_coord, obj_coord)
    if (_plain_cuda_f32(*ts) and enc_outputs_class.dim() == 3 and enc_outputs_class.shape[1] > 0
            and all(tuple(t.shape) == tuple(enc_outputs_class.shape[:2]) + (63,) for t in ts[1:])
            and obj_classes[1] - obj_classes[0] < 14 and 0 <= min(obj_classes[0], left, right)):
        idx, refp = MSDA.assembly_select(*(t.detach().contiguous() for t in ts), obj_classes, left, right)
    else:
        idx, refp = select_composition(*ts, obj_classes, left, right)
    return (refp, idx) if return_indices else refp
