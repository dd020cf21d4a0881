"""The set criteria of UVHand (models/actic_detr.py SetArcticCriterion :365-569, models/assembly_detr.py SetAssemblyCriterion
:248-446, models/dino/dino.py SetCriterion :428-781) over the device result of ``matcher.match`` (csrc/msda_criterion.hip,
csrc/msda_criterion_dino.hip, include/msda.h).

The reference turns every set's (final, aux, interm / enc) CPU index lists into index tensors, masks with booleans (a
``nonzero`` and a host sync each), reads counts with ``.item()`` and launches some 15-25 small kernels per set, as many
again backward.  Here:

  * ``set_losses(outputs_list, packed, result, num_boxes)``  every set's matched losses from ``match``'s padded device
    indices in ONE forward launch and ONE backward launch, no host sync (graph-capturable): a ``[sets, 4]`` fp32 tensor
    (columns ``ARCTIC_TERMS`` / ``ASSEMBLY_TERMS``); the backward takes that tensor's gradient, so loss weights apply on
    the device.
  * ``SetArcticCriterion`` / ``SetAssemblyCriterion``  drop-ins: the reference's constructor and ``forward``, the same loss
    dict keys.  A step is one ``match`` over all sets, one loss launch, ``num_boxes`` from host lengths (``all_reduce``d
    and clamped on the device under torch.distributed); the values are 0-d device views.  The AssemblyHands forward makes
    no host sync; the ARCTIC one makes none besides the MANO / ARCTIC small losses, which stay the reference's code
    (``small_loss``) unless ``small_loss`` is a ``small_loss.ArcticSmallLoss``, whose ``many`` covers every set sync-free.

  * ``dino_set_losses`` / ``SetDinoCriterion``  DINO's criterion: sets that differ in query count in one node, the
    matched final / aux / interm sets followed by the denoising sets, whose fixed pairs (dino.py:623-633) need no matcher;
    the empty class is K - 1; two forward launches (chunks, then a finish) and one backward launch, no host sync.

Reference behaviour kept: slot k of a set pairs output frame k with the k-th VALID frame's targets (ARCTIC, as the matcher);
AssemblyHands' ``joint_valid`` rows go with matched rows in query order (row r of a frame's matched block uses the frame's
joint_valid row r, not that of its target); ARCTIC ``loss_hand_keypoint`` is 0 without a matched hand and
``loss_obj_keypoint`` 0 / 0 = nan without a matched object; AssemblyHands ``enc_outputs`` raises the reference's
IndexError (its binarised label 0 is never a hand) before anything is launched.

Changed on purpose: the reference omits a set's ARCTIC DETR keys when its matcher returns 0 (no valid frame has a label);
the drop-in returns every key with the value 0, so all ranks of a DDP job report the same keys.

The one deviation: where the reference raises the IndexError of its joint_valid mask (an AssemblyHands matched label
outside ``hand_idx``, or a frame with unmatched targets), the fused path cannot know without a sync.  It sets that set's
status bit and returns nan for its ``loss_hand_keypoint``; ``MSDA_CRITERION_CHECK=1`` syncs once per step and raises the
reference's error (and the matcher's errors) instead.

The package's torch restatement of the reference's maths (``arctic_set_losses`` / ``assembly_set_losses``, per-set host
indices) runs instead for CPU tensors, non-fp32 predictions (bf16 autocast heads), anything over the matcher's limits
(Q > 1024, more than 16 targets in a frame, more than 16 sets) and with ``MSDA_CRITERION_FUSED=0`` (A/B knob)."""
import copy
import functools
import os
from typing import NamedTuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _native as MSDA
from . import matcher as MT

ARCTIC_TERMS = ("loss_ce", "loss_hand_keypoint", "loss_obj_keypoint", "cardinality_error")
ASSEMBLY_TERMS = ("loss_ce", "loss_hand_keypoint", "cardinality_error", "class_error")
ARCTIC_HANDS = (12, 13)
KEYPOINT_DIV = 21


def _fused_enabled():
    return os.environ.get("MSDA_CRITERION_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatement


def _check_enabled():
    return os.environ.get("MSDA_CRITERION_CHECK", "0") not in ("", "0")


class SetLosses(NamedTuple):
    """``set_losses``' result."""
    losses: torch.Tensor    # [sets, 4] fp32, columns ``names``
    names: tuple
    status: torch.Tensor    # [sets] int32 status bits (include/msda.h; 0 = ok)
    stats: torch.Tensor     # [sets, 4] int32: status, matched hand rows, matched object rows, no valid target (ARCTIC)


def pack_joint_valid(targets, device):
    """AssemblyHands' per-target ``joint_valid`` ([T_k, 21, 3] bool per frame) as one uint8 [n, 63] device tensor, in
    target order (``torch.cat`` on the device; no sync)."""
    device = torch.device(device)
    parts = [v["joint_valid"].to(device, non_blocking=True).flatten(1) for v in targets]   # (a frame may have no target)
    return torch.cat(parts).to(torch.uint8).contiguous()


def _hand_mask(labels):
    mask = 0
    for lab in labels:
        if not 0 <= int(lab) < 64:
            raise ValueError("set_losses: hand labels must lie in [0, 64)")
        mask |= 1 << int(lab)
    return mask


def _split_preds(sets, preds):
    """(logits, hand, obj) lists of a node's flat ``preds`` (the sets' logits, then each keypoint head's; None: no such head)."""
    heads = [list(preds[i:i + sets]) for i in range(0, len(preds), sets)] + [None, None]
    return heads[0], heads[1], heads[2]


class _SetLossNode(torch.autograd.Function):
    """One criterion's losses as an autograd node over ``fwd`` / ``bwd``, its pair of ``_native`` functions: both take
    (logits, hand, obj, *args), ``bwd`` the losses' gradient and the forward's stats after them."""

    @staticmethod
    def forward(ctx, fwd, bwd, sets, args, *preds):
        losses, stats = fwd(*_split_preds(sets, preds), *args)
        ctx.bwd, ctx.sets, ctx.args, ctx.stats = bwd, sets, args, stats
        ctx.save_for_backward(*preds)
        ctx.mark_non_differentiable(stats)
        return losses, stats

    @staticmethod
    def backward(ctx, grad_losses, _grad_stats):
        grads = ctx.bwd(*_split_preds(ctx.sets, ctx.saved_tensors), *ctx.args, grad_losses.contiguous(), ctx.stats)
        return (None, None, None, None, *grads[0], *grads[1], *grads[2])


def _num_boxes_tensor(num_boxes, device):
    if torch.is_tensor(num_boxes):
        return num_boxes.to(device=device, dtype=torch.float32).reshape(1).contiguous()
    return torch.full((1,), float(num_boxes), dtype=torch.float32, device=device)


def set_losses(outputs_list, packed, result, num_boxes, kind=None, focal_alpha=0.25, hand_idx=(1, 2), joint_valid=None):
    """The matched losses of every prediction dict of ``outputs_list`` (the sets ``match`` was given, same order) in one
    launch, differentiable through one backward launch, with no host sync.  ``packed``: ``matcher.pack_targets``;
    ``result``: ``matcher.match``'s MatchResult; ``num_boxes``: a device scalar (or a number).  ``kind`` defaults to
    ``packed.kind``.  ARCTIC: hands are labels 12 / 13; AssemblyHands: labels in ``hand_idx``, and ``joint_valid`` is
    ``pack_joint_valid(targets)`` (needed with target keypoints).  Returns ``SetLosses``."""
    kind = kind or packed.kind
    arctic = kind == "arctic"
    if kind not in ("arctic", "assembly"):
        raise ValueError("set_losses: kind must be 'arctic' or 'assembly'")
    logits = [o["pred_logits"].contiguous() for o in outputs_list]
    dev = logits[0].device
    has_kp = packed.keypoints is not None
    preds = list(logits)
    if has_kp and arctic:
        preds += [o["pred_hand_key"].contiguous() for o in outputs_list]
        preds += [o["pred_obj_key"].contiguous() for o in outputs_list]
    elif has_kp:
        preds += [o["pred_keypoints"].contiguous() for o in outputs_list]
        if joint_valid is None:
            raise ValueError("set_losses: AssemblyHands needs joint_valid (pack_joint_valid)")
    kind = MSDA.CRIT_ARCTIC if arctic else MSDA.CRIT_ASSEMBLY
    args = (result.buffer, packed.t_max, packed.labels, packed.keypoints, packed.offsets,
            packed.is_valid if arctic else None, joint_valid if not arctic else None,
            _hand_mask(ARCTIC_HANDS if arctic else hand_idx), _num_boxes_tensor(num_boxes, dev), float(focal_alpha))
    losses, stats = _SetLossNode.apply(functools.partial(MSDA.criterion_fwd, kind), functools.partial(MSDA.criterion_bwd, kind),
                                       len(logits), args, *preds)
    return SetLosses(losses, ARCTIC_TERMS if arctic else ASSEMBLY_TERMS, stats[:, 0], stats)


def raise_on_status(result, out, sets, bs, t_max, n_targets, zero_if_empty=False):
    """``MSDA_CRITERION_CHECK=1``: one copy of the matcher's result and the stats to the host (the step's one sync), then
    the reference's error for the first set that has one: scipy's ValueError for a matcher status, IndexError for a label
    out of range or the AssemblyHands joint_valid mask mismatch."""
    host = torch.cat([result.buffer, out.stats.reshape(-1).to(torch.int64)]).cpu()
    buf, stats = host[:result.buffer.numel()], host[result.buffer.numel():].view(sets, 4).tolist()
    MT.indices_from_host(buf, sets, bs, t_max, zero_if_empty)          # raises the matcher's errors, sets in order
    for s in range(sets):
        st = stats[s][0]
        if st & MSDA.CRIT_BAD_LABEL:
            raise IndexError("a target label is out of bounds for the class dimension")
        if st & MSDA.CRIT_BAD_TARGETS:
            raise RuntimeError("criterion: target offsets do not describe the targets")
        if st & MSDA.CRIT_MASK_MISMATCH:
            raise IndexError("The shape of the mask [%d, 63] at index 0 does not match the shape of the indexed tensor "
                             "[%d, 63] at index 0" % (n_targets, stats[s][1]))


# ---- the torch restatement of the reference's maths (host indices; the fallback) ----------------------------------------
def sigmoid_focal_loss(inputs, targets, num_boxes, alpha=0.25, gamma=2):
    """RetinaNet's focal loss as DETR-style criteria use it: summed over classes and frames, averaged over queries, / num_boxes."""
    prob = inputs.sigmoid()
    ce = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = prob * targets + (1 - prob) * (1 - targets)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean(1).sum() / num_boxes


def _src_index(indices):
    batch = torch.cat([torch.full_like(i, k) for k, (i, _) in enumerate(indices)])
    return batch, torch.cat([i for i, _ in indices])


def _focal_ce(logits, idx, matched_labels, num_classes, num_boxes, alpha):
    cls = torch.full(logits.shape[:2], num_classes, dtype=torch.int64, device=logits.device)
    cls[idx] = matched_labels
    onehot = torch.zeros(logits.shape[:2] + (logits.shape[2] + 1,), dtype=logits.dtype, device=logits.device)
    onehot.scatter_(2, cls.unsqueeze(-1), 1)
    return sigmoid_focal_loss(logits, onehot[:, :, :-1], num_boxes, alpha=alpha, gamma=2) * logits.shape[1]


def _cardinality(logits, lengths, empty):
    card = (logits.argmax(-1) != empty).sum(1)
    return F.l1_loss(card.float(), torch.as_tensor(lengths, device=logits.device).float())


def _top1_error(logits, labels):
    if labels.numel() == 0:
        return 100 - torch.zeros([], device=logits.device)
    correct = logits.topk(1, 1, True, True)[1].t().eq(labels.view(1, -1)).view(-1).float().sum(0)
    return 100 - correct.mul_(100.0 / labels.size(0))


def arctic_set_losses(outputs, targets, indices, num_boxes, losses, num_classes, focal_alpha=0.25, empty=0, log=False):
    """One ARCTIC set's DETR terms from the matcher's host ``indices`` (or 0: every requested key 0, not omitted).  DINO's
    criterion is the same maths with the empty class ``empty`` = K - 1 and, for its final set (``log``), ``class_error``."""
    if not isinstance(indices, list):
        zero = outputs["pred_logits"].new_zeros(())
        return {k: zero for k in _arctic_keys(losses, log)}
    logits = outputs["pred_logits"]
    dev = logits.device
    valid = [f for f in range(len(targets["labels"])) if targets["is_valid"][f] == 1]
    idx = _src_index(indices)
    matched = torch.cat([torch.as_tensor(targets["labels"][f], dtype=torch.int64)[indices[k][1]]
                         for k, f in enumerate(valid)]).to(dev)
    out = {}
    for loss in losses:
        if loss == "labels":
            out["loss_ce"] = _focal_ce(logits, idx, matched, num_classes, num_boxes, focal_alpha)
            if log:
                out["class_error"] = _top1_error(logits[idx], matched)
        elif loss == "boxes":
            tgt = torch.cat([targets["keypoints"][f][indices[k][1]] for k, f in enumerate(valid)]).to(dev)
            hand = (matched == ARCTIC_HANDS[0]) + (matched == ARCTIC_HANDS[1])
            l_hand = F.l1_loss(outputs["pred_hand_key"][idx][hand], tgt[hand], reduction="none")
            l_obj = F.l1_loss(outputs["pred_obj_key"][idx][~hand], tgt[~hand], reduction="none")
            n_hand = int(hand.sum())
            out["loss_hand_keypoint"] = (l_hand.sum() / n_hand) / KEYPOINT_DIV if len(l_hand) else logits.new_zeros(())
            out["loss_obj_keypoint"] = (l_obj.sum() / int((~hand).sum())) / KEYPOINT_DIV
        elif loss == "cardinality":
            out["cardinality_error"] = _cardinality(logits, [len(t) for t in targets["labels"]], empty)
        else:
            raise AssertionError(f"do you really want to compute {loss} loss?")
    return out


def assembly_set_losses(outputs, targets, indices, num_boxes, losses, num_classes, hand_idx, focal_alpha=0.25, log=True):
    """One AssemblyHands set's terms from the matcher's host ``indices``; raises the reference's IndexError on a joint_valid
    mask mismatch."""
    logits = outputs["pred_logits"]
    idx = _src_index(indices)
    matched = torch.cat([t["labels"][j] for t, (_, j) in zip(targets, indices)])
    out = {}
    for loss in losses:
        if loss == "labels":
            out["loss_ce"] = _focal_ce(logits, idx, matched, num_classes, num_boxes, focal_alpha)
            if log:
                out["class_error"] = _top1_error(logits[idx], matched)
        elif loss == "cardinality":
            out["cardinality_error"] = _cardinality(logits, [len(v["labels"]) for v in targets], logits.shape[-1] - 1)
        elif loss == "hand_keypoint":
            jv = torch.cat([v["joint_valid"] for v in targets]).view(-1, 63)
            tgt = torch.cat([t["keypoints"][j] for t, (_, j) in zip(targets, indices)])
            hand = torch.zeros_like(matched, dtype=torch.bool)
            for lab in hand_idx:
                hand |= matched == lab
            l1 = F.l1_loss(outputs["pred_keypoints"][idx][hand], tgt[hand].view(-1, 63), reduction="none")[jv]
            out["loss_hand_keypoint"] = l1.sum() / KEYPOINT_DIV
        else:
            raise AssertionError(f"do you really want to compute {loss} loss?")
    return out


def _arctic_keys(losses, log=False):
    keys = []
    for loss in losses:
        keys += {"labels": ["loss_ce", "class_error"] if log else ["loss_ce"],
                 "boxes": ["loss_hand_keypoint", "loss_obj_keypoint"],
                 "cardinality": ["cardinality_error"]}.get(loss, [])
    return keys


# ---- the drop-ins --------------------------------------------------------------------------------------------------------
def _dist():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


def _num_boxes_device(n, device):
    """The reference's num_boxes on the device: all_reduce'd over ranks, / world size, clamped at 1; no .item()."""
    nb = torch.full((1,), float(n), dtype=torch.float32, device=device)
    world = 1
    if _dist():
        torch.distributed.all_reduce(nb)
        world = torch.distributed.get_world_size()
    return torch.clamp(nb / world, min=1)


def _num_boxes_host(n, device):
    nb = torch.as_tensor([n], dtype=torch.float, device=device)
    world = 1
    if _dist():
        torch.distributed.all_reduce(nb)
        world = torch.distributed.get_world_size()
    return torch.clamp(nb / world, min=1).item()


def _fusable(preds, sizes, bs, sets):
    return (_fused_enabled() and all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in preds)
            and len({t.device for t in preds}) == 1 and preds[0].dim() == 3 and 1 <= bs <= MSDA.MATCH_MAX_QUERIES
            and len(sizes) == bs and preds[0].shape[1] <= MSDA.MATCH_MAX_QUERIES
            and max(sizes, default=0) <= MSDA.MATCH_MAX_TARGETS and sets <= MSDA.MATCH_MAX_SETS)


class SetArcticCriterion(nn.Module):
    """Drop-in for models/actic_detr.py:365-569: ``forward(outputs, targets, args, meta_info)`` returns the reference's
    loss dict.  The DETR terms of the final, aux and interm sets come from one ``match`` and one loss launch; the MANO /
    ARCTIC terms come from ``small_loss(outputs, targets, meta_info, args, suffix)``, a dict whose keys carry the suffix
    ("" for the final set, "_{i}" for aux set i; default: the reference's
    ``get_arctic_item`` + ``compute_small_loss``, imported from ``arctic_tools`` on first use) for the final and aux sets."""

    def __init__(self, num_classes, matcher, weight_dict, losses, focal_alpha=0.25, cfg=None, pre_process_models=None,
                 small_loss=None):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.losses = losses
        self.focal_alpha = focal_alpha
        self.cfg = cfg
        self.pre_process_models = pre_process_models
        self.small_loss = small_loss

    def _small(self, outputs, targets, meta_info, args, suffix):
        if self.small_loss is None:
            from arctic_tools.process import get_arctic_item
            from arctic_tools.src.callbacks.loss.loss_arctic_sf import compute_small_loss

            def reference_small_loss(out, tgt, meta, a, sfx):
                d = compute_small_loss(get_arctic_item(out, self.cfg, a.device), tgt, meta, self.pre_process_models,
                                       a.img_res)
                return {k + sfx: v for k, v in d.items()}
            self.small_loss = reference_small_loss
        return self.small_loss(outputs, targets, meta_info, args, suffix)

    def _small_many(self, final, aux, targets, meta_info, args):
        """Every set's small-loss dict from one ``small_loss.many(...)`` call (``ArcticSmallLoss``), or None when the
        ``small_loss`` has no callable ``many`` (the per-set calls then run as before)."""
        many = getattr(self.small_loss, "many", None)
        if not callable(many):
            return None
        return many([final] + aux, targets, meta_info, args, [""] + [f"_{i}" for i in range(len(aux))])

    @staticmethod
    def _sets(outputs):
        final = {k: v for k, v in outputs.items() if k not in ("aux_outputs", "interm_outputs")}
        aux = list(outputs.get("aux_outputs", []))
        return final, aux, outputs.get("interm_outputs")

    def forward(self, outputs, targets, args, meta_info):
        final, aux, interm = self._sets(outputs)
        sets = [final] + aux + ([interm] if interm is not None else [])
        has_kp = "keypoints" in targets
        preds = [o["pred_logits"] for o in sets]
        if has_kp:
            preds += [o[k] for o in sets for k in ("pred_hand_key", "pred_obj_key")]
        sizes = [len(t) for t in targets["labels"]]
        kps = list(targets["keypoints"]) if has_kp else []
        bs = final["pred_logits"].shape[0]
        if not (_fusable(preds, sizes, bs, len(sets)) and set(self.losses) <= {"labels", "boxes", "cardinality"}
                and ("boxes" not in self.losses or has_kp)
                and all(torch.is_tensor(k) and k.dtype == torch.float32 and k.shape[-1] == preds[-1].shape[-1]
                        for k in kps)):
            return self._forward_reference(outputs, targets, args, meta_info)
        dev = final["pred_logits"].device
        packed = MT.pack_targets(targets, dev)
        result = MT.match(sets, packed, self.matcher.cost_class, self.matcher.cost_keypoint)
        nb = _num_boxes_device(sum(sizes), dev)
        out = set_losses(sets, packed, result, nb, "arctic", self.focal_alpha)
        if _check_enabled():
            raise_on_status(result, out, len(sets), bs, packed.t_max, int(packed.labels.shape[0]))
        L = out.losses
        col = {name: c for c, name in enumerate(ARCTIC_TERMS)}
        keys = _arctic_keys(self.losses)
        losses = {k: L[0, col[k]] for k in keys}
        small = self._small_many(final, aux, targets, meta_info, args)
        losses.update(small[0] if small else self._small(final, targets, meta_info, args, ""))
        for i, a in enumerate(aux):
            losses.update({k + f"_{i}": L[1 + i, col[k]] for k in keys})
            losses.update(small[1 + i] if small else self._small(a, targets, meta_info, args, f"_{i}"))
        if interm is not None:
            losses.update({k + "_interm": L[len(sets) - 1, col[k]] for k in keys})
        return losses

    def _forward_reference(self, outputs, targets, args, meta_info):
        """The torch restatement: the matcher per set, host indices, the reference's maths."""
        final, aux, interm = self._sets(outputs)
        kw = dict(losses=self.losses, num_classes=self.num_classes, focal_alpha=self.focal_alpha)
        nb = _num_boxes_host(sum(len(t) for t in targets["labels"]), final["pred_logits"].device)
        losses = dict(arctic_set_losses(final, targets, self.matcher(final, targets), nb, **kw))
        small = self._small_many(final, aux, targets, meta_info, args)
        losses.update(small[0] if small else self._small(final, targets, meta_info, args, ""))
        for i, a in enumerate(aux):
            losses.update({k + f"_{i}": v for k, v in arctic_set_losses(a, targets, self.matcher(a, targets), nb,
                                                                          **kw).items()})
            losses.update(small[1 + i] if small else self._small(a, targets, meta_info, args, f"_{i}"))
        if interm is not None:
            losses.update({k + "_interm": v for k, v in arctic_set_losses(interm, targets, self.matcher(interm, targets),
                                                                           nb, **kw).items()})
        return losses


class SetAssemblyCriterion(nn.Module):
    """Drop-in for models/assembly_detr.py:248-446: ``forward(outputs, targets)`` returns the reference's loss dict; targets
    carry ``joint_valid`` ([T_k, 21, 3] bool, added by the training loop).  The final and aux sets take one ``match`` and one
    loss launch and no host sync."""

    def __init__(self, num_classes, matcher, weight_dict, losses, focal_alpha=0.25, cfg=None):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.losses = losses
        self.focal_alpha = focal_alpha
        self.cfg = cfg

    @property
    def hand_idx(self):
        return tuple(self.cfg.hand_idx) if self.cfg is not None else (1, 2)

    def forward(self, outputs, targets):
        final = {k: v for k, v in outputs.items() if k not in ("aux_outputs", "enc_outputs")}
        aux = list(outputs.get("aux_outputs", []))
        n_targets = sum(len(t["labels"]) for t in targets)
        if "enc_outputs" in outputs and n_targets > 0:
            # binarised to label 0, never in hand_idx: the reference's joint_valid mask cannot match a non-empty batch
            n_hand = sum(len(t["labels"]) for t in targets) if 0 in self.hand_idx else 0
            if "hand_keypoint" in self.losses and n_hand != n_targets:
                raise IndexError("The shape of the mask [%d, 63] at index 0 does not match the shape of the indexed "
                                 "tensor [%d, 63] at index 0" % (n_targets, n_hand))
        sets = [final] + aux + ([outputs["enc_outputs"]] if "enc_outputs" in outputs else [])
        preds = [o["pred_logits"] for o in sets] + [o["pred_keypoints"] for o in sets]
        sizes = [len(v["keypoints"]) for v in targets]
        bs = final["pred_logits"].shape[0]
        if not (_fusable(preds, sizes, bs, len(sets)) and set(self.losses) <= {"labels", "cardinality", "hand_keypoint"}
                and preds[-1].shape[-1] == 63 and ("enc_outputs" not in outputs or n_targets == 0)
                and all(torch.is_tensor(v["keypoints"]) and v["keypoints"].numel() == 63 * len(v["keypoints"])
                        and torch.is_tensor(v.get("joint_valid")) and v["joint_valid"].numel() == 63 * len(v["keypoints"])
                        for v in targets)):
            return self._forward_reference(outputs, targets)
        dev = final["pred_logits"].device
        packed = MT.pack_targets(targets, dev)
        result = MT.match(sets, packed, self.matcher.cost_class, self.matcher.cost_keypoint)
        nb = _num_boxes_device(n_targets, dev)
        out = set_losses(sets, packed, result, nb, "assembly", self.focal_alpha, self.hand_idx,
                         pack_joint_valid(targets, dev))
        if _check_enabled():
            raise_on_status(result, out, len(sets), bs, packed.t_max, int(packed.labels.shape[0]))
        L = out.losses
        losses = {}
        for s, o in enumerate(sets):
            sfx = "" if s == 0 else ("_enc" if o is outputs.get("enc_outputs") else f"_{s - 1}")
            for loss in self.losses:
                if loss == "labels":
                    losses["loss_ce" + sfx] = L[s, 0]
                    if s == 0:
                        losses["class_error"] = L[0, 3]
                elif loss == "cardinality":
                    losses["cardinality_error" + sfx] = L[s, 2]
                else:
                    losses["loss_hand_keypoint" + sfx] = L[s, 1]
        return losses

    def _forward_reference(self, outputs, targets):
        final = {k: v for k, v in outputs.items() if k not in ("aux_outputs", "enc_outputs")}
        kw = dict(losses=self.losses, num_classes=self.num_classes, hand_idx=self.hand_idx, focal_alpha=self.focal_alpha)
        nb = _num_boxes_host(sum(len(t["labels"]) for t in targets), final["pred_logits"].device)
        losses = dict(assembly_set_losses(final, targets, self.matcher(final, targets), nb, **kw))
        for i, a in enumerate(outputs.get("aux_outputs", [])):
            d = assembly_set_losses(a, targets, self.matcher(a, targets), nb, log=False, **kw)
            losses.update({k + f"_{i}": v for k, v in d.items()})
        if "enc_outputs" in outputs:
            enc = outputs["enc_outputs"]
            bin_targets = copy.deepcopy(targets)
            for bt in bin_targets:
                bt["labels"] = torch.zeros_like(bt["labels"])
            d = assembly_set_losses(enc, bin_targets, self.matcher(enc, bin_targets), nb, log=False, **kw)
            losses.update({k + "_enc": v for k, v in d.items()})
        return losses


# ---- DINO (models/dino/dino.py SetCriterion :428-781): matched sets and denoising sets in one node ------------------------
DINO_ZERO_DN_KEYS = ("loss_bbox_dn", "loss_giou_dn", "loss_ce_dn", "loss_xy_dn", "loss_hw_dn", "cardinality_error_dn")
_PRED_KEYS = ("pred_logits", "pred_hand_key", "pred_obj_key")


def dino_set_losses(outputs_list, packed, result, num_boxes, dn_outputs_list=(), single_pad=0, groups=0, focal_alpha=0.25):
    """DINO's matched losses of every prediction dict of ``outputs_list`` (the sets ``match`` was given, same order) followed
    by the denoising losses of every dict of ``dn_outputs_list`` ([bs, groups * single_pad, .] predictions, paired with the
    targets as dino.py:623-633 does), in one autograd node: two forward launches, one backward launch, no host sync.
    ``packed``: ``matcher.pack_targets`` of the ARCTIC targets dict; ``result``: ``matcher.match``'s MatchResult (None
    without matched sets); ``num_boxes``: a device scalar (or a number); a denoising set divides its focal loss by
    ``num_boxes * groups``.  Returns ``SetLosses`` with ``len(outputs_list) + len(dn_outputs_list)`` rows in ``ARCTIC_TERMS``
    order; the empty class is K - 1."""
    matched, dn = list(outputs_list), list(dn_outputs_list)
    if packed.kind != "arctic":
        raise ValueError("dino_set_losses: the targets are the ARCTIC dict (labels, keypoints, is_valid)")
    if not matched and not dn:
        raise ValueError("dino_set_losses: no prediction set")
    if matched and result is None:
        raise ValueError("dino_set_losses: matched sets need matcher.match's result")
    logits = [o["pred_logits"].contiguous() for o in matched + dn]
    preds = list(logits)
    if packed.keypoints is not None:
        preds += [o["pred_hand_key"].contiguous() for o in matched + dn]
        preds += [o["pred_obj_key"].contiguous() for o in matched + dn]
    match_sets = int(result.count.shape[0]) if result is not None else 0
    if len(matched) > match_sets:
        raise ValueError("dino_set_losses: %d matched sets, the match result has %d" % (len(matched), match_sets))
    args = ([*range(len(matched))] + [-1] * len(dn), result.buffer if result is not None else None, match_sets,
            packed.t_max, packed.labels, packed.keypoints, packed.offsets, packed.is_valid, _hand_mask(ARCTIC_HANDS),
            _num_boxes_tensor(num_boxes, logits[0].device), float(focal_alpha), int(single_pad), int(groups))
    losses, stats = _SetLossNode.apply(MSDA.criterion_dino_fwd, MSDA.criterion_dino_bwd, len(logits), args, *preds)
    return SetLosses(losses, ARCTIC_TERMS, stats[:, 0], stats)


def _class_error_device(logits, packed, result, none_flag, set_index=0):
    """``100 - accuracy(src_logits[idx], target_classes_o)[0]`` of one matched set from the device match result: torch ops,
    no host sync.  0 where ``none_flag`` (no valid frame has a target) is set."""
    bs, Q, _ = logits.shape
    W, n = packed.t_max, int(packed.labels.shape[0])
    if W == 0 or n == 0:
        return logits.new_zeros(())
    dev = logits.device
    order = torch.argsort((packed.is_valid == 0).to(torch.int8), stable=True)      # slot k -> the k-th valid frame
    mask = torch.arange(W, device=dev)[None, :] < result.count[set_index][:, None]
    q = result.query_idx[set_index].clamp(0, Q - 1)
    rows = (packed.offsets[:-1][order][:, None] + result.target_idx[set_index].clamp(min=0)).clamp(0, n - 1)
    pred = logits.detach().argmax(-1).gather(1, q)
    correct = ((pred == packed.labels[rows]) & mask).sum().to(torch.float32)
    pairs = mask.sum()
    scale = (100.0 / pairs.to(torch.float64)).to(torch.float32)                     # accuracy: correct.mul_(100.0 / n)
    err = torch.where(pairs > 0, 100 - correct * scale, torch.full_like(correct, 100.0))
    return torch.where(none_flag != 0, torch.zeros_like(err), err)


class SetDinoCriterion(SetArcticCriterion):
    """Drop-in for models/dino/dino.py:428-781 (``loss_masks`` left out): the reference's constructor order and
    ``forward(outputs, targets, args, meta_info, return_indices=False)``, returning the reference's dict in the reference's
    key order.  The final, aux and interm sets and the denoising set of ``outputs['dn_meta']`` take one ``pack_targets``, one
    ``match`` and one ``dino_set_losses``; values are 0-d views of its tensor; ``class_error`` comes from the match result
    with torch ops; no host sync (``return_indices=True`` copies the match buffer once).  Without denoising outputs (not
    training, falsy ``dn_meta``, no ``output_known_lbs_bboxes``) the reference's six zero keys are returned and no
    denoising set is launched.  When no valid frame has a target every key is 0 (the reference's matcher raises).
    ``enc_outputs`` without keypoint heads raise the reference's ``loss_boxes`` assertion before anything is launched."""

    def __init__(self, num_classes, matcher, weight_dict, focal_alpha, losses, cfg, pre_process_models, small_loss=None):
        super().__init__(num_classes, matcher, weight_dict, losses, focal_alpha, cfg, pre_process_models, small_loss)

    @staticmethod
    def _sets(outputs):
        skip = ("aux_outputs", "interm_outputs", "enc_outputs", "dn_meta")
        final = {k: v for k, v in outputs.items() if k not in skip}
        return final, list(outputs.get("aux_outputs", [])), outputs.get("interm_outputs")

    def _dn(self, outputs):
        """(output_known_lbs_bboxes, single_pad, groups) as ``prep_for_dn`` (:775-781), or None: the six zero keys."""
        dn_meta = outputs["dn_meta"]
        if not (self.training and dn_meta and "output_known_lbs_bboxes" in dn_meta):
            return None
        groups, pad = dn_meta["num_dn_group"], dn_meta["pad_size"]
        assert pad % groups == 0
        return dn_meta["output_known_lbs_bboxes"], pad // groups, groups

    def _fused_ok(self, sets, dn, targets):
        has_kp = "keypoints" in targets
        keys = _PRED_KEYS if has_kp else _PRED_KEYS[:1]
        if not all(k in o for o in sets + ([dn[0]] if dn else []) for k in keys):
            return False
        preds = [o[k] for k in keys for o in sets]
        sizes = [len(t) for t in targets["labels"]]
        kps = list(targets["keypoints"]) if has_kp else []
        bs = sets[0]["pred_logits"].shape[0]
        if not (_fusable(preds, sizes, bs, len(sets) + (1 if dn else 0))
                and all(t.shape[:2] == preds[0].shape[:2] for t in preds)
                and set(self.losses) <= {"labels", "boxes", "cardinality"} and ("boxes" not in self.losses or has_kp)
                and getattr(self.matcher, "focal_alpha", MT.ALPHA) == MT.ALPHA
                and all(torch.is_tensor(k) and k.dtype == torch.float32 and k.shape[-1] == preds[-1].shape[-1] for k in kps)):
            return False
        if dn:
            known, single_pad, groups = dn
            dn_preds = [known[k] for k in keys]
            if not (all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.device == preds[0].device
                        and t.dim() == 3 and tuple(t.shape[:2]) == (bs, groups * single_pad) for t in dn_preds)
                    and groups >= 1 and single_pad >= 2 and single_pad % 2 == 0 and max(sizes, default=0) <= single_pad // 2):
                return False
        return True

    def forward(self, outputs, targets, args, meta_info, return_indices=False):
        final, aux, interm = self._sets(outputs)
        if "boxes" in self.losses:
            for enc in outputs.get("enc_outputs", ()):       # the reference's loss_boxes assertion, before any launch
                assert "pred_hand_key" in enc and "pred_obj_key" in enc
        dn = self._dn(outputs)
        sets = [final] + aux + ([interm] if interm is not None else [])
        if "enc_outputs" in outputs or not self._fused_ok(sets, dn, targets):
            return self._forward_reference(outputs, targets, args, meta_info, return_indices)
        dev = final["pred_logits"].device
        bs = final["pred_logits"].shape[0]
        packed = MT.pack_targets(targets, dev)
        result = MT.match(sets, packed, self.matcher.cost_class, self.matcher.cost_keypoint)
        nb = _num_boxes_device(sum(packed.sizes), dev)
        out = dino_set_losses(sets, packed, result, nb, [dn[0]] if dn else [], dn[1] if dn else 0, dn[2] if dn else 0,
                              self.focal_alpha)
        if _check_enabled():
            self._raise_on_status(result, out, len(sets), bs, packed.t_max)
        L = out.losses
        col = {name: c for c, name in enumerate(ARCTIC_TERMS)}
        keys = _arctic_keys(self.losses)
        if dn:
            losses = {k + "_dn": L[len(sets), col[k]] for k in keys}
        else:
            zero = torch.zeros((), device=dev)
            losses = {k: zero for k in DINO_ZERO_DN_KEYS}
        for k in _arctic_keys(self.losses, log=True):
            losses[k] = (_class_error_device(final["pred_logits"], packed, result, out.stats[0, 3]) if k == "class_error"
                         else L[0, col[k]])
        small = self._small_many(final, aux, targets, meta_info, args)
        losses.update(small[0] if small else self._small(final, targets, meta_info, args, ""))
        for i in range(len(aux)):
            losses.update({k + f"_{i}": L[1 + i, col[k]] for k in keys})
            losses.update(small[1 + i] if small else self._small(aux[i], targets, meta_info, args, f"_{i}"))
        if interm is not None:
            losses.update({k + "_interm": L[len(sets) - 1, col[k]] for k in keys})
        if return_indices:
            per_set = MT.indices_from_host(result.buffer.cpu(), len(sets), bs, packed.t_max, zero_if_empty=True)
            return losses, per_set[1:] + per_set[:1]         # the reference's order: aux..., interm, final
        return losses

    @staticmethod
    def _raise_on_status(result, out, match_sets, bs, t_max):
        """``MSDA_CRITERION_CHECK=1``: one copy to the host (the step's one sync), then the reference's error."""
        rows = out.stats.shape[0]
        host = torch.cat([result.buffer, out.stats.reshape(-1).to(torch.int64)]).cpu()
        buf, stats = host[:result.buffer.numel()], host[result.buffer.numel():].view(rows, 4).tolist()
        MT.indices_from_host(buf, match_sets, bs, t_max, True)
        for st, *_ in stats:
            if st & MSDA.CRIT_BAD_LABEL:
                raise IndexError("a target label is out of bounds for the class dimension")
            if st & MSDA.CRIT_BAD_TARGETS:
                raise RuntimeError("criterion: target offsets do not describe the targets")

    def _forward_reference(self, outputs, targets, args, meta_info, return_indices=False):
        """The torch restatement: the matcher per set, host indices, the denoising index lists of :620-634, host num_boxes."""
        if "masks" in self.losses:
            raise NotImplementedError("SetDinoCriterion: loss_masks is left out")
        final, aux, interm = self._sets(outputs)
        dev = final["pred_logits"].device

        def terms(o, indices, num_boxes, log=False):
            return arctic_set_losses(o, targets, indices, num_boxes, losses=self.losses, num_classes=self.num_classes,
                                     focal_alpha=self.focal_alpha, empty=o["pred_logits"].shape[-1] - 1, log=log)

        indices0 = self.matcher(final, targets)
        indices_list = []
        nb = _num_boxes_host(sum(len(t) for t in targets["labels"]), dev)
        dn = self._dn(outputs)
        if dn:
            known, single_pad, scalar = dn
            dn_pos_idx = 0
            if isinstance(indices0, list):
                dn_pos_idx = []
                for f in range(len(targets["labels"])):
                    if targets["is_valid"][f] != 1:
                        continue
                    t = torch.arange(len(targets["labels"][f]), dtype=torch.int64).unsqueeze(0).repeat(scalar, 1)
                    out_idx = (torch.arange(scalar, dtype=torch.int64) * single_pad).unsqueeze(1) + t
                    dn_pos_idx.append((out_idx.flatten(), t.flatten()))
            losses = {k + "_dn": v for k, v in terms(known, dn_pos_idx, nb * scalar).items()}
        else:
            zero = torch.zeros((), device=dev)
            losses = {k: zero for k in DINO_ZERO_DN_KEYS}
        losses.update(terms(final, indices0, nb, log=True))
        small = self._small_many(final, aux, targets, meta_info, args)
        losses.update(small[0] if small else self._small(final, targets, meta_info, args, ""))
        for i, a in enumerate(aux):
            indices = self.matcher(a, targets)
            indices_list.append(indices)
            losses.update({k + f"_{i}": v for k, v in terms(a, indices, nb).items()})
            losses.update(small[1 + i] if small else self._small(a, targets, meta_info, args, f"_{i}"))
        if interm is not None:
            indices = self.matcher(interm, targets)
            indices_list.append(indices)
            losses.update({k + "_interm": v for k, v in terms(interm, indices, nb).items()})
        for i, enc in enumerate(outputs.get("enc_outputs", ())):
            indices = self.matcher(enc, targets)
            indices_list.append(indices)
            losses.update({k + f"_enc_{i}": v for k, v in terms(enc, indices, nb).items()})
        if return_indices:
            return losses, indices_list + [indices0]
        return losses
