"""The set criteria of UVHand (models/actic_detr.py SetArcticCriterion :365-569, models/assembly_detr.py SetAssemblyCriterion
:248-446) over the device result of ``matcher.match`` (csrc/msda_criterion.hip, include/msda.h).

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


class _SetLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *preds):
        n = meta["sets"]
        logits, heads = list(preds[:n]), [list(preds[n * (i + 1):n * (i + 2)]) for i in range(len(preds) // n - 1)]
        hand = heads[0] if heads else None
        obj = heads[1] if len(heads) > 1 else None
        losses, stats = MSDA.criterion_fwd(meta["kind"], logits, hand, obj, *meta["args"])
        ctx.meta, ctx.stats = meta, stats
        ctx.save_for_backward(*preds)
        ctx.mark_non_differentiable(stats)
        return losses, stats

    @staticmethod
    def backward(ctx, grad_losses, _grad_stats):
        meta, n = ctx.meta, ctx.meta["sets"]
        preds = ctx.saved_tensors
        logits, heads = list(preds[:n]), [list(preds[n * (i + 1):n * (i + 2)]) for i in range(len(preds) // n - 1)]
        hand = heads[0] if heads else None
        obj = heads[1] if len(heads) > 1 else None
        g_logits, g_hand, g_obj = MSDA.criterion_bwd(meta["kind"], logits, hand, obj, *meta["args"],
                                                     grad_losses.contiguous(), ctx.stats)
        return (None, *g_logits, *g_hand, *g_obj)


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
    meta = {"sets": len(logits), "kind": MSDA.CRIT_ARCTIC if arctic else MSDA.CRIT_ASSEMBLY,
            "args": (result.buffer, packed.t_max, packed.labels, packed.keypoints, packed.offsets,
                     packed.is_valid if arctic else None, joint_valid if not arctic else None,
                     _hand_mask(ARCTIC_HANDS if arctic else hand_idx), _num_boxes_tensor(num_boxes, dev),
                     float(focal_alpha))}
    losses, stats = _SetLossFunction.apply(meta, *preds)
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


def arctic_set_losses(outputs, targets, indices, num_boxes, losses, num_classes, focal_alpha=0.25):
    """One ARCTIC set's DETR terms from the matcher's host ``indices`` (or 0: every requested key 0, not omitted)."""
    if not isinstance(indices, list):
        zero = outputs["pred_logits"].new_zeros(())
        return {k: zero for k in _arctic_keys(losses)}
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
        elif loss == "boxes":
            tgt = torch.cat([targets["keypoints"][f][indices[k][1]] for k, f in enumerate(valid)]).to(dev)
            hand = (matched == ARCTIC_HANDS[0]) + (matched == ARCTIC_HANDS[1])
            l_hand = F.l1_loss(outputs["pred_hand_key"][idx][hand], tgt[hand], reduction="none")
            l_obj = F.l1_loss(outputs["pred_obj_key"][idx][~hand], tgt[~hand], reduction="none")
            n_hand = int(hand.sum())
            out["loss_hand_keypoint"] = (l_hand.sum() / n_hand) / KEYPOINT_DIV if len(l_hand) else logits.new_zeros(())
            out["loss_obj_keypoint"] = (l_obj.sum() / int((~hand).sum())) / KEYPOINT_DIV
        elif loss == "cardinality":
            out["cardinality_error"] = _cardinality(logits, [len(t) for t in targets["labels"]], 0)
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


def _arctic_keys(losses):
    keys = []
    for loss in losses:
        keys += {"labels": ["loss_ce"], "boxes": ["loss_hand_keypoint", "loss_obj_keypoint"],
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
