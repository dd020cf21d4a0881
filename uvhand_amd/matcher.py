"""The Hungarian matchers of UVHand's criterion (models/matcher.py: ArcticMatcher :20-125, AssemblyMatcher :128-230) on HIP
(csrc/msda_matcher.hip, include/msda.h), and DINO's HungarianMatcher (models/dino/matcher.py:25-130) over the same kernel.

The reference builds the cost matrix of every query of every frame against every target of the batch, copies it to the
host and runs scipy's ``linear_sum_assignment`` per frame; its ``is_valid[idx] == 1`` comprehensions sync once per frame
each.  Here one launch builds each frame's ``Q x T_k`` block on chip and solves it with scipy's algorithm (same tie rule,
fp64 duals), for any number of prediction sets at once:

  * ``ArcticMatcher`` / ``AssemblyMatcher``  drop-ins: the reference's constructor, assert and ``forward(outputs,
    targets)``, returning the same list of ``(int64 CPU tensor, int64 CPU tensor)`` (or ``0`` when no valid frame has a
    label).  One launch and one device-to-host copy of the small result per call: that copy is the call's only sync.
  * ``pack_targets`` + ``match``  the device API: ``pack_targets`` does the list work once per step (host lists to one
    pinned copy, keypoints concatenated on the device, ``is_valid`` kept there); ``match`` takes the final, aux and
    interm prediction dicts and returns padded device tensors in one launch with no host sync, so it captures in a graph.

Pairing quirk, kept: the reference splits the VALID frames' targets by their sizes and matches chunk k against output
frame k (``enumerate(C.split(sizes, -1))`` then ``c[i]``, :122-123), not against the frame the chunk came from.  The
two differ when an earlier frame is invalid; the list has one entry per valid frame.

The reference's composition (the torch cost matrix, ``.cpu()``, scipy per frame; scipy imported only there) runs instead
for CPU tensors, non-fp32 inputs, more than 1024 queries or 16 targets in a frame, and with ``MSDA_MATCHER_FUSED=0``
(A/B knob).  The kernel also covers frames with more targets than queries (scipy then keeps the queries as rows)."""
import os
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _native as MSDA

FUSED = os.environ.get("MSDA_MATCHER_FUSED", "1") != "0"    # A/B knob: 0 = the reference's composition
ALPHA, GAMMA = 0.25, 2.0                                    # focal cost constants, fixed in the reference
HAND_LABELS = (12, 13)                                      # ARCTIC left / right hand: L1 against pred_hand_key
INVALID_MSG = "matrix contains invalid numeric entries"     # scipy's two ValueErrors
INFEASIBLE_MSG = "cost matrix is infeasible"


class PackedTargets(NamedTuple):
    """One step's targets on the device (``pack_targets``)."""
    kind: str                           # "arctic" (dict of per-frame lists) or "assembly" (list of per-frame dicts)
    labels: torch.Tensor                # [n] int64, every frame's labels flattened
    keypoints: Optional[torch.Tensor]   # [n, D] fp32, or None (ARCTIC targets without "keypoints")
    offsets: torch.Tensor               # [frames + 1] int64
    is_valid: Optional[torch.Tensor]    # [frames] int32 (is_valid == 1), ARCTIC only
    sizes: tuple                        # host: targets per frame
    t_max: int                          # host: max(sizes)


class MatchResult(NamedTuple):
    """``match``'s device result; all int64 views of ``buffer``."""
    query_idx: torch.Tensor    # [sets, bs, t_max], ascending, -1 padding
    target_idx: torch.Tensor   # [sets, bs, t_max]
    count: torch.Tensor        # [sets, bs]: pairs per slot (min(Q, T_k)); -1 past the valid frames
    status: torch.Tensor       # [sets, bs]: 0 ok, 1 invalid entries, 2 infeasible, 3 label out of range, 4 bad offsets
    num_valid: torch.Tensor    # [] valid frames (slots with a chunk)
    buffer: torch.Tensor       # the whole result, for one copy to the host


def _to_device(t, device):
    return torch.as_tensor(t).to(device, non_blocking=True)


def _host_to_device_i64(values, device):
    host = torch.tensor(values, dtype=torch.int64)
    if device.type == "cuda":
        host = host.pin_memory()
    return host.to(device, non_blocking=True)


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def pack_targets(targets, device):
    """Device form of one step's targets; never reads the device.  ARCTIC: ``targets`` is the reference's dict (``labels``
    a list of per-frame label lists, ``keypoints`` a list of [T_k, D] tensors (optional), ``is_valid`` [frames]); the
    labels and offsets go to the device in one pinned copy.  AssemblyHands: a list of per-frame dicts with ``labels`` and
    ``keypoints`` tensors, concatenated on the device; the sizes are ``len(v["keypoints"])`` (shapes, no sync)."""
    device = torch.device(device)
    if isinstance(targets, dict):
        sizes = tuple(len(t) for t in targets["labels"])
        flat = [int(x) for t in targets["labels"] for x in t]
        both = _host_to_device_i64(flat + _offsets(sizes), device)
        n = len(flat)
        kps = None
        if "keypoints" in targets:
            kps = torch.cat([_to_device(k, device) for k in targets["keypoints"]]).reshape(n, -1).contiguous()
        is_valid = (_to_device(targets["is_valid"], device).reshape(-1) == 1).to(torch.int32)
        return PackedTargets("arctic", both[:n], kps, both[n:], is_valid, sizes, max(sizes, default=0))
    sizes = tuple(len(v["keypoints"]) for v in targets)
    if sum(len(v["labels"]) for v in targets) != sum(sizes):
        raise ValueError("pack_targets: every frame needs as many labels as keypoint rows")
    n = sum(sizes)
    labels = torch.cat([_to_device(v["labels"], device).reshape(-1) for v in targets]).to(torch.int64)
    kps = torch.cat([_to_device(v["keypoints"], device) for v in targets]).reshape(n, -1).contiguous()
    return PackedTargets("assembly", labels, kps, _host_to_device_i64(_offsets(sizes), device), None, sizes,
                         max(sizes, default=0))


def match(outputs_list, packed, cost_class=1, cost_keypoint=1, cost_debug=None):
    """Matches every prediction dict of ``outputs_list`` (final, aux, interm; same shapes) against ``packed`` in ONE launch
    with no host sync (graph-capturable).  Needs contiguous-able fp32 CUDA predictions, Q <= 1024 and every frame's
    targets <= 16.  ``cost_debug`` (tests): fp32 [sets, bs, Q, t_max] receiving the cost blocks."""
    sets = len(outputs_list)
    logits = [o["pred_logits"].contiguous() for o in outputs_list]
    bs = logits[0].shape[0]
    if packed.offsets.shape[0] != bs + 1:
        raise ValueError("match: %d target frames for %d output frames" % (packed.offsets.shape[0] - 1, bs))
    if packed.kind == "arctic":
        has_kp = packed.keypoints is not None
        hand = [o["pred_hand_key"].contiguous() for o in outputs_list] if has_kp else None
        obj = [o["pred_obj_key"].contiguous() for o in outputs_list] if has_kp else None
        buf = MSDA.match_arctic(logits, hand, obj, packed.labels, packed.keypoints, packed.offsets, packed.is_valid,
                                packed.t_max, cost_class, cost_keypoint, cost_debug)
    else:
        kp = [o["pred_keypoints"].contiguous() for o in outputs_list]
        buf = MSDA.match_assembly(logits, kp, packed.labels, packed.keypoints, packed.offsets, packed.t_max, cost_class,
                                  cost_keypoint, cost_debug)
    return MatchResult(*MSDA.match_views(buf, sets, bs, packed.t_max), buf)


def indices_from_host(buffer, sets, bs, t_max, zero_if_empty=False):
    """The reference's per-set result from ``MatchResult.buffer`` copied to the host: a list (per set) of lists of
    ``(query_idx, target_idx)`` int64 CPU tensors, one per valid frame, or 0 for a set whose valid frames have no label
    (``zero_if_empty``, ARCTIC).  Raises scipy's ValueError on a slot whose status says so, frames in order."""
    qi, ti, count, status, nvalid = MSDA.match_views(buffer, sets, bs, t_max)
    count, status, nvalid = count.tolist(), status.tolist(), int(nvalid)
    result = []
    for s in range(sets):
        if zero_if_empty and all(count[s][k] == 0 and status[s][k] == 0 for k in range(nvalid)):
            result.append(0)
            continue
        for k in range(nvalid):
            st = status[s][k]
            if st == MSDA.MATCH_INVALID:
                raise ValueError(INVALID_MSG)
            if st == MSDA.MATCH_INFEASIBLE:
                raise ValueError(INFEASIBLE_MSG)
            if st == MSDA.MATCH_BAD_LABEL:
                raise IndexError("a target label is out of bounds for the class dimension")
            if st != 0:
                raise RuntimeError("matcher: target offsets do not describe the targets (status %d)" % st)
        result.append([(qi[s, k, :count[s][k]].clone(), ti[s, k, :count[s][k]].clone()) for k in range(nvalid)])
    return result


# ---- the reference's composition --------------------------------------------------------------------------------------
def _class_cost(logits, ids, alpha=ALPHA):
    prob = logits.flatten(0, 1).sigmoid()
    neg = (1 - alpha) * (prob ** GAMMA) * (-(1 - prob + 1e-8).log())
    pos = alpha * ((1 - prob) ** GAMMA) * (-(prob + 1e-8).log())
    return pos[:, ids] - neg[:, ids]


def _solve_blocks(C, sizes):
    from scipy.optimize import linear_sum_assignment       # only this route needs scipy
    pairs = [linear_sum_assignment(block[k]) for k, block in enumerate(C.split(sizes, -1))]
    return [(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)) for i, j in pairs]


def arctic_composition(outputs, targets, cost_class, cost_keypoint, alpha=ALPHA):
    """ArcticMatcher.forward as the reference computes it (host reads of is_valid, torch cost, .cpu(), scipy); ``alpha``:
    the focal cost's alpha (fixed in ArcticMatcher, a constructor argument of DINO's HungarianMatcher)."""
    logits = outputs["pred_logits"]
    bs, Q = logits.shape[:2]
    valid = [f for f in range(len(targets["labels"])) if targets["is_valid"][f] == 1]
    ids = [int(x) for f in valid for x in targets["labels"][f]]
    if not ids:
        return 0
    ids = torch.tensor(ids, device=logits.device)
    cost = _class_cost(logits, ids, alpha)
    if "keypoints" in targets:
        tgt = torch.cat([targets["keypoints"][f] for f in valid], dim=0)
        hand = (ids == HAND_LABELS[0]) | (ids == HAND_LABELS[1])
        obj = (ids != 0) & ~hand
        kp = torch.zeros_like(cost)
        kp[:, hand] = torch.cdist(outputs["pred_hand_key"].flatten(0, 1), tgt[hand], p=1)
        kp[:, obj] = torch.cdist(outputs["pred_obj_key"].flatten(0, 1), tgt[obj], p=1)
        C = cost_keypoint * kp + cost_class * cost
    else:
        C = cost_class * cost
    return _solve_blocks(C.view(bs, Q, -1).cpu(), [len(targets["labels"][f]) for f in valid])


def assembly_composition(outputs, targets, cost_class, cost_keypoint):
    """AssemblyMatcher.forward as the reference computes it."""
    logits = outputs["pred_logits"]
    bs, Q = logits.shape[:2]
    ids = torch.cat([v["labels"] for v in targets])
    tgt = torch.cat([v["keypoints"] for v in targets]).reshape(-1, 63)
    cost = _class_cost(logits, ids)
    hand = ids != 0
    kp = torch.zeros_like(cost)
    kp[:, hand] = torch.cdist(outputs["pred_keypoints"].flatten(0, 1), tgt[hand], p=1)
    C = cost_keypoint * kp + cost_class * cost
    return _solve_blocks(C.view(bs, Q, -1).cpu(), [len(v["keypoints"]) for v in targets])


def _fused_ok(preds, sizes, bs, extra=()):
    return (FUSED and all(t.is_cuda and t.dtype == torch.float32 for t in preds + list(extra))
            and len({t.device for t in preds + list(extra)}) == 1 and preds[0].dim() == 3
            and 1 <= bs and len(sizes) == bs and preds[0].shape[1] <= MSDA.MATCH_MAX_QUERIES
            and max(sizes, default=0) <= MSDA.MATCH_MAX_TARGETS)


class _MatcherBase(nn.Module):
    def __init__(self, cost_class: float = 1, cost_keypoint: float = 1, cfg=None):
        super().__init__()
        self.cost_class = cost_class
        self.cost_keypoint = cost_keypoint
        self.cfg = cfg
        assert cost_class != 0 or cost_keypoint != 0, "all costs cant be 0"


def _arctic_forward(outputs, targets, cost_class, cost_keypoint, alpha=ALPHA):
    """One set's host index lists over ARCTIC-style targets: one launch and one copy, or the composition."""
    with torch.no_grad():
        logits = outputs["pred_logits"]
        preds = [logits]
        if "keypoints" in targets:
            preds += [outputs["pred_hand_key"], outputs["pred_obj_key"]]
        sizes = [len(t) for t in targets["labels"]]
        kps = list(targets["keypoints"]) if "keypoints" in targets else []
        if not (alpha == ALPHA and _fused_ok(preds, sizes, logits.shape[0], [k for k in kps if torch.is_tensor(k)])
                and all(torch.is_tensor(k) and k.dtype == torch.float32 for k in kps)
                and all(k.shape[-1] == preds[-1].shape[-1] <= MSDA.MATCH_MAX_DIM for k in kps)):
            return arctic_composition(outputs, targets, cost_class, cost_keypoint, alpha)
        packed = pack_targets(targets, logits.device)
        res = match([outputs], packed, cost_class, cost_keypoint)
        return indices_from_host(res.buffer.cpu(), 1, logits.shape[0], packed.t_max, zero_if_empty=True)[0]


class ArcticMatcher(_MatcherBase):
    """Drop-in for models/matcher.py:20-125.  ``forward(outputs, targets)``: ``outputs`` has ``pred_logits`` [bs, Q, K] and
    (when ``targets`` has ``keypoints``) ``pred_hand_key`` / ``pred_obj_key`` [bs, Q, D]; ``targets`` is the reference's
    dict.  Returns one ``(query_idx, target_idx)`` pair of int64 CPU tensors per valid frame, or 0 without any label."""

    def forward(self, outputs, targets):
        return _arctic_forward(outputs, targets, self.cost_class, self.cost_keypoint)


class DinoHungarianMatcher(nn.Module):
    """Drop-in for DINO's HungarianMatcher (models/dino/matcher.py:25-130): the reference's constructor and assertion, and
    ``forward(outputs, targets)`` over the ARCTIC targets dict.  Its cost is ArcticMatcher's with ``cost_bbox`` in the place of
    ``cost_keypoint`` (``cost_giou`` is kept and, as in the reference, unused), so ``cost_keypoint`` reads ``cost_bbox`` for
    ``match``'s callers.  The kernel's focal alpha is 0.25; any other ``focal_alpha`` takes the torch composition.  (The
    reference raises without any valid label, where this returns 0 as ArcticMatcher does.)"""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, focal_alpha=0.25):
        super().__init__()
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.focal_alpha = focal_alpha

    @property
    def cost_keypoint(self):
        return self.cost_bbox

    def forward(self, outputs, targets):
        return _arctic_forward(outputs, targets, self.cost_class, self.cost_bbox, self.focal_alpha)


class AssemblyMatcher(_MatcherBase):
    """Drop-in for models/matcher.py:128-230.  ``outputs`` has ``pred_logits`` [bs, Q, K] and ``pred_keypoints``
    [bs, Q, 63]; ``targets`` a list of per-frame dicts with ``labels`` and ``keypoints``.  Returns one pair per frame."""

    def forward(self, outputs, targets):
        with torch.no_grad():
            logits = outputs["pred_logits"]
            preds = [logits, outputs["pred_keypoints"]]
            sizes = [len(v["keypoints"]) for v in targets]
            kps = [v["keypoints"] for v in targets]
            if not (_fused_ok(preds, sizes, logits.shape[0], kps) and preds[1].shape[-1] == 63
                    and all(k.numel() == 63 * len(k) for k in kps)):
                return assembly_composition(outputs, targets, self.cost_class, self.cost_keypoint)
            packed = pack_targets(targets, logits.device)
            res = match([outputs], packed, self.cost_class, self.cost_keypoint)
            return indices_from_host(res.buffer.cpu(), 1, logits.shape[0], packed.t_max)[0]
