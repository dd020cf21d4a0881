"""Seeded inputs of the DINO criterion fixture (gen_dino_criterion.py; tests/test_dino_criterion*.py), regenerated from the
stored seeds so that the fixture keeps only the reference's loss values (and, for the small case, its gradients).

14 classes (12 / 13 the hands; the criterion's empty class is K - 1), 42 keypoint values, 1-3 targets per frame.  The
prediction sets are the final one, N aux sets and interm_outputs; ``outputs['dn_meta']`` carries the denoising set
``output_known_lbs_bboxes`` of ``groups * single_pad`` queries.  Cases:

  small        4 frames x 40 queries, groups 2, single_pad 6, 2 aux sets, ['labels', 'boxes', 'cardinality']; gradients stored
  interleaved  8 frames, every third frame invalid (the slot pairing, for matched and denoising sets alike)
  no_hand      no target is a hand: loss_hand_keypoint 0
  no_object    every target is a hand: loss_obj_keypoint nan (0 / 0)
  labels_only  ['labels', 'cardinality'] (the targets keep their keypoints: the reference's matcher reads them)
  eval         the criterion in eval mode: the six zero denoising keys
  no_dn        training, dn_meta without the known outputs: the six zero keys
  window       32 frames x 900 queries, groups 33, single_pad 6, 5 aux sets; values only
"""
from types import SimpleNamespace

import torch

K, D = 14, 42
COST_CLASS, COST_BBOX, COST_GIOU = 1.5, 4.0, 2.0
FOCAL_ALPHA = 0.25
CASES = ("small", "interleaved", "no_hand", "no_object", "labels_only", "eval", "no_dn", "window")
ARGS = SimpleNamespace(device="cpu", img_res=224)
TERMS = ("loss_ce", "loss_hand_keypoint", "loss_obj_keypoint", "cardinality_error")
HEADS = ("pred_logits", "pred_hand_key", "pred_obj_key")


def shape(case):
    """(frames, queries, groups, single_pad, aux sets)"""
    if case == "window":
        return 32, 900, 33, 6, 5
    if case == "small":
        return 4, 40, 2, 6, 2
    return 8, 40, 2, 6, 2


def losses(case):
    return ["labels", "cardinality"] if case == "labels_only" else ["labels", "boxes", "cardinality"]


def weight_dict(n_aux):
    """Distinct weights per key (the gradients of the weighted total test every column of every set)."""
    base = {n: 1.0 + 0.75 * i for i, n in enumerate(TERMS)}
    w = dict(base)
    for i, sfx in enumerate([f"_{a}" for a in range(n_aux)] + ["_interm", "_dn"]):
        w.update({k + sfx: v * (1.1 + 0.2 * i) for k, v in base.items()})
    return w


def _set(g, bs, Q):
    return {"pred_logits": torch.randn(bs, Q, K, generator=g) * 2.0,
            "pred_hand_key": torch.rand(bs, Q, D, generator=g),
            "pred_obj_key": torch.rand(bs, Q, D, generator=g)}


def make(case, seed):
    """(outputs, targets, losses) on the CPU in the reference's layouts: outputs has aux_outputs, interm_outputs and dn_meta;
    targets = {"labels": list of label lists, "keypoints": list of [T_k, 42] tensors, "is_valid": float32 [bs]}."""
    bs, Q, groups, single_pad, n_aux = shape(case)
    g = torch.Generator().manual_seed(seed)
    outputs = _set(g, bs, Q)
    outputs["aux_outputs"] = [_set(g, bs, Q) for _ in range(n_aux)]
    outputs["interm_outputs"] = _set(g, bs, Q)
    known = _set(g, bs, groups * single_pad)
    known["aux_outputs"] = [_set(g, bs, groups * single_pad) for _ in range(n_aux)]     # present, unused (:709-731)
    outputs["dn_meta"] = {"pad_size": groups * single_pad, "num_dn_group": groups}
    if case != "no_dn":
        outputs["dn_meta"]["output_known_lbs_bboxes"] = known
    labels, keypoints = [], []
    for f in range(bs):
        T = int(torch.randint(1, single_pad // 2 + 1, (1,), generator=g))
        lab = []
        for t in range(T):
            r = int(torch.randint(0, 10, (1,), generator=g))
            if case == "no_hand":
                lab.append(int(torch.randint(0, 12, (1,), generator=g)))
            elif case == "no_object":
                lab.append(12 + (r & 1))
            else:
                lab.append(12 + (r & 1) if r < 5 else (0 if r == 9 else int(torch.randint(1, 12, (1,), generator=g))))
        labels.append(lab)
        keypoints.append(torch.rand(T, D, generator=g))
    is_valid = torch.ones(bs, dtype=torch.float32)
    if case == "interleaved":
        is_valid[2::3] = 0
    return outputs, {"labels": labels, "keypoints": keypoints, "is_valid": is_valid}, losses(case)


def sets_of(outputs):
    """The matched prediction dicts in the drop-in's order: final, aux..., interm."""
    skip = ("aux_outputs", "interm_outputs", "dn_meta")
    final = {k: v for k, v in outputs.items() if k not in skip}
    return [final] + list(outputs.get("aux_outputs", [])) + [outputs["interm_outputs"]]


def dn_set(outputs):
    """The denoising set's own prediction dict, or None."""
    known = outputs["dn_meta"].get("output_known_lbs_bboxes")
    return None if known is None else {k: known[k] for k in HEADS}


def _map(outputs, leaf):
    out = {}
    for k, v in outputs.items():
        if k == "aux_outputs":
            out[k] = [_map(a, leaf) for a in v]
        elif isinstance(v, dict):
            out[k] = _map(v, leaf)
        elif torch.is_tensor(v):
            out[k] = leaf(v)
        else:
            out[k] = v
    return out


def to_device(outputs, targets, device, requires_grad=False, dtype=None):
    """The same inputs on `device` (new leaves; the targets' tensors moved too)."""
    def leaf(t):
        return t.detach().to(device=device, dtype=dtype or t.dtype).clone().requires_grad_(requires_grad)

    t = dict(targets)
    t["is_valid"] = targets["is_valid"].to(device)
    t["keypoints"] = [k.to(device=device, dtype=dtype or k.dtype) for k in targets["keypoints"]]
    return _map(outputs, leaf), t


def weighted_total(loss_dict, weights):
    return sum(loss_dict[k] * weights[k] for k in loss_dict.keys() if k in weights)


def gradients(outputs):
    """{"grad_<head>": [sets, bs, Q, .], "grad_dn_<head>": [bs, pad, .]} of leaves made by to_device(requires_grad=True); a
    leaf the total does not reach counts as zero."""
    def grad(t):
        return t.grad if t.grad is not None else torch.zeros_like(t)

    out = {"grad_" + h: torch.stack([grad(s[h]) for s in sets_of(outputs)]) for h in HEADS}
    dn = dn_set(outputs)
    if dn is not None:
        out.update({"grad_dn_" + h: grad(dn[h]) for h in HEADS})
    return out
