"""Seeded inputs of the criterion fixtures (gen_golden_r09.py; tests/test_criterion*.py), regenerated from the stored seeds so
that the fixtures keep only the reference's loss values (and, for the small cases, its gradients).

  ARCTIC         14 classes (12 / 13 the hands), 42 keypoint values, 1-3 targets per frame; the prediction sets are the final
                 one, N_AUX aux sets and (unless the case says otherwise) interm_outputs.  Cases:
                   full            window 32 (32 frames x 300 queries), every frame valid, ['labels', 'boxes'], 5 aux sets
                   interleaved     every third frame invalid (the pairing quirk), ['labels', 'boxes', 'cardinality']
                   no_hand         no target is a hand: loss_hand_keypoint 0
                   no_object       every target is a hand: loss_obj_keypoint nan (0 / 0)
                   labels_only     targets without keypoints, ['labels', 'cardinality']
                   no_valid_label  labels only on invalid frames: the matcher returns 0 (no interm set: the reference
                                   cannot take one there)
                   small           4 frames x 40 queries, 5 aux sets and interm, gradients stored
  AssemblyHands  3 classes (hand_idx [1, 2]), 63 keypoint values, 1-2 hands per frame, joint_valid with false entries;
                 final + 5 aux sets, ['labels', 'cardinality', 'hand_keypoint'].  Cases:
                   full            window 32, every label a hand
                   small           4 frames x 40 queries, gradients stored
                   enc             full plus enc_outputs: the reference raises (label 0 is not a hand)
                   not_hand        full with one label 0 target: the reference raises (joint_valid mask mismatch)
"""
from types import SimpleNamespace

import torch

ARCTIC_K, ARCTIC_D = 14, 42
ASSEMBLY_K, ASSEMBLY_D = 3, 63
COST_CLASS, COST_KEYPOINT = 1.5, 4.0
FOCAL_ALPHA = 0.25
ARCTIC_CASES = ("full", "interleaved", "no_hand", "no_object", "labels_only", "no_valid_label", "small")
ASSEMBLY_CASES = ("full", "small", "enc", "not_hand")
HAND_IDX = [1, 2]
ASSEMBLY_CFG = SimpleNamespace(hand_idx=HAND_IDX)
ARCTIC_ARGS = SimpleNamespace(device="cpu", img_res=224)


def _shape(case):
    return (4, 40) if case == "small" else (32, 300)


def _n_aux(case):
    return 5 if case in ("full", "small") else 2


def arctic_losses(case):
    if case == "full" or case == "no_valid_label":
        return ["labels", "boxes"]
    if case == "labels_only":
        return ["labels", "cardinality"]
    return ["labels", "boxes", "cardinality"]


def weight_dict(names, n_aux, extra=("_interm",)):
    """Distinct weights per key (the gradients of the weighted total test every column)."""
    base = {n: 1.0 + 0.75 * i for i, n in enumerate(names)}
    w = dict(base)
    for i, sfx in enumerate([f"_{a}" for a in range(n_aux)] + list(extra)):
        w.update({k + sfx: v * (1.1 + 0.2 * i) for k, v in base.items()})
    return w


ARCTIC_WEIGHTS = ("loss_ce", "loss_hand_keypoint", "loss_obj_keypoint", "cardinality_error")
ASSEMBLY_WEIGHTS = ("loss_ce", "loss_hand_keypoint", "cardinality_error", "class_error")


def _arctic_set(g, bs, Q):
    return {"pred_logits": torch.randn(bs, Q, ARCTIC_K, generator=g) * 2.0,
            "pred_hand_key": torch.rand(bs, Q, ARCTIC_D, generator=g),
            "pred_obj_key": torch.rand(bs, Q, ARCTIC_D, generator=g)}


def arctic_case(case, seed):
    """(outputs, targets, losses) on the CPU in the reference's layouts: outputs has aux_outputs (and interm_outputs);
    targets = {"labels": list of label lists, "keypoints": list of [T_k, 42] tensors, "is_valid": float32 [bs]}."""
    bs, Q = _shape(case)
    g = torch.Generator().manual_seed(seed)
    outputs = _arctic_set(g, bs, Q)
    outputs["aux_outputs"] = [_arctic_set(g, bs, Q) for _ in range(_n_aux(case))]
    if case != "no_valid_label":
        outputs["interm_outputs"] = _arctic_set(g, bs, Q)
    labels, keypoints = [], []
    for f in range(bs):
        T = int(torch.randint(1, 4, (1,), generator=g))
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
        keypoints.append(torch.rand(T, ARCTIC_D, generator=g))
    is_valid = torch.ones(bs, dtype=torch.float32)
    if case == "interleaved":               # (a valid frame without labels makes the reference's torch.tensor([]) float)
        is_valid[2::3] = 0
    elif case == "no_valid_label":
        is_valid[1::2] = 0
        for f in range(0, bs, 2):
            labels[f] = []
            keypoints[f] = keypoints[f][:0]
    targets = {"labels": labels, "keypoints": keypoints, "is_valid": is_valid}
    if case == "labels_only":               # class cost only: two targets of one label would tie, so labels stay distinct
        del targets["keypoints"]
        targets["labels"] = [list(dict.fromkeys(lab)) for lab in labels]
    return outputs, targets, arctic_losses(case)


def _assembly_set(g, bs, Q):
    return {"pred_logits": torch.randn(bs, Q, ASSEMBLY_K, generator=g) * 2.0,
            "pred_keypoints": torch.rand(bs, Q, ASSEMBLY_D, generator=g)}


def assembly_case(case, seed):
    """(outputs, targets, losses): targets is a list of {"labels": int64 [T_k], "keypoints": [T_k, 63], "joint_valid": bool
    [T_k, 21, 3]}."""
    bs, Q = _shape(case)
    g = torch.Generator().manual_seed(seed)
    outputs = _assembly_set(g, bs, Q)
    outputs["aux_outputs"] = [_assembly_set(g, bs, Q) for _ in range(_n_aux(case))]
    if case == "enc":
        outputs["enc_outputs"] = _assembly_set(g, bs, Q)
    targets = []
    for f in range(bs):
        T = int(torch.randint(1, 3, (1,), generator=g))
        lab = torch.randint(1, ASSEMBLY_K, (T,), generator=g)
        if case == "not_hand" and f == 7:
            lab[0] = 0
        jv = (torch.rand(T, 21, generator=g) > 0.2).unsqueeze(-1).repeat(1, 1, 3)
        targets.append({"labels": lab, "keypoints": torch.rand(T, ASSEMBLY_D, generator=g), "joint_valid": jv})
    return outputs, targets, ["labels", "cardinality", "hand_keypoint"]


def sets_of(outputs):
    """The prediction dicts in the drop-ins' order: final, aux..., interm / enc."""
    final = {k: v for k, v in outputs.items() if k not in ("aux_outputs", "interm_outputs", "enc_outputs")}
    extra = [outputs[k] for k in ("interm_outputs", "enc_outputs") if k in outputs]
    return [final] + list(outputs.get("aux_outputs", [])) + extra


def heads(kind):
    return ("pred_logits", "pred_hand_key", "pred_obj_key") if kind == "arctic" else ("pred_logits", "pred_keypoints")


def to_device(outputs, targets, device, requires_grad=False):
    """The same inputs on `device` (new leaves; targets' tensors moved too)."""
    def leaf(t):
        t = t.detach().to(device).clone()
        return t.requires_grad_(requires_grad)

    out = {}
    for k, v in outputs.items():
        if k == "aux_outputs":
            out[k] = [{kk: leaf(vv) for kk, vv in a.items()} for a in v]
        elif isinstance(v, dict):
            out[k] = {kk: leaf(vv) for kk, vv in v.items()}
        else:
            out[k] = leaf(v)
    if isinstance(targets, dict):
        t = dict(targets)
        t["is_valid"] = targets["is_valid"].to(device)
        if "keypoints" in t:
            t["keypoints"] = [k.to(device) for k in targets["keypoints"]]
        return out, t
    return out, [{k: v.to(device) for k, v in d.items()} for d in targets]


def weighted_total(loss_dict, weights):
    return sum(loss_dict[k] * weights[k] for k in loss_dict.keys() if k in weights)
