"""Seeded inputs of the matcher fixtures (gen_golden_r08.py; tests/test_matcher*.py), regenerated from the stored seeds so
that the fixtures keep only the reference's indices and margins.

  ARCTIC      32 frames x 300 queries, 14 classes (12 / 13 the hands), 42 keypoint values, 1-3 targets per frame (some of
              label 0), cost_class 1.5, cost_keypoint 4; cases:
                all_valid     every frame valid
                interleaved   every third frame invalid (the chunk-pairing quirk) and two valid frames without labels
                no_keypoints  all_valid's targets without "keypoints" (class cost only), repeated labels dropped
                no_labels     valid frames without labels, labels only on invalid frames: forward returns 0
  AssemblyHands  32 frames x 300 queries, 3 classes, 63 keypoint values, 1-2 hands per frame (one label 0 target).
  LSAP        random fp32 matrices [B, Q, T] for the solver (numpy PCG64, per (Q, T) seed) and integer-valued ones with ties.
"""
import numpy as np
import torch

BS, Q = 32, 300
ARCTIC_K, ARCTIC_D = 14, 42
ASSEMBLY_K, ASSEMBLY_D = 3, 63
COST_CLASS, COST_KEYPOINT = 1.5, 4.0
ARCTIC_CASES = ("all_valid", "interleaved", "no_keypoints", "no_labels")

LSAP_Q = (1, 3, 16, 64, 300, 900, 1024)
LSAP_T = (0, 1, 2, 3, 7, 16)
LSAP_WIDE = ((1, 2), (1, 16), (3, 7), (3, 16), (7, 16))      # T > Q: scipy keeps the queries as rows
LSAP_B = 4
TIE_SHAPES = ((3, 3), (16, 16), (64, 3), (300, 16), (1024, 7))


def arctic_case(case, seed):
    """(outputs, targets) on the CPU, the reference's layouts: targets = {"labels": list of label lists, "keypoints": list of
    [T_k, 42] tensors, "is_valid": float32 [bs]}."""
    g = torch.Generator().manual_seed(seed)
    outputs = {"pred_logits": torch.randn(BS, Q, ARCTIC_K, generator=g) * 2.0,
               "pred_hand_key": torch.rand(BS, Q, ARCTIC_D, generator=g),
               "pred_obj_key": torch.rand(BS, Q, ARCTIC_D, generator=g)}
    labels, keypoints = [], []
    for f in range(BS):
        T = int(torch.randint(1, 4, (1,), generator=g))
        lab = []
        for t in range(T):
            r = int(torch.randint(0, 10, (1,), generator=g))
            lab.append(12 + (r & 1) if r < 5 else (0 if r == 9 else int(torch.randint(1, 12, (1,), generator=g))))
        labels.append(lab)
        keypoints.append(torch.rand(T, ARCTIC_D, generator=g))
    is_valid = torch.ones(BS, dtype=torch.float32)
    if case == "interleaved":
        is_valid[2::3] = 0
        for f in (4, 10):                   # valid frames with an empty label list
            labels[f] = []
            keypoints[f] = keypoints[f][:0]
    elif case == "no_labels":
        is_valid[1::2] = 0
        for f in range(0, BS, 2):
            labels[f] = []
            keypoints[f] = keypoints[f][:0]
    targets = {"labels": labels, "keypoints": keypoints, "is_valid": is_valid}
    if case == "no_keypoints":              # class cost only: two targets of one label would tie, so labels stay distinct
        del targets["keypoints"]
        targets["labels"] = [list(dict.fromkeys(lab)) for lab in labels]
    return outputs, targets


def assembly_case(seed):
    """(outputs, targets): targets is a list of {"labels": int64 [T_k], "keypoints": [T_k, 63]}."""
    g = torch.Generator().manual_seed(seed)
    outputs = {"pred_logits": torch.randn(BS, Q, ASSEMBLY_K, generator=g) * 2.0,
               "pred_keypoints": torch.rand(BS, Q, ASSEMBLY_D, generator=g)}
    targets = []
    for f in range(BS):
        T = int(torch.randint(1, 3, (1,), generator=g))
        lab = torch.randint(1, ASSEMBLY_K, (T,), generator=g)
        if f == 7:
            lab[0] = 0
        targets.append({"labels": lab, "keypoints": torch.rand(T, ASSEMBLY_D, generator=g)})
    return outputs, targets


def to_device(outputs, targets, device):
    """The same inputs on `device` (is_valid and keypoints too, as the reference's prefetcher moves them)."""
    out = {k: v.to(device) for k, v in outputs.items()}
    if isinstance(targets, dict):
        t = dict(targets)
        t["is_valid"] = targets["is_valid"].to(device)
        if "keypoints" in t:
            t["keypoints"] = [k.to(device) for k in targets["keypoints"]]
        return out, t
    return out, [{k: v.to(device) for k, v in d.items()} for d in targets]


def lsap_matrix(Q, T, B=LSAP_B):
    rng = np.random.default_rng(1000 * Q + T)
    return rng.random((B, Q, T), dtype=np.float32)


def tie_matrix(Q, T, B=LSAP_B):
    rng = np.random.default_rng(7000 + 1000 * Q + T)
    return rng.integers(0, 4, size=(B, Q, T)).astype(np.float32)


def lsap_shapes():
    return [(q, t) for q in LSAP_Q for t in LSAP_T if t <= q] + list(LSAP_WIDE)


def flatten_indices(result):
    """(lengths [frames], i concatenated, j concatenated) of a matcher's list result; (-1 lengths, empty) for the int 0."""
    if isinstance(result, int):
        return np.array([-1], np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    lens = np.array([len(i) for i, _ in result], np.int64)
    cat = lambda xs: np.concatenate([np.asarray(x, np.int64) for x in xs]) if xs else np.zeros(0, np.int64)  # noqa: E731
    return lens, cat([i for i, _ in result]), cat([j for _, j in result])
