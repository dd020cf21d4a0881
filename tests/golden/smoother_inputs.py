"""Seeded inputs of the SmoothNet fixtures (gen_golden_r11.py) and of tests/test_smoother*.py / tests/test_arctic_item*.py:
MotionSmoother cases at small sizes, the default-size ArcticSmoother case and the query-selection cases.  Shared by the
generator and the tests, so nothing at test time reads the reference."""
import hashlib

import torch

# name: (T, H, res hidden, num_blocks, B, C, seed); eval mode
SMALL_CASES = {
    "t8_b3": (8, 64, 32, 2, 3, 5, 201),
    "t16_b1_c1": (16, 64, 32, 2, 1, 1, 202),
    "t16_b3": (16, 64, 32, 2, 3, 48, 203),
}
ARCTIC_T, ARCTIC_B, ARCTIC_SEED = 32, 1, 211
ARCTIC_WIDTHS = (3, 3, 3, 48, 48, 10, 10, 3, 1)    # root_l, root_r, root_o, pose_l, pose_r, shape_l, shape_r, obj_rot, obj_rad


def build_motion(cls, name):
    T, H, R, nb, _, _, seed = SMALL_CASES[name]
    torch.manual_seed(seed)
    return cls(T, T, H, R, nb).eval()


def motion_input(name):
    T, _, _, _, B, C, seed = SMALL_CASES[name]
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randn(B, T, C, generator=g)


def build_arctic(cls):
    torch.manual_seed(ARCTIC_SEED)
    return cls(ARCTIC_B, ARCTIC_T).eval()


def arctic_inputs(B=ARCTIC_B, T=ARCTIC_T, seed=ARCTIC_SEED + 1):
    """The nine [B * T, w] parameters ArcticSmoother.forward takes, flat, in ARCTIC_WIDTHS order."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B * T, w, generator=g) for w in ARCTIC_WIDTHS]


def structure(flat):
    return [flat[0], flat[1], flat[2]], [flat[3], flat[4]], [flat[5], flat[6]], [flat[7], flat[8]]


def flatten(out):
    return [t for group in out for t in group]


def weighted_sum(outs, seed):
    g = torch.Generator().manual_seed(seed)
    total = 0
    for o in outs:
        total = total + (o * torch.randn(o.shape, generator=g).to(o.device)).sum()
    return total


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ---- get_arctic_item --------------------------------------------------------------------------------------------------------
class Cfg:
    hand_idx = [12, 13]


K_CLASSES = 14
SOURCE_WIDTHS = (("hand_cam", 3), ("obj_cam", 3), ("mano_pose", 48), ("mano_shape", 10), ("obj_rad", 1), ("obj_rot", 3))
ITEM_CASES = ("ties", "negative", "same_query", "nan")


def item_outputs(name, bs=5, Q=24):
    """DETR outputs for the selection: logits [bs, Q, 14] and the six sources, by case:
    ties        saturated logits (sigmoid == 1.0f) on several queries of object and hand classes
    negative    every object logit -200 (probability 0: obj_idx stays 0)
    same_query  both hand classes peak on the same query
    nan         one NaN logit in a hand column and one in an object column"""
    g = torch.Generator().manual_seed(300 + ITEM_CASES.index(name))
    logits = torch.randn(bs, Q, K_CLASSES, generator=g) * 3
    if name == "ties":
        logits[0, 5, 3] = 30.0
        logits[0, 2, 7] = 25.0
        logits[0, 9, 7] = 40.0
        logits[1, 4, 12] = 20.0
        logits[1, 1, 12] = 35.0
        logits[2, 3:8, 13] = 50.0
        logits[3, :, 1:12] = 18.0
    elif name == "negative":
        logits[:, :, 1:12] = -200.0
    elif name == "same_query":
        logits[:, 6, 12] = 9.0
        logits[:, 6, 13] = 9.0
        logits[2, 6, 12] = 40.0
        logits[2, 11, 12] = 40.0
    elif name == "nan":
        logits[0, 4, 12] = float("nan")
        logits[1, 7, 5] = float("nan")
        logits[2, 3, 2] = float("nan")
        logits[2, 10, 9] = 30.0
    srcs = {k: torch.randn(bs, Q, w, generator=g) for k, w in SOURCE_WIDTHS}
    return {"pred_logits": logits, "pred_cams": [srcs["hand_cam"], srcs["obj_cam"]],
            "pred_mano_params": [srcs["mano_pose"], srcs["mano_shape"]],
            "pred_obj_params": [srcs["obj_rad"], srcs["obj_rot"]]}
