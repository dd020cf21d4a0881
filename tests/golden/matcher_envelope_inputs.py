"""Seeded inputs of the matcher / criterion envelope tests (gen_matcher_envelope.py; tests/test_matcher_envelope*.py),
regenerated from the seeds of the case table so that matcher_envelope.npz keeps only scipy's indices, the optima, the
uniqueness gaps and version strings.  Nothing here imports scipy.

The kernels' envelope (csrc/msda_matcher.hip, csrc/msda_criterion.hip): Q <= 1024 queries, T <= 16 targets per frame,
D <= 64 keypoint values, up to 16 sets, bs <= 1024 frames.  MATCH_CASES visits its corners; every frame's target count comes
from a cycle over SIZES = (0, 1, 4, 15, 16) unless the case says otherwise, so every batch mixes T = 0, 1, 4, 15 and
16 = t_max (the MtCol register vector and, with D = 64, sh.kp full) and every case has W = 16.

  case            for which branch
  *_q1            Q = 1: one query thread; wide (Q <= T, the block handed through sh.stage) for T >= 1, Q = T at T = 1
  *_q5            Q = 5: wide for T = 15 / 16, Q = T + 1 at T = 4; targets stay unmatched (AssemblyHands: status bit 4)
  *_q16           Q = 16: Q = T at T = 16 (wide), Q = T + 1 at T = 15; a frame with 16 matched rows
  *_q17           Q = 17: Q = T + 1 at T = 16, the narrowest tall block with every register row in use
  *_q63/64/65     either side of the wavefront boundary (one wave with an idle lane, one full wave, two waves)
  *_q300          the production query count
  *_q1024         16 waves: every entry of sh.red, the whole of the criterion's frame_of / card arrays' query loop
  arctic_d64      D = 64 = kMatchMaxDim with T = 16: sh.kp full; the last keypoint value is scaled by 8 so that a kernel
                  that stops at D = 63 changes assignments
  arctic_bs130    bs = 130 with Q = 16: a 64-thread block needs three rounds of the valid-frame prefix; 45 frames are
                  invalid at irregular positions, with runs that cross frames 64 and 128 (the chunk-pairing quirk)
  *_sets7         7 independent prediction sets (their assignments differ); ARCTIC with interleaved invalid frames
  arctic_ties_*   class-only targets (no keypoints) WITH repeated labels: identical cost columns, so scipy's tie rule
                  decides.  Tall (Q = 300 / 65) they are identical ROWS of the solved problem and the strict `<` of the
                  path update decides who keeps the better query; wide (Q = 5, and 16 at T = 16) they are identical
                  columns and the argmin's rule (an unassigned column wins, the last in `remaining` order) decides
  arctic_label0   every label 0 with keypoints: the L1 term is 0, identical columns again; no hand row in the criterion
  arctic_hands    every target a hand (12 / 13): loss_obj_keypoint is 0 / 0 = nan
  arctic_objects  every target an object (1..11): loss_hand_keypoint is 0
  assembly_label0 Q = 5 with label 0 targets among the hands: their columns tie exactly (wide), the criterion reports
                  status bit 4

LSAP_KINDS are cost matrices for the bare solver (`_native.lsap`), given exactly in fp32, for which scipy's indices are
demanded exactly: feasible with 10-50 % +inf entries, signed, scaled by 1e30 and 1e-30, columns spanning 12 orders of
magnitude, integer ties in {0..3}, duplicated rows and duplicated columns.

Tolerances.  EPS = 1e-5 is the bound tests/test_matcher_gpu.py asserts on a cost block (max |diff| / max |C|).  Two
assignments of n = min(Q, T) pairs each move by at most n EPS max|C| when every entry is off by EPS max|C|, so totals
are compared within 2 n EPS max|C|, and a frame's indices must equal scipy's when its uniqueness gap is at least 2 n EPS.

The uniqueness gap of a frame: the optimum with one matched pair forbidden, minimised over the matched pairs, minus the
optimum, over max|C|.  Targets of one label whose columns are identical by construction (no target keypoints, or label 0,
whose L1 term is 0) form one class, and forbidding a pair forbids the query's pairs with the whole class: swapping two
identical columns does not change the optimum, and which of them a query gets is what scipy's tie rule decides.  scipy
is given the fp64 restatement rounded to fp32, as the reference hands it an fp32 matrix: the fp64 duals of fp32 costs are
(almost always) exact, so the tie rule sees exact ties where the columns are identical, which it does not on rounded fp64
sums.  TIE_CASES and the LSAP matrices are exact by construction: no frame of theirs may fall under the gap.
"""
import numpy as np
import torch

COST_CLASS, COST_KEYPOINT = 1.5, 4.0
FOCAL_ALPHA = 0.25
HAND_IDX = (1, 2)
EPS = 1e-5
MAX_EXCLUDED = 0.25                 # share of a case's frames that may fall under the gap
SIZES = (0, 1, 4, 15, 16)
ARCTIC_K, ARCTIC_D = 14, 42
ASSEMBLY_K, ASSEMBLY_D = 3, 63

# invalid runs (first frame, length) of arctic_bs130: 45 of 130 frames; the runs at 58 and 122 cross frames 64 and 128
BS130_INVALID = ((3, 1), (7, 2), (13, 1), (20, 1), (26, 3), (33, 1), (41, 1), (47, 2), (58, 13), (77, 1), (85, 2), (92, 1),
                 (99, 1), (101, 1), (106, 1), (110, 4), (119, 1), (122, 8))


def _case(kind, bs, Q, seed, D=None, sets=1, labels="mixed", keypoints=True, invalid=(), sizes=SIZES, scale_last=1.0):
    arctic = kind == "arctic"
    return dict(kind=kind, bs=bs, Q=Q, K=ARCTIC_K if arctic else ASSEMBLY_K, D=D or (ARCTIC_D if arctic else ASSEMBLY_D),
                sets=sets, labels=labels, keypoints=keypoints, invalid=tuple(invalid), sizes=tuple(sizes), seed=seed,
                scale_last=scale_last)


def _runs(runs):
    return tuple(f for lo, n in runs for f in range(lo, lo + n))


MATCH_CASES = {}
for _i, _q in enumerate((1, 5, 16, 17, 63, 64, 65, 300, 1024)):
    MATCH_CASES["arctic_q%d" % _q] = _case("arctic", 5 if _q == 1024 else 10, _q, 100 + _i)
    MATCH_CASES["assembly_q%d" % _q] = _case("assembly", 5 if _q == 1024 else 10, _q, 200 + _i)
MATCH_CASES.update({
    "arctic_d64": _case("arctic", 10, 65, 120, D=64, scale_last=8.0),
    "arctic_bs130": _case("arctic", 130, 16, 121, invalid=_runs(BS130_INVALID)),
    "arctic_sets7": _case("arctic", 12, 64, 122, sets=7, invalid=(1, 2, 5, 9)),
    "arctic_ties_q300": _case("arctic", 10, 300, 123, labels="repeat", keypoints=False),
    "arctic_ties_q65": _case("arctic", 10, 65, 124, labels="repeat", keypoints=False),
    "arctic_ties_q5": _case("arctic", 10, 5, 125, labels="repeat", keypoints=False),
    "arctic_ties_q16": _case("arctic", 10, 16, 129, labels="repeat", keypoints=False),
    "arctic_label0": _case("arctic", 10, 64, 126, labels="zeros"),
    "arctic_hands": _case("arctic", 10, 17, 127, labels="hands"),
    "arctic_objects": _case("arctic", 10, 17, 128, labels="objects"),
    "assembly_sets7": _case("assembly", 10, 65, 220, sets=7),
    "assembly_label0": _case("assembly", 10, 5, 221, labels="with_zero"),
})
TIE_CASES = ("arctic_ties_q300", "arctic_ties_q65", "arctic_ties_q5", "arctic_ties_q16", "arctic_label0", "assembly_label0")

# which cases each wrong kernel of tests/test_matcher_envelope.py must be caught by
MUTANT_TARGETS = {
    "greedy": ("arctic_q5", "arctic_q17", "arctic_q65", "assembly_q16", "assembly_q64"),
    "first_min": ("arctic_ties_q5", "arctic_ties_q16", "assembly_label0"),      # wide: identical columns tie
    "path_le": ("arctic_ties_q300", "arctic_ties_q65", "arctic_label0"),        # tall: identical rows tie
    "slot_is_frame": ("arctic_bs130", "arctic_sets7"),
    "prefix_no_carry": ("arctic_bs130",),
    "wide_untransposed": ("arctic_q5", "arctic_q16", "assembly_q1", "assembly_q5"),
    "t_clip15": ("arctic_q16", "arctic_q17", "arctic_q1024", "assembly_q17", "assembly_q64"),
    "d_clip63": ("arctic_d64",),
}


def _labels(case, T, g):
    mode, arctic = case["labels"], case["kind"] == "arctic"
    draw = lambda lo, hi: [int(x) for x in torch.randint(lo, hi, (T,), generator=g)]     # noqa: E731
    if mode == "zeros":
        return [0] * T
    if mode == "hands":
        return draw(12, 14)
    if mode == "objects":
        return draw(1, 12)
    if mode == "repeat":                    # 5 labels for up to 16 targets: repeated labels in every frame with T >= 6
        return [(0, 3, 7, 12, 13)[x] for x in draw(0, 5)]
    if mode == "with_zero":                 # AssemblyHands: label 0 at every third target
        return [0 if t % 3 == 1 else x for t, x in enumerate(draw(1, ASSEMBLY_K))]
    if not arctic:
        return draw(1, ASSEMBLY_K)
    out = []
    for r in draw(0, 10):                   # as matcher_inputs.arctic_case: half hands, one in ten label 0
        out.append(12 + (r & 1) if r < 5 else (0 if r == 9 else 1 + (r * 7 + len(out)) % 11))
    return out


def match_case(name):
    """(sets, targets) on the CPU in the reference's layouts.  sets: list of prediction dicts (fp32).  ARCTIC targets:
    {"labels": list of label lists, "keypoints": list of [T_k, D] (optional), "is_valid": float32 [bs]}; AssemblyHands: a list
    of {"labels": int64 [T_k], "keypoints": [T_k, 63], "joint_valid": bool [T_k, 21, 3]}."""
    c = MATCH_CASES[name]
    bs, Q, K, D = c["bs"], c["Q"], c["K"], c["D"]
    arctic = c["kind"] == "arctic"
    g = torch.Generator().manual_seed(c["seed"])
    heads = ("pred_hand_key", "pred_obj_key") if arctic else ("pred_keypoints",)
    sets = []
    for _ in range(c["sets"]):
        o = {"pred_logits": torch.randn(bs, Q, K, generator=g) * 2.0}
        if name in TIE_CASES:               # each class's logits over a frame's queries: a permutation of an even grid,
            step = 8.0 / (Q - 1)            # jittered by less than a third of its step, so that no two queries nearly tie
            order = torch.rand(bs, Q, K, generator=g).argsort(1)            # for a label and the gap stays wide
            o["pred_logits"] = -4.0 + step * (order + 0.6 * torch.rand(bs, Q, K, generator=g) - 0.3)
        if c["keypoints"]:
            for h in heads:
                o[h] = torch.rand(bs, Q, D, generator=g)
                o[h][..., -1] *= c["scale_last"]
        sets.append(o)
    sizes = [c["sizes"][(f + c["seed"]) % len(c["sizes"])] for f in range(bs)]
    labels = [_labels(c, T, g) for T in sizes]
    kps = [torch.rand(T, D, generator=g) for T in sizes]
    for k in kps:
        k[..., -1] *= c["scale_last"]
    if arctic:
        is_valid = torch.ones(bs, dtype=torch.float32)
        is_valid[list(c["invalid"])] = 0
        targets = {"labels": labels, "is_valid": is_valid}
        if c["keypoints"]:
            targets["keypoints"] = kps
        return sets, targets
    targets = []
    for lab, k in zip(labels, kps):
        jv = (torch.rand(len(lab), 21, generator=g) > 0.2).unsqueeze(-1).repeat(1, 1, 3)
        targets.append({"labels": torch.tensor(lab, dtype=torch.int64), "keypoints": k, "joint_valid": jv})
    return sets, targets


def convert(sets, targets, device="cpu", dtype=torch.float32, requires_grad=False):
    """The same inputs on `device` with floating tensors as `dtype` (new leaves)."""
    def leaf(t):
        return t.detach().to(device=device, dtype=dtype).clone().requires_grad_(requires_grad)

    out = [{k: leaf(v) for k, v in o.items()} for o in sets]
    if isinstance(targets, dict):
        t = dict(targets)
        t["is_valid"] = targets["is_valid"].to(device)
        if "keypoints" in t:
            t["keypoints"] = [k.to(device=device, dtype=dtype) for k in targets["keypoints"]]
        return out, t
    return out, [{"labels": d["labels"].to(device), "keypoints": d["keypoints"].to(device=device, dtype=dtype),
                  "joint_valid": d["joint_valid"].to(device)} for d in targets]


def frame_sizes(targets):
    if isinstance(targets, dict):
        return [len(t) for t in targets["labels"]]
    return [len(d["labels"]) for d in targets]


def valid_frames(targets):
    """Slot k pairs output frame k with the targets of valid_frames(targets)[k] (the reference's chunk pairing)."""
    if isinstance(targets, dict):
        return [f for f in range(len(targets["labels"])) if targets["is_valid"][f] == 1]
    return list(range(len(targets)))


def frame_labels(targets, f):
    if isinstance(targets, dict):
        return [int(x) for x in targets["labels"][f]]
    return [int(x) for x in targets[f]["labels"]]


def column_classes(targets, f):
    """Per target of frame f the first target of its class of identical cost columns (see the module docstring)."""
    lab = frame_labels(targets, f)
    has_kp = not isinstance(targets, dict) or "keypoints" in targets
    first = {}
    return [first.setdefault(x, t) if (not has_kp or x == 0) else t for t, x in enumerate(lab)]


def cost_blocks(M, outputs, targets, frames=None, dims=None):
    """The restatement of matcher.arctic_composition / assembly_composition's cost (`M._class_cost`, torch.cdist p=1) per
    slot, in the dtype of `outputs` (fp64 in the tests): a list of [Q, T] tensors, slot k = output frame k against the
    targets of frames[k] (default: the k-th valid frame).  `dims`: keep only the first `dims` keypoint values."""
    frames = valid_frames(targets) if frames is None else frames
    logits = outputs["pred_logits"]
    arctic = isinstance(targets, dict)
    blocks = []
    for k, f in enumerate(frames):
        ids = torch.tensor(frame_labels(targets, f), dtype=torch.int64)
        cost = M._class_cost(logits[k:k + 1], ids)
        if not arctic or "keypoints" in targets:
            tgt = (targets["keypoints"][f] if arctic else targets[f]["keypoints"])[:, :dims]
            kp = torch.zeros_like(cost)
            if arctic:
                hand = (ids == 12) | (ids == 13)
                obj = (ids != 0) & ~hand
                kp[:, hand] = torch.cdist(outputs["pred_hand_key"][k][:, :dims], tgt[hand], p=1)
                kp[:, obj] = torch.cdist(outputs["pred_obj_key"][k][:, :dims], tgt[obj], p=1)
            else:
                kp[:, ids != 0] = torch.cdist(outputs["pred_keypoints"][k][:, :dims], tgt[ids != 0], p=1)
            cost = COST_KEYPOINT * kp + COST_CLASS * cost
        else:
            cost = COST_CLASS * cost
        blocks.append(cost)
    return blocks


def bound(Q, T):
    """2 min(Q, T) EPS: how far two assignments' totals can move, relative to max|C|, when every entry is off by EPS."""
    return 2 * min(Q, T) * EPS


# ---- the bare solver's matrices --------------------------------------------------------------------------------------------
LSAP_KINDS = ("inf", "signed", "big", "tiny", "range", "ties", "dup_rows", "dup_cols")
LSAP_B = 4


def lsap_shapes():
    tall = [(q, t) for q in (1, 3, 16, 64, 300, 1024) for t in (1, 2, 3, 7, 16) if t <= q]
    return tall + [(1, 2), (1, 16), (3, 7), (3, 16), (7, 16), (15, 16)]


def lsap_matrix(kind, Q, T, B=LSAP_B):
    """fp32 [B, Q, T] (numpy PCG64, one seed per kind and shape)."""
    rng = np.random.default_rng(90000 + 10000 * LSAP_KINDS.index(kind) + 17 * Q + T)
    c = rng.random((B, Q, T), dtype=np.float32)
    if kind == "inf":                       # 10-50 % forbidden edges; a planted assignment keeps every block feasible
        for b in range(B):
            keep = np.zeros((Q, T), bool)
            n = min(Q, T)
            keep[rng.permutation(Q)[:n], rng.permutation(T)[:n]] = True
            share = 0.1 + 0.4 * b / max(B - 1, 1)
            c[b][(rng.random((Q, T)) < share) & ~keep] = np.inf
    elif kind == "signed":
        c = c * 2 - 1
    elif kind == "big":
        c = c * np.float32(1e30)
    elif kind == "tiny":
        c = c * np.float32(1e-30)
    elif kind == "range":                   # column t scaled by 10^(-6 .. 6)
        c = c * (10.0 ** np.linspace(-6, 6, T)).astype(np.float32)[rng.permutation(T)]
    elif kind == "ties":
        c = rng.integers(0, 4, size=(B, Q, T)).astype(np.float32)
    elif kind == "dup_rows":                # every row is one of (at most) three
        c = c[:, rng.integers(0, min(Q, 3), size=Q), :]
    elif kind == "dup_cols":
        c = c[:, :, rng.integers(0, min(T, 3), size=T)]
    return np.ascontiguousarray(c, dtype=np.float32)
