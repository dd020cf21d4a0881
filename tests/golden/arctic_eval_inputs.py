"""Seeded synthetic inputs of the ARCTIC evaluation fixtures (gen_arctic_eval.py) and of tests/test_arctic_eval*.py, built on
small_loss_inputs.py (synthetic objects, targets) and mano_inputs.py (MANO models): a [B, Q, C] DETR output dict for
get_arctic_item, the targets with gt ``object.v.cam`` / ``object.v_len`` / ``object.parts_ids`` / ``object.diameter`` and every
normalised 2d key prepare_data de-normalises, and the meta_info of arctic_pre_process (``part_ids``, ``diameter``,
``object.v_len``).  Hand and object gt live in camera space at the depth their weak-perspective cameras give (z of 10 to 20 m).
In the first half of the frames the gt object pose is the selected prediction's plus a small perturbation, so that the v2v
success rate is neither 0 nor 100 there.  Shared by the generator and the tests: nothing at test time reads the reference."""
import types

import torch

import mano_inputs as MI
import small_loss_inputs as SI
from uvhand_amd.arctic_item import get_arctic_item_reference
from uvhand_amd.mano import MANO
from uvhand_amd.object_tensors import object_tensors_reference
from uvhand_amd.small_loss import weak_perspective_to_perspective

CASES = {"all_valid": 1901, "left_invalid": 1902, "right_invalid": 1903, "partial": 1904, "no_contact": 1905}
SEQUENCE = ("all_valid", "no_contact", "partial", "left_invalid", "right_invalid")     # the evaluator's steps
Q, NUM_CLASSES = 5, 14
CFG = types.SimpleNamespace(hand_idx=[12, 13])
FOCAL = 1000.0
NN_SEED = 1950
# the realistic-size case of the GPU tests: objects of about 4000 rows, no vertex within BIG_MARGIN of its success threshold
BIG = dict(case="partial", B=32, seed=31, margin=2e-3)
BIG_LENGTHS = [4000 - 37 * i for i in range(11)]
BIG_MARGIN = 1e-3          # what the tests assert in fp64 (the inputs are built with twice that)


def args(device="cpu"):
    return types.SimpleNamespace(focal_length=FOCAL, img_res=SI.IMG_RES, device=device)


def mano_models(device="cpu"):
    return {"mano_l": MANO.from_arrays(**MI.model_arrays("left", dtype=torch.float32), is_rhand=False).to(device),
            "mano_r": MANO.from_arrays(**MI.model_arrays("right", dtype=torch.float32)).to(device)}


def success_margin(gt_v, pred_v, v_len, part_ids, diameter):
    """fp64, from the data alone: per frame the smallest |dist - threshold| / threshold over the real rows of eval_v2v_success's
    root-relative vertex distance (threshold 0.05 x diameter); also the per-row distances' list for the callers that move rows."""
    margins, dists = [], []
    for b in range(gt_v.shape[0]):
        n = int(v_len[b])
        g, p = gt_v[b, :n].double(), pred_v[b, :n].double()
        bot = part_ids[b, :n] == 2
        d = ((g - g[bot].mean(0)) - (p - p[bot].mean(0))).norm(dim=1)
        thr = float(diameter[b]) * 0.05
        margins.append(float(((d - thr).abs() / thr).min()))
        dists.append((d, thr))
    return torch.tensor(margins, dtype=torch.float64), dists


def _clear_thresholds(gt_v, pred_v, v_len, part_ids, diameter, margin):
    """Move every gt row whose fp64 distance lies within `margin` (relative) of its success threshold radially by 4 x margin x
    threshold, away from the threshold; repeated because the object root moves with the bottom rows (by far less)."""
    for _ in range(4):
        m, dists = success_margin(gt_v, pred_v, v_len, part_ids, diameter)
        if float(m.min()) > margin:
            return gt_v
        for b, (d, thr) in enumerate(dists):
            n = int(v_len[b])
            near = ((d - thr).abs() <= margin * thr).nonzero().view(-1)
            if near.numel() == 0:
                continue
            g, p = gt_v[b, :n].double(), pred_v[b, :n].double()
            bot = part_ids[b, :n] == 2
            diff = (g - g[bot].mean(0)) - (p - p[bot].mean(0))
            step = torch.where(d[near] >= thr, 1.0, -1.0) * 4 * margin * thr
            gt_v[b, near] = (g[near] + diff[near] / d[near, None] * step[:, None]).float()
    raise AssertionError("rows remain on their success threshold")


def case_inputs(case, B=SI.FIXTURE_B, lengths=None, seed=None, margin=None):
    """(outputs, targets, meta_info) in fp32 on the CPU.  `margin`: no gt vertex within that relative distance of its success
    threshold (in fp64, against the prediction computed by the torch restatements); None leaves the rows as drawn."""
    seed = CASES[case] if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    per_q = [SI.case_inputs(case, B=B, seed=seed + 10 * (q + 1)) for q in range(Q)]
    _, gt, meta = SI.case_inputs(case, B=B, seed=seed)
    st = lambda pick: torch.stack([pick(p[0]) for p in per_q], dim=1)  # noqa: E731
    outputs = {"pred_logits": torch.randn(B, Q, NUM_CLASSES, generator=g),
               "pred_cams": [st(lambda p: p[0][0]), st(lambda p: p[0][2])],
               "pred_mano_params": [st(lambda p: p[1][0]), st(lambda p: p[2][0])],
               "pred_obj_params": [st(lambda p: p[3][1]), st(lambda p: p[3][0])]}
    ot = SI.obj_arrays(lengths=lengths)
    idx = torch.tensor([SI.OBJECTS.index(n) for n in meta["query_names"]])
    v_len = ot["v_len"][idx]
    max_len = int(v_len.max())
    K = meta["intrinsics"]
    focal = (K[:, 0, 0] + K[:, 1, 1]) / 2.0
    items = get_arctic_item_reference(outputs, CFG)
    half = B // 2
    gt["object.rot"][:half] = items[3][0][:half] + 0.02 * torch.randn(half, 3, generator=g)
    gt["object.radian"][:half] = items[3][1][:half, 0] + 0.02 * torch.randn(half, generator=g)
    o = object_tensors_reference(ot, gt["object.radian"].view(-1, 1), gt["object.rot"], None, idx, max_len)
    gt["object.v.cam"] = o["v"] + weak_perspective_to_perspective(gt["object.cam_t.wp"], focal, SI.IMG_RES)[:, None, :]
    if margin is not None:
        pred_o = object_tensors_reference(ot, items[3][1].view(-1, 1), items[3][0], None, idx, max_len)["v"] \
            + weak_perspective_to_perspective(items[0][2], focal, SI.IMG_RES)[:, None, :]
        gt["object.v.cam"] = _clear_thresholds(gt["object.v.cam"], pred_o, v_len, o["parts_ids"], o["diameter"], margin)
    gt["object.v_len"] = v_len
    gt["object.parts_ids"] = o["parts_ids"]
    gt["object.diameter"] = o["diameter"]
    for s in ("l", "r"):
        gt["mano.j3d.cam." + s] = gt["mano.j3d.cam." + s] \
            + weak_perspective_to_perspective(gt["mano.cam_t.wp." + s], focal, SI.IMG_RES)[:, None, :]
    if lengths is not None:                       # contact indices over the whole (longer) object
        for k in ("ro", "lo"):
            gt["idx." + k] = torch.randint(0, int(v_len.min()), gt["idx." + k].shape, generator=g)
    gt["object.kp2d.norm"] = torch.cat((gt["object.kp2d.norm.t"], gt["object.kp2d.norm.b"]), dim=1)
    gt["object.bbox2d.norm.t"] = 0.5 * torch.randn(B, SI.NB_BOX, 2, generator=g)
    gt["object.bbox2d.norm.b"] = 0.5 * torch.randn(B, SI.NB_BOX, 2, generator=g)
    meta = dict(meta, **{"object.v_len": gt["object.v_len"], "part_ids": gt["object.parts_ids"], "diameter": gt["object.diameter"]})
    return outputs, gt, meta


def to_device(outputs, targets, meta, dev):
    mv = lambda v: v.to(dev) if torch.is_tensor(v) else ([mv(x) for x in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else v)  # noqa: E731
    return ({k: mv(v) for k, v in outputs.items()}, {k: mv(v) for k, v in targets.items()}, {k: mv(v) for k, v in meta.items()})


def nn_inputs(seed, B, N1, N2, pairs=2, dtype=torch.float32):
    """Camera-space clouds for the nearest-neighbour tests: an object of 0.15 m spread and hands of 0.06 m around it, all offset
    by a cam_t with z = 12 m.  fp32 values (exactly representable in fp64)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(pairs):
        cam_t = torch.tensor([0.1, -0.05, 12.0]) + 0.05 * torch.randn(B, 1, 3, generator=g)
        src = 0.15 * torch.randn(B, N1, 3, generator=g) + cam_t
        trg = 0.06 * torch.randn(B, N2, 3, generator=g) + cam_t + 0.05 * torch.randn(B, 1, 3, generator=g)
        out.append((src.float().to(dtype), trg.float().to(dtype)))
    return out


def nn_yardstick(src, trg, chunk=250):
    """fp64 brute force: (argmin index [B, N1], squared distance there, relative gap between the best and second-best squared
    distance) for fp64 clouds."""
    idx, best, gap = [], [], []
    for i0 in range(0, src.shape[1], chunk):
        d = ((src[:, i0:i0 + chunk, None, :] - trg[:, None, :, :]) ** 2).sum(-1)
        two, ind = torch.topk(d, 2, dim=2, largest=False)
        first = torch.where(d == two[..., :1], torch.arange(d.shape[2], device=d.device), d.shape[2]).min(dim=2).values
        idx.append(first)
        best.append(two[..., 0])
        gap.append((two[..., 1] - two[..., 0]) / two[..., 1].clamp(min=1e-300))
    return torch.cat(idx, 1), torch.cat(best, 1), torch.cat(gap, 1)
