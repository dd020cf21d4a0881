#!/usr/bin/env python3
"""Time, host synchronisations and kernels of the ARCTIC small losses of one criterion step: 6 prediction sets
at B frames (B = 32 is window 32), forward + backward with respect to the nine get_arctic_item tensors, on the synthetic MANO
of tests/golden/mano_inputs.py and synthetic objects padded to --obj-len rows (ARCTIC's meshes are not available here; about
4000 is an assumption).

Routes: `restatement` (small_loss_reference per set, MSDA_SMALL_LOSS_FUSED=0: the reference's structure, its gates and boolean
masks, MANO and object layer through the drop-ins), `dropin` (6 per-set compute_small_loss calls) and `many` (one pass over
all sets: one mano_many, one objects_many, one loss node).  Per route: wall ms and GPU ms per step, host syncs per step
(torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler), and the bytes the loss and object kernels must
move (read inputs, write outputs, from the shapes) with their time at the HBM rate.  One JSON line per route, on stdout and
appended to --out (default profiles/small_loss_time.jsonl).

    python tools/small_loss_time.py [--iters N] [--batch 32] [--obj-len 4000] [--only ROUTE] [--out FILE]

`--autocast` times the amp step instead: the six sets as DETR outputs at Q = 300 (fp32 logits, bf16
pred_cams / pred_mano_params / pred_obj_params), ArcticSmallLoss.many forward + backward under bf16 autocast with the selection
inside the timed step.  Routes: `amp_knob_off` (MSDA_SMALL_LOSS_BF16 unset: the restatements), `amp_knob_on` (the grouped bf16
selection and the fp32 nodes) and `fp32_many` (no autocast, `.float()` sources, per-set selection), --runs times each,
interleaved.  A last line, `amp_distance`, gives per key the largest relative distance of the two amp routes from
small_loss_reference in fp64 on the same bf16-valued inputs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import mano_inputs as MI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from smoother_time import count_kernels, count_syncs, measure  # noqa: E402
from uvhand_amd.mano import MANO  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors  # noqa: E402
from uvhand_amd.arctic_item import get_arctic_item_reference  # noqa: E402
from uvhand_amd.small_loss import KEYS, ArcticSmallLoss, compute_small_loss, small_loss_many, small_loss_reference  # noqa: E402

DEV = torch.device("cuda", 0)
SETS = 6
HBM_GBS = 8000.0                                # MI355X peak HBM3E rate, GB/s


def bytes_moved(B, L):
    """Bytes the object and loss kernels of one step must read and write at least (fp32), forward + backward."""
    obj_rows = L + 600 + 16 + 32
    obj = SETS * B * obj_rows * 3 * 4 * 3                        # forward write; backward read of the gradient + template
    loss_in = SETS * B * (2 * (778 + 21) * 3 + (L + 32) * 3) * 4
    loss = loss_in * 3 + SETS * B * L * 3 * 4                   # forward read, backward read + write; smoothing neighbour
    return obj + loss


def detr_sets(preds, Q, seed=33):
    """Per set DETR outputs whose every query holds that frame's prediction plus a little noise, rounded to bf16: whichever
    queries the random logits select, the small losses see inputs of the usual size."""
    g = torch.Generator().manual_seed(seed)
    sets = []
    for p in preds:
        (rl, rr, ro), (pl, pr), (bl, br), (rot, rad) = [[t.detach().cpu() for t in grp] for grp in p]
        B = rl.shape[0]
        spread = lambda a, b: (torch.where(torch.rand(B, Q, 1, generator=g) < 0.5, a[:, None, :], b[:, None, :])  # noqa: E731
                               + 0.01 * torch.randn(B, Q, a.shape[1], generator=g))
        srcs = [spread(rl, rr), spread(ro, ro), spread(pl, pr), spread(bl, br), spread(rad.reshape(B, 1), rad.reshape(B, 1)),
                spread(rot.reshape(B, 3), rot.reshape(B, 3))]
        leaf = lambda t: t.to(torch.bfloat16).to(DEV).requires_grad_(True)  # noqa: E731
        hc, oc, mp, ms, orad, orot = [leaf(t) for t in srcs]
        sets.append({"pred_logits": (torch.randn(B, Q, 14, generator=g) * 2).to(DEV), "pred_cams": [hc, oc],
                     "pred_mano_params": [mp, ms], "pred_obj_params": [orad, orot]})
    return sets


def _sources(o):
    return o["pred_cams"] + o["pred_mano_params"] + o["pred_obj_params"]


def autocast_routes(args, m, preds, gt, meta):
    import types
    B, L, Q = args.batch, args.obj_len, 300
    cfg = types.SimpleNamespace(hand_idx=[12, 13])
    crit_args = types.SimpleNamespace(img_res=SI.IMG_RES, device=DEV)
    small = ArcticSmallLoss(m, cfg)
    suffixes = [""] + ["_%d" % i for i in range(SETS - 1)]
    bf16_sets = detr_sets(preds, Q)
    f32_sets = [dict(o, pred_cams=[t.detach().float().requires_grad_(True) for t in o["pred_cams"]],
                     pred_mano_params=[t.detach().float().requires_grad_(True) for t in o["pred_mano_params"]],
                     pred_obj_params=[t.detach().float().requires_grad_(True) for t in o["pred_obj_params"]]) for o in bf16_sets]

    def run(route, backward=True):
        sets = f32_sets if route == "fp32_many" else bf16_sets
        if route == "amp_knob_on":
            os.environ["MSDA_SMALL_LOSS_BF16"] = "1"
        else:
            os.environ.pop("MSDA_SMALL_LOSS_BF16", None)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=route != "fp32_many"):
            ds = small.many(sets, gt, meta, crit_args, suffixes)
            loss = sum(v.sum() for d in ds for v in d.values())
        if backward:
            torch.autograd.grad(loss, [t for o in sets for t in _sources(o)], allow_unused=True)
        return ds

    routes = ("amp_knob_off", "amp_knob_on", "fp32_many")
    with open(args.out, "a") as f:
        for rep in range(args.runs):
            for route in routes:
                if args.only and route != args.only:
                    continue
                step = lambda: run(route)  # noqa: E731
                wall, gpu = measure(step, args.iters)
                line = json.dumps({"tool": "small_loss_time", "mode": "autocast", "route": route, "run": rep, "sets": SETS,
                                   "batch": B, "queries": Q, "obj_len": L, "wall_ms_per_step": round(wall, 4),
                                   "gpu_event_ms_per_step": round(gpu, 4), "host_syncs_per_step": count_syncs(step),
                                   "kernels_per_step": count_kernels(step), "iters": args.iters,
                                   "device": torch.cuda.get_device_name(DEV)})
                print(line, flush=True)
                f.write(line + "\n")
        # for the record: what the autocast composition's bf16 products cost, against fp64 on the same bf16-valued inputs
        with torch.no_grad():
            ref = [small_loss_reference(get_arctic_item_reference(o, cfg), gt, meta, m, SI.IMG_RES, dtype=torch.float64)
                   for o in f32_sets]
            dist = {}
            for route in routes[:2]:
                ds = run(route, backward=False)
                dist[route] = {k: max(float(((d[k + sfx].double().reshape(-1) - r[k].reshape(-1)).abs()
                                             / r[k].reshape(-1).abs().clamp_min(1e-30)).max())
                                      for d, r, sfx in zip(ds, ref, suffixes)) for k in KEYS}
        line = json.dumps({"tool": "small_loss_time", "mode": "autocast", "route": "amp_distance", "sets": SETS, "batch": B,
                           "queries": Q, "obj_len": L, "max_rel_distance_from_fp64": dist})
        print(line, flush=True)
        f.write(line + "\n")
    os.environ.pop("MSDA_SMALL_LOSS_BF16", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--obj-len", type=int, default=4000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--autocast", action="store_true", help="the amp step: knob off, knob on, and the fp32 many route")
    ap.add_argument("--runs", type=int, default=3, help="--autocast: runs of each route, interleaved")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_loss_time.jsonl"))
    args = ap.parse_args()
    B, L = args.batch, args.obj_len
    m = {"mano_l": MANO.from_arrays(**MI.model_arrays("left", dtype=torch.float32), is_rhand=False).to(DEV),
         "mano_r": MANO.from_arrays(**MI.model_arrays("right", dtype=torch.float32)).to(DEV),
         "arti_head": ObjectTensors.from_arrays(SI.obj_arrays(lengths=[L - 37 * i for i in range(11)])).to(DEV)}
    pred, gt, meta = SI.case_inputs("partial", B=B, seed=31)
    g = torch.Generator().manual_seed(32)
    for k in ("ro", "lo"):
        gt["idx." + k] = torch.randint(0, L - 400, gt["idx." + k].shape, generator=g)
    gt = {k: v.to(DEV) for k, v in gt.items()}
    meta = dict(meta, intrinsics=meta["intrinsics"].to(DEV))
    preds = []
    for s in range(SETS):
        p = pred if s == 0 else SI.case_inputs("partial", B=B, seed=31 + 10 * s, objects=meta["query_names"])[0]
        preds.append(SI.unflat_pred([t.to(DEV).requires_grad_(True) for t in SI.flat_pred(p)]))
    if args.autocast:
        return autocast_routes(args, m, preds, gt, meta)
    leaves = [t for p in preds for t in SI.flat_pred(p)]
    nbytes = bytes_moved(B, L)
    for route in ("restatement", "dropin", "many"):
        if args.only and route != args.only:
            continue
        os.environ["MSDA_SMALL_LOSS_FUSED"] = "0" if route == "restatement" else "1"

        def step():
            if route == "many":
                ds = small_loss_many(preds, gt, meta, m, SI.IMG_RES)
            elif route == "dropin":
                ds = [compute_small_loss(p, gt, meta, m, SI.IMG_RES) for p in preds]
            else:
                ds = [small_loss_reference(p, gt, meta, m, SI.IMG_RES) for p in preds]
            loss = sum(d[k].sum() for d in ds for k in KEYS)
            torch.autograd.grad(loss, leaves, allow_unused=True)

        wall, gpu = measure(step, args.iters)
        line = json.dumps({"tool": "small_loss_time", "route": route, "sets": SETS, "batch": B, "obj_len": L,
                           "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                           "host_syncs_per_step": count_syncs(step), "kernels_per_step": count_kernels(step),
                           "object_and_loss_bytes": nbytes, "hbm_bound_ms": round(nbytes / (HBM_GBS * 1e6), 4),
                           "iters": args.iters, "device": torch.cuda.get_device_name(DEV)})
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    os.environ.pop("MSDA_SMALL_LOSS_FUSED", None)


if __name__ == "__main__":
    main()
