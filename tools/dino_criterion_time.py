#!/usr/bin/env python3
"""Time, kernels, host synchronisations and library launches of DINO's criterion in one window-32 step, forward
+ backward of the weighted total: 32 frames x 900 queries x 3 targets, 14 classes, 42 keypoint values, the 7 matched sets
(final, 5 aux, interm) and the denoising set of 33 groups x single_pad 6 = 198 queries, losses ['labels', 'boxes',
'cardinality'].

routes: `composition` — SetDinoCriterion's torch restatement (the matcher's torch + scipy composition per set, host index
lists, the denoising lists of dino.py:620-634; MSDA_MATCHER_FUSED and MSDA_CRITERION_FUSED off); `drop_in` — SetDinoCriterion
as it ships (one pack_targets, one match, one dino_set_losses, class_error from the match result); `set_losses` — bare match +
dino_set_losses + backward on targets packed once (what a captured step runs).

Three runs of each route, interleaved, in one process.  Per run: wall ms per step, GPU ms from device events, host syncs per
step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler) and library launches per step
(msda_launch_count); then one `summary` row per route with the median of the three runs beside the runs.  One JSON line each,
on stdout and appended to --out.  `--route NAME --steps N` runs one route N times and nothing else: the command a rocprofv3
kernel-trace run of its own wraps for profiles/dino_criterion_kernel_stats.csv.

    python tools/dino_criterion_time.py [--iters N] [--out FILE] [--route NAME --steps N]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from detr_time import DEV, count_kernels, count_syncs, measure  # noqa: E402
from uvhand_amd import _native as MSDA  # noqa: E402
from uvhand_amd import criterion as C  # noqa: E402
from uvhand_amd import matcher as M  # noqa: E402

BS, Q, T, K, D, AUX, GROUPS, SINGLE_PAD = 32, 900, 3, 14, 42, 5, 33, 6
LOSSES = ["labels", "boxes", "cardinality"]
ROUTES = ("composition", "drop_in", "set_losses")
COST_CLASS, COST_BBOX = 2.0, 5.0


def _set(g, q):
    return {"pred_logits": (torch.randn(BS, q, K, generator=g) * 2).to(DEV).requires_grad_(True),
            "pred_hand_key": torch.rand(BS, q, D, generator=g).to(DEV).requires_grad_(True),
            "pred_obj_key": torch.rand(BS, q, D, generator=g).to(DEV).requires_grad_(True)}


def weights():
    base = {"loss_ce": 2.0, "loss_hand_keypoint": 5.0, "loss_obj_keypoint": 5.0, "cardinality_error": 1.0}
    w = dict(base)
    for sfx in [f"_{i}" for i in range(AUX)] + ["_interm", "_dn"]:
        w.update({k + sfx: v for k, v in base.items()})
    return w


def build():
    g = torch.Generator().manual_seed(0)
    sets = [_set(g, Q) for _ in range(AUX + 2)]
    dn = _set(g, GROUPS * SINGLE_PAD)
    outputs = dict(sets[0], aux_outputs=sets[1:1 + AUX], interm_outputs=sets[-1],
                   dn_meta={"pad_size": GROUPS * SINGLE_PAD, "num_dn_group": GROUPS, "output_known_lbs_bboxes": dn})
    targets = {"labels": [[12, 13, int(torch.randint(1, 12, (1,), generator=g))] for _ in range(BS)],
               "keypoints": [torch.rand(T, D, generator=g).to(DEV) for _ in range(BS)], "is_valid": torch.ones(BS, device=DEV)}
    leaves = [s[k] for s in sets + [dn] for k in ("pred_logits", "pred_hand_key", "pred_obj_key")]
    w = weights()
    crit = C.SetDinoCriterion(K, M.DinoHungarianMatcher(COST_CLASS, COST_BBOX), w, 0.25, LOSSES, None, None,
                              small_loss=lambda *a: {}).train()
    wt = torch.tensor([[w["loss_ce"], w["loss_hand_keypoint"], w["loss_obj_keypoint"], 0.0]] * (len(sets) + 1), device=DEV)
    packed = M.pack_targets(targets, DEV)
    nb = torch.full((1,), float(BS * T), device=DEV)

    def drop_in():
        d = crit(outputs, targets, None, None)
        torch.autograd.grad(sum(d[k] * w[k] for k in d if k in w), leaves)

    def composition():
        M.FUSED = False
        os.environ["MSDA_CRITERION_FUSED"] = "0"
        try:
            drop_in()
        finally:
            M.FUSED = True
            os.environ.pop("MSDA_CRITERION_FUSED")

    def set_losses():
        res = M.match(sets, packed, COST_CLASS, COST_BBOX)
        out = C.dino_set_losses(sets, packed, res, nb, [dn], SINGLE_PAD, GROUPS)
        torch.autograd.grad((out.losses * wt).sum(), leaves)

    return {"composition": composition, "drop_in": drop_in, "set_losses": set_losses}


def count_launches(fn):
    n0 = MSDA.launch_count()
    fn()
    return MSDA.launch_count() - n0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino_criterion_time.jsonl"))
    ap.add_argument("--route", default=None, choices=ROUTES)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    steps = build()
    if args.route:                                                    # for a kernel trace: this route alone
        for _ in range(args.steps):
            steps[args.route]()
        torch.cuda.synchronize()
        return

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    gpu_ms = {r: [] for r in ROUTES}
    wall_ms = {r: [] for r in ROUTES}
    last = {}
    for run in range(3):                                              # the routes interleaved, run by run
        for route in ROUTES:
            fn = steps[route]
            iters = max(2, args.iters // 5) if route == "composition" else args.iters
            wall, gpu = measure(fn, iters)
            gpu_ms[route].append(round(gpu, 4))
            wall_ms[route].append(round(wall, 4))
            last[route] = {"tool": "dino_criterion_time", "route": route, "frames": BS, "queries": Q, "targets_per_frame": T,
                           "classes": K, "matched_sets": AUX + 2, "dn_groups": GROUPS, "single_pad": SINGLE_PAD, "iters": iters,
                           "device": torch.cuda.get_device_name(DEV), "host_syncs_per_step": count_syncs(fn),
                           "kernels_per_step": count_kernels(fn), "library_launches_per_step": count_launches(fn)}
            emit(dict(last[route], run=run, wall_ms_per_step=round(wall, 4), gpu_event_ms_per_step=round(gpu, 4)))
    for route in ROUTES:
        emit(dict(last[route], run="summary", gpu_event_ms_median=statistics.median(gpu_ms[route]), gpu_event_ms_runs=gpu_ms[route],
                  wall_ms_median=statistics.median(wall_ms[route]), wall_ms_runs=wall_ms[route]))


if __name__ == "__main__":
    main()
