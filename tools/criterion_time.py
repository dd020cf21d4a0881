#!/usr/bin/env python3
"""Time and host synchronisations of the set criterion's DETR half in one window-32 ARCTIC step: 32 frames x
300 queries x 3 targets, 14 classes, 42 keypoint values, the 7 prediction sets SetArcticCriterion takes (final, 5 aux,
interm), losses ['labels', 'boxes', 'cardinality'], forward + backward of the weighted total:

  reference   the reference composition: the matcher's torch + scipy composition per set, then the torch restatement of
              the losses (MSDA_MATCHER_FUSED and MSDA_CRITERION_FUSED off)
  dropin      uvhand_amd.criterion.SetArcticCriterion (one match, one loss launch), weighted sum, backward
  set_losses  pack_targets + match + set_losses + backward (the device API a captured step would run)

Per route: wall ms per step (host clock around the step, ending in a device synchronise), GPU ms from device events around
the step, and host syncs per step (torch.cuda.set_sync_debug_mode("warn")).  One JSON line per route, on stdout and appended
to --out (default profiles/criterion_time.jsonl).  The MANO / ARCTIC small losses are not part of any route.

    python tools/criterion_time.py [--iters N] [--only NAME] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from uvhand_amd import criterion as C  # noqa: E402
from uvhand_amd import matcher as M  # noqa: E402

DEV = torch.device("cuda", 0)
BS, Q, T, K, D, SETS = 32, 300, 3, 14, 42, 7
LOSSES = ["labels", "boxes", "cardinality"]


def inputs():
    g = torch.Generator().manual_seed(0)
    sets = [{"pred_logits": (torch.randn(BS, Q, K, generator=g) * 2).to(DEV).requires_grad_(True),
             "pred_hand_key": torch.rand(BS, Q, D, generator=g).to(DEV).requires_grad_(True),
             "pred_obj_key": torch.rand(BS, Q, D, generator=g).to(DEV).requires_grad_(True)} for _ in range(SETS)]
    outputs = dict(sets[0], aux_outputs=sets[1:6], interm_outputs=sets[6])
    labels = [[12, 13, int(torch.randint(1, 12, (1,), generator=g))] for _ in range(BS)]
    targets = {"labels": labels, "keypoints": [torch.rand(T, D, generator=g).to(DEV) for _ in range(BS)],
               "is_valid": torch.ones(BS, device=DEV)}
    return sets, outputs, targets


def weights():
    base = {"loss_ce": 2.0, "loss_hand_keypoint": 5.0, "loss_obj_keypoint": 5.0, "cardinality_error": 1.0}
    w = dict(base)
    for sfx in [f"_{i}" for i in range(5)] + ["_interm"]:
        w.update({k + sfx: v for k, v in base.items()})
    return w


def count_syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(0)
    return sum("synchroniz" in str(w.message) for w in caught)


def measure(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return wall, a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "criterion_time.jsonl"))
    args = ap.parse_args()
    sets, outputs, targets = inputs()
    leaves = [s[k] for s in sets for k in ("pred_logits", "pred_hand_key", "pred_obj_key")]
    w = weights()
    crit = C.SetArcticCriterion(K, M.ArcticMatcher(1.5, 4.0), w, LOSSES, small_loss=lambda *a: {})
    wt = torch.tensor([[w["loss_ce"], w["loss_hand_keypoint"], w["loss_obj_keypoint"], 0.0]] * SETS, device=DEV)

    def dropin():
        d = crit(outputs, targets, None, None)
        torch.autograd.grad(sum(d[k] * w[k] for k in d if k in w), leaves)

    def reference():
        M.FUSED = False
        os.environ["MSDA_CRITERION_FUSED"] = "0"
        try:
            dropin()
        finally:
            M.FUSED = True
            os.environ.pop("MSDA_CRITERION_FUSED")

    def set_losses():
        packed = M.pack_targets(targets, DEV)
        res = M.match(sets, packed, 1.5, 4.0)
        out = C.set_losses(sets, packed, res, torch.full((1,), float(BS * T), device=DEV), "arctic")
        torch.autograd.grad((out.losses * wt).sum(), leaves)

    steps = {"reference": reference, "dropin": dropin, "set_losses": set_losses}
    for name, fn in steps.items():
        if args.only and name != args.only:
            continue
        wall, gpu = measure(fn, args.iters)
        line = json.dumps({"tool": "criterion_time", "figure": name, "frames": BS, "queries": Q, "targets": T, "classes": K,
                           "sets": SETS, "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                           "host_syncs_per_step": count_syncs(fn), "iters": args.iters,
                           "device": torch.cuda.get_device_name(DEV)})
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
