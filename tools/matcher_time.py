#!/usr/bin/env python3
"""Time and host synchronisations of the Hungarian matching in one window-32 criterion step: 32 frames x
300 queries x 3 targets, 14 classes, the 7 prediction sets SetArcticCriterion matches (final, 5 aux, interm):

  reference  the reference's composition x 7 (torch cost matrix, .cpu(), scipy per frame; MSDA_MATCHER_FUSED off)
  dropin     uvhand_amd.matcher.ArcticMatcher x 7 (one launch + one copy each)
  match      one uvhand_amd.matcher.match() over the 7 sets, then one copy of its result to the host
  match_only the match() launch alone (what a captured step pays)

Per figure: wall ms per step (host clock around the step, ending in a device synchronise), GPU ms from device events
around the step, and host syncs per step (torch.cuda.set_sync_debug_mode("warn")).  One JSON line per figure, on stdout
and appended to --out (default profiles/matcher_time.jsonl).

    python tools/matcher_time.py [--iters N] [--only NAME] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from uvhand_amd import matcher as M  # noqa: E402

DEV = torch.device("cuda", 0)
BS, Q, T, K, D, SETS = 32, 300, 3, 14, 42, 7


def inputs():
    g = torch.Generator().manual_seed(0)
    sets = [{"pred_logits": torch.randn(BS, Q, K, generator=g).to(DEV) * 2,
             "pred_hand_key": torch.rand(BS, Q, D, generator=g).to(DEV),
             "pred_obj_key": torch.rand(BS, Q, D, generator=g).to(DEV)} for _ in range(SETS)]
    labels = [[12, 13, int(torch.randint(1, 12, (1,), generator=g))] for _ in range(BS)]
    targets = {"labels": labels, "keypoints": [torch.rand(T, D, generator=g).to(DEV) for _ in range(BS)],
               "is_valid": torch.ones(BS, device=DEV)}
    return sets, targets


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matcher_time.jsonl"))
    args = ap.parse_args()
    sets, targets = inputs()
    fused = M.ArcticMatcher(1.5, 4.0)
    steps = {
        "reference": lambda: [M.arctic_composition(s, targets, 1.5, 4.0) for s in sets],
        "dropin": lambda: [fused(s, targets) for s in sets],
        "match": lambda: M.match(sets, M.pack_targets(targets, DEV), 1.5, 4.0).buffer.cpu(),
        "match_only": lambda: M.match(sets, packed, 1.5, 4.0),
    }
    packed = M.pack_targets(targets, DEV)
    ref = steps["reference"]()
    assert [[(a.tolist(), b.tolist()) for a, b in r] for r in ref] == \
           [[(a.tolist(), b.tolist()) for a, b in r] for r in steps["dropin"]()], "drop-in differs from the composition"
    for name, fn in steps.items():
        if args.only and name != args.only:
            continue
        wall, gpu = measure(fn, args.iters)
        line = json.dumps({"tool": "matcher_time", "figure": name, "frames": BS, "queries": Q, "targets": T, "classes": K,
                           "sets": SETS, "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                           "host_syncs_per_step": count_syncs(fn), "iters": args.iters,
                           "device": torch.cuda.get_device_name(DEV)})
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
