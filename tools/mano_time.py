#!/usr/bin/env python3
"""Time, host synchronisations and kernels of the MANO calls of one ARCTIC criterion step: 6 prediction
sets x left / right hands at B hands each (B = 32 is window 32), forward + backward with respect to betas, global_orient and
hand_pose, on the synthetic MANO of tests/golden/mano_inputs.py (MANO's sizes).

Routes: `composition` (the torch restatement of smplx's lbs, MSDA_MANO_FUSED=0: smplx's kernel structure, 12 separate calls),
`dropin` (12 separate drop-in MANO calls: 12 forward and 24 backward HIP launches) and `many` (one mano_many: 1 forward and
2 backward launches).  Per route and batch: wall ms per step (host clock around the steps, ending in a device synchronise),
GPU ms from device events, host syncs per step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler),
and the kernels' own bound: model bytes each hand tile streams and FLOPs per hand.  One JSON line per route and batch, on
stdout and appended to --out (default profiles/mano_time.jsonl).

    python tools/mano_time.py [--iters N] [--batches 32,256] [--only composition|dropin|many] [--out FILE]"""
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
from smoother_time import count_kernels, count_syncs, measure  # noqa: E402
from uvhand_amd.mano import MANO, mano_many  # noqa: E402

DEV = torch.device("cuda", 0)
SETS = 6
HAND_TILE, SLICE = 8, 64                      # csrc/msda_mano.hip kHT, kVS


def bound(B):
    """(model bytes one hand tile streams, forward FLOPs per hand, forward model bytes of the whole step)."""
    V, NB, P, J = MI.V, MI.NB, MI.NPF, MI.NJ
    tile_bytes = 4 * (P * 3 * V + 3 * V * NB + 3 * V + V * J)
    flops = 2 * 3 * V * (P + NB) + V * (2 * J * 12 + 2 * 12)
    tiles = 2 * SETS * -(-B // HAND_TILE)
    return tile_bytes, flops, tiles * tile_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mano_time.jsonl"))
    args = ap.parse_args()
    layers = {s: MANO.from_arrays(**MI.model_arrays(s, dtype=torch.float32)).to(DEV) for s in ("left", "right")}
    for B in [int(b) for b in args.batches.split(",")]:
        calls = []
        for i in range(2 * SETS):
            betas, go, hp = MI.pose_inputs(900 + i, B)
            calls.append((layers["right" if i % 2 else "left"],) + tuple(t.float().to(DEV).requires_grad_(True)
                                                                         for t in (betas, go, hp)))
        leaves = [t for c in calls for t in c[1:]]
        for route in ("composition", "dropin", "many"):
            if args.only and route != args.only:
                continue
            os.environ["MSDA_MANO_FUSED"] = "0" if route == "composition" else "1"

            def step():
                outs = mano_many(calls) if route == "many" else [c[0](*c[1:]) for c in calls]
                loss = sum(o.vertices.square().sum() + o.joints.sum() for o in outs)
                torch.autograd.grad(loss, leaves)

            wall, gpu = measure(step, args.iters)
            tile_bytes, flops, fwd_bytes = bound(B)
            line = json.dumps({"tool": "mano_time", "route": route, "batch": B, "calls": 2 * SETS,
                               "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                               "host_syncs_per_step": count_syncs(step), "kernels_per_step": count_kernels(step),
                               "model_bytes_per_hand_tile": tile_bytes, "fwd_flops_per_hand": flops,
                               "fwd_model_bytes_streamed": fwd_bytes, "iters": args.iters,
                               "device": torch.cuda.get_device_name(DEV)})
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    os.environ.pop("MSDA_MANO_FUSED", None)


if __name__ == "__main__":
    main()
