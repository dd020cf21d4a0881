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

    python tools/small_loss_time.py [--iters N] [--batch 32] [--obj-len 4000] [--only ROUTE] [--out FILE]"""
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
from uvhand_amd.small_loss import KEYS, compute_small_loss, small_loss_many, small_loss_reference  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--obj-len", type=int, default=4000)
    ap.add_argument("--only", default=None)
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
