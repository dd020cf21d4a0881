#!/usr/bin/env python3
"""Time, host synchronisations and kernels of the SmoothNet criterion on one window-32 step: N = 32 frames,
synthetic MANO of tests/golden/mano_inputs.py and synthetic objects padded to --obj-len rows (ARCTIC's meshes are not
available here; about 4000 is an assumption), forward + backward, --runs times in one session.

Routes: `restatement` (MSDA_SMOOTH_LOSS_FUSED=0: the torch restatement with the reference's structure: `.nonzero()`-style
gates, the validity vectors copied to the host, the "any non-NaN" tests), `dropin` (compute_smoothnet_loss with the kernels of
csrc/msda_smooth_loss.hip; `dropin_acc_grad` the same with acc_grad=True), `train` (the SmoothNet-style step of README
"make_output's pose, camera and projection glue" with the drop-in criterion attached: the nine get_arctic_item tensors require
grad, make_output, prepare_data(flag='train'), SmoothCriterion, the weighted sum, backward) and `train_graph` (that step
captured once as one graph and replayed).  Per route: wall ms per step and the device-event interval per step, host syncs per
step (torch.cuda.set_sync_debug_mode("warn")) and kernels per step (torch.profiler).  One JSON line per route and run, on stdout
and appended to --out (default profiles/smooth_loss_time.jsonl), then one line with the four kernels' own durations in a trace.

    python tools/smooth_loss_time.py [--iters N] [--batch 32] [--obj-len 4000] [--only ROUTE] [--out FILE] [--runs 3]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import arctic_eval_inputs as EI  # noqa: E402
import smooth_loss_inputs as MI  # noqa: E402
from smoother_time import count_kernels, count_syncs, measure  # noqa: E402
from uvhand_amd import arctic_eval as AE  # noqa: E402
from uvhand_amd import smooth_loss as SL  # noqa: E402
from uvhand_amd.modules import SmoothCriterion  # noqa: E402

DEV = torch.device("cuda", 0)
WEIGHTS = {"loss/cd": 10.0, "acc/h": 1, "acc/o": 1}       # util/scripts.py:16-29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--obj-len", type=int, default=4000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_loss_time.jsonl"))
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    B, L = a.batch, a.obj_len
    lengths = [L - 37 * i for i in range(11)]
    m = MI.models(DEV, lengths=lengths)
    outputs, targets, meta = EI.to_device(*MI.raw_inputs("all_valid", B=B, lengths=lengths, seed=31), DEV)
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    meta = dict(meta, obj_idx=idx, max_len=max_len)
    args = EI.args(DEV)
    items = AE.get_arctic_item(outputs, EI.CFG, DEV)
    leaves = [[t.detach().clone().requires_grad_(True) for t in grp] for grp in items]
    flat = [t for grp in leaves for t in grp]
    crit = SmoothCriterion(1, B, WEIGHTS, m)
    with torch.no_grad():
        data = AE.prepare_data(args, outputs, targets, meta, EI.CFG, flag="device", models=m)
    pred, gt = data.search("pred.", ""), data.search("targets.", "")
    pred, pred_leaves = MI.leaves(pred)

    def loss_step(acc_grad):
        out = SL.compute_smoothnet_loss(pred, gt, meta, m, args.img_res, acc_grad=acc_grad)
        sum(out[k] * WEIGHTS[k] for k in out).backward()
        for t in pred_leaves:
            t.grad = None

    def train_step():
        p = AE.make_output(args, *leaves, meta["query_names"], meta["intrinsics"], models=m, obj_idx=idx, max_len=max_len)
        d = AE.prepare_data(args, None, targets, meta, EI.CFG, pred=p, flag="train", models=m)
        losses = crit(args, d, targets, meta)
        sum(losses[k] * WEIGHTS[k] for k in losses if k in WEIGHTS).backward()

    def eager_train():
        train_step()
        for t in flat:
            t.grad = None

    def graphed_train():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                eager_train()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            train_step()
        return graph.replay

    count_syncs(lambda: None)            # torch's one-off notice about the sync debug mode itself names synchronisation too
    for run in range(a.runs):
        for route in ("restatement", "dropin", "dropin_acc_grad", "train", "train_graph"):
            if a.only and route != a.only:
                continue
            os.environ["MSDA_SMOOTH_LOSS_FUSED"] = "0" if route == "restatement" else "1"
            if route == "train":
                step = eager_train
            elif route == "train_graph":
                step = graphed_train()
            else:
                step = lambda: loss_step(route == "dropin_acc_grad")  # noqa: E731
            wall, gpu = measure(step, a.iters)
            line = json.dumps({"tool": "smooth_loss_time", "run": run, "route": route, "frames": B, "obj_len": int(max_len),
                               "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                               "host_syncs_per_step": count_syncs(step), "kernels_per_step": count_kernels(step),
                               "iters": a.iters, "device": torch.cuda.get_device_name(DEV)})
            print(line, flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    os.environ["MSDA_SMOOTH_LOSS_FUSED"] = "1"
    if not a.only:                       # the new kernels' own durations in a profiler trace of one drop-in step with acc_grad
        loss_step(True)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            loss_step(True)
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        dur = lambda e: float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))  # noqa: E731
        line = json.dumps({"tool": "smooth_loss_time", "mode": "trace", "route": "dropin_acc_grad", "frames": B, "obj_len": int(max_len),
                           "all_kernels_us": round(sum(dur(e) for e in evs), 1),
                           "kernel_us": {re.search(r"sm_\w+?_kernel", e.name).group(0): round(dur(e), 1) for e in evs
                                         if re.search(r"sm_\w+?_kernel", e.name)},
                           "device": torch.cuda.get_device_name(DEV)})
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    os.environ.pop("MSDA_SMOOTH_LOSS_FUSED", None)


if __name__ == "__main__":
    main()
