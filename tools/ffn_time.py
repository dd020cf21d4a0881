#!/usr/bin/env python3
"""Time, host synchronisations, kernels and memory of the layers' FFN, linear2(dropout(relu(linear1(x)))), forward + backward
under torch.autocast("cuda", dtype=torch.bfloat16), at the two shapes of a window-32 step: the encoder's
(M = 33 440 rows) and the decoder's (M = 9600), C = 256, F = 1024, p = 0.1, fp32 x, training mode.

Routes: `amp_composition` (knob off: bracket_linear -> F.relu -> nn.Dropout -> bracket_linear, what autocast gets by default)
and `amp_bf16_node` (MSDA_FFN_BF16=1: one node on the bf16 MFMA, csrc/msda_ffn_bf16.hip), three runs of each, interleaved, in
one process.  Per run: wall ms per step (host clock around the steps, ending in a device synchronise), GPU ms from device
events, host syncs per step (torch.cuda.set_sync_debug_mode("warn")), kernels per step (torch.profiler) and the step's peak
memory above what was allocated before it; then one `summary` row per route and shape with the median of the three runs.  One
JSON line each, on stdout and appended to --out (default profiles/ffn_time.jsonl).

    python tools/ffn_time.py [--iters N] [--only ROUTE] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from detr_time import DEV, count_kernels, count_syncs, measure, peak_mib  # noqa: E402
from uvhand_amd.functions.linear_func import fused_ffn  # noqa: E402

C, FFN, P = 256, 1024, 0.1
SHAPES = (("encoder", 33440), ("decoder", 9600))
ROUTES = ("amp_composition", "amp_bf16_node")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffn_time.jsonl"))
    args = ap.parse_args()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for shape, M in SHAPES:
        torch.manual_seed(0)
        l1, drop, l2 = torch.nn.Linear(C, FFN).to(DEV), torch.nn.Dropout(P), torch.nn.Linear(FFN, C).to(DEV)
        params = list(l1.parameters()) + list(l2.parameters())
        x = torch.randn(M, C, device=DEV, requires_grad=True)
        go = torch.randn(M, C, device=DEV).to(torch.bfloat16)

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = fused_ffn(x, l1, F.relu, drop, l2)
            torch.autograd.grad(y, [x] + params, go)

        gpu_ms = {r: [] for r in ROUTES}
        last = {}
        for run in range(3):                                          # the two routes interleaved, run by run
            for route in ROUTES:
                if args.only and route != args.only:
                    continue
                os.environ["MSDA_FFN_BF16"] = "1" if route == "amp_bf16_node" else "0"
                wall, gpu = measure(step, args.iters)
                gpu_ms[route].append(round(gpu, 4))
                last[route] = {"tool": "ffn_time", "shape": shape, "route": route, "rows": M, "C": C, "F": FFN, "p": P,
                               "autocast": "bfloat16", "iters": args.iters, "device": torch.cuda.get_device_name(DEV),
                               "host_syncs_per_step": count_syncs(step), "kernels_per_step": count_kernels(step),
                               "peak_mib_per_step": round(peak_mib(step), 1)}
                emit(dict(last[route], run=run, wall_ms_per_step=round(wall, 4), gpu_event_ms_per_step=round(gpu, 4)))
        for route in ROUTES:
            if gpu_ms[route]:
                emit(dict(last[route], run="summary", gpu_event_ms_median=statistics.median(gpu_ms[route]),
                          gpu_event_ms_runs=gpu_ms[route]))
    os.environ.pop("MSDA_FFN_BF16", None)


if __name__ == "__main__":
    main()
