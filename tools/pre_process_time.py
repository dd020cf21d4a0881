#!/usr/bin/env python3
"""Time, host synchronisations, kernels and peak memory of one arctic_pre_process step: B frames (B = 32 is
window 32), synthetic MANO of tests/golden/mano_inputs.py and synthetic objects padded to --obj-len rows (ARCTIC's meshes are
not available here; about 4000 is an assumption).

Routes, `--runs` times over in one session, alternating:
  `restatement`   MSDA_PRE_PROCESS_FUSED=0 with the reference's structure: nothing is built from disk, the object is posed
                  twice, the two hands are posed by calls of their own, the rigid fit goes through `.cpu()` and numpy's
                  batched SVD and the translation through a per-frame loop of `np.linalg.solve` on the host (as
                  common/transforms.py batch_solve_rigid_tf and common/camera.py estimate_translation_k do), and the distance
                  fields are torch brute force (pytorch3d's knn_points cannot run on ROCm, so the reference's own route cannot)
  `dropin`        arctic_pre_process(args, targets, meta_info, models=...)
  `device`        pre_process(..., obj_idx=, max_len=), eager
  `device_graph`  the same call captured once and replayed as one graph
Per row: wall ms per step and the device-event interval per step, host syncs per step (torch.cuda.set_sync_debug_mode("warn")),
kernels per step (torch.profiler), launches through the library per step (msda_launch_count), peak allocated bytes of a step
above what was allocated before it.  One JSON line per row, on stdout and appended to --out (default
profiles/pre_process_time.jsonl).

    python tools/pre_process_time.py [--iters N] [--batch 32] [--obj-len 4000] [--only ROUTE] [--out FILE] [--runs 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import arctic_eval_inputs as EI  # noqa: E402
import pre_process_inputs as PI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from smoother_time import count_kernels, count_syncs, measure  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd import pre_process as PP  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors  # noqa: E402

DEV = torch.device("cuda", 0)
ROUTES = ("restatement", "dropin", "device", "device_graph")


def reference_structure_step(targets, meta, m):
    """process_data's structure on the package's layers (see the module's head); returns the vertex clouds and fields."""
    K = meta["intrinsics"]
    obj = m["arti_head"]
    pose = lambda: obj.forward(targets["object.radian"].view(-1, 1), targets["object.rot"].view(-1, 3), None, meta["query_names"])  # noqa: E731
    out = pose()
    nk = out["kp3d"].shape[1] // 2
    kp_cano = out["kp3d"][:, nk:]
    A, Bm = targets["object.kp3d.full.b"].cpu().numpy(), kp_cano.cpu().numpy()           # host round trip 1
    cA, cB = A.mean(1, keepdims=True), Bm.mean(1, keepdims=True)
    U, _, Vt = np.linalg.svd(np.swapaxes(A - cA, 1, 2) @ (Bm - cB))
    R = np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)
    T = cB[:, 0, :, None] - R @ cA[:, 0, :, None]
    R0, T0 = torch.from_numpy(R).float().to(DEV), torch.from_numpy(T).float().to(DEV)
    hands = {}
    for s in ("r", "l"):
        p = targets["mano.pose." + s]
        h = m["mano_" + s](betas=targets["mano.beta." + s], hand_pose=p[:, 3:], global_orient=p[:, :3], transl=None)
        j0 = (torch.bmm(R0, targets["mano.j3d.full." + s].permute(0, 2, 1)) + T0).permute(0, 2, 1)
        hands[s] = (h.vertices + (j0 - h.joints).mean(dim=1)[:, None, :], j0)
    px = (0.5 * PP.IMG_RES * (targets["object.kp2d.norm.b"] + 1)).cpu().numpy().astype(np.float64)   # host round trip 2
    S, Kn = kp_cano.cpu().numpy().astype(np.float64), K.cpu().numpy().astype(np.float64)
    trans = np.zeros((S.shape[0], 3), dtype=np.float32)
    for i in range(S.shape[0]):                                                            # the per-frame loop
        F, O = np.tile([Kn[i, 0, 0], Kn[i, 1, 1]], S.shape[1]), np.tile([Kn[i, 0, 2], Kn[i, 1, 2]], S.shape[1])
        Q = np.stack([F * np.tile([1, 0], S.shape[1]), F * np.tile([0, 1], S.shape[1]), O - px[i].reshape(-1)], axis=1)
        c = (px[i].reshape(-1) - O) * np.repeat(S[i, :, 2], 2) - F * S[i, :, :2].reshape(-1)
        trans[i] = np.linalg.solve(Q.T @ Q, Q.T @ c)
    t = torch.from_numpy(trans).to(DEV)
    v_r, v_l = hands["r"][0] + t[:, None, :], hands["l"][0] + t[:, None, :]
    out = pose()                                                                           # the second, identical object forward
    v_o = out["v"] + t[:, None, :]
    return v_r, v_l, v_o, PP.distance_fields(v_r, v_l, v_o, out["v_len"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--obj-len", type=int, default=4000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pre_process_time.jsonl"))
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pre_process_time.py measures on the GPU"
    B, L = a.batch, a.obj_len
    lengths = [L - 37 * i for i in range(11)]                  # arctic_eval_inputs.BIG_LENGTHS at the default --obj-len
    m = dict(EI.mano_models(DEV), arti_head=ObjectTensors.from_arrays(SI.obj_arrays(lengths=lengths)).to(DEV))
    targets, meta = PI.case_inputs("partial", B=B, lengths=lengths, seed=31)
    targets = {k: v.to(DEV) for k, v in targets.items()}
    meta = dict(meta, intrinsics=meta["intrinsics"].to(DEV))
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    args = EI.args(DEV)
    count_syncs(lambda: None)            # torch's one-off notice about the sync debug mode itself names synchronisation too

    def device_step():
        return PP.pre_process(dict(targets), meta, models=m, obj_idx=idx, max_len=max_len)

    device_step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        device_step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kept = device_step()                                  # noqa: F841  (the graph's outputs stay alive)
    steps = {"restatement": lambda: reference_structure_step(targets, meta, m),
             "dropin": lambda: PP.arctic_pre_process(args, dict(targets), meta, models=m),
             "device": device_step, "device_graph": graph.replay}
    for run in range(a.runs):
        for route in ROUTES:
            if a.only and route != a.only:
                continue
            os.environ["MSDA_PRE_PROCESS_FUSED"] = "0" if route == "restatement" else "1"
            step = steps[route]
            iters = max(3, a.iters // 10) if route == "restatement" else a.iters
            wall, gpu = measure(step, iters)
            torch.cuda.synchronize()
            n0 = _native.launch_count()
            step()
            launches = _native.launch_count() - n0
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(DEV)
            torch.cuda.reset_peak_memory_stats(DEV)
            step()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(DEV) - base
            line = json.dumps({"tool": "pre_process_time", "run": run, "route": route, "batch": B, "obj_len": int(max_len),
                               "wall_ms_per_step": round(wall, 4), "gpu_event_ms_per_step": round(gpu, 4),
                               "host_syncs_per_step": count_syncs(step), "kernels_per_step": count_kernels(step),
                               "library_launches_per_step": int(launches), "peak_bytes_above_start": int(peak), "iters": iters,
                               "device": torch.cuda.get_device_name(DEV)})
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    os.environ.pop("MSDA_PRE_PROCESS_FUSED", None)


if __name__ == "__main__":
    main()
