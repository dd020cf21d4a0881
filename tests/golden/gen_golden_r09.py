#!/usr/bin/env python3
"""Criterion fixtures, made by RUNNING THE REFERENCE'S SetArcticCriterion (models/actic_detr.py) and SetAssemblyCriterion
(models/assembly_detr.py) with the reference's ArcticMatcher / AssemblyMatcher (models/matcher.py), scipy,
sigmoid_focal_loss (models/segmentation.py) and accuracy (util/misc.py) on the seeded inputs of criterion_inputs.py:

  criterion_arctic.npz    per ARCTIC case: the seed, the loss dict's keys and values; gradients of the weighted total for
                          "small" (every set's pred_logits / pred_hand_key / pred_obj_key)
  criterion_assembly.npz  the same for AssemblyHands; for "enc" and "not_hand" the reference's error (type and message)

As gen_golden_r08.py does, the definitions are taken out of their files with `ast` and executed unchanged, except that the
criteria's 'cuda' device strings and .cuda() calls are rewritten to the CPU (the fixtures are made on the CPU; importing the
modules needs torchvision and the MANO tools).  get_arctic_item / compute_small_loss are stubbed to return {} (the MANO /
ARCTIC terms are not part of these fixtures), is_dist_avail_and_initialized to False and get_world_size to 1.  The seed of
each case is the first one whose every cost block the reference hands to scipy has an assignment margin >= 1e-3 (as in
gen_golden_r08.py), so that any exact solver returns the reference's indices.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r09.py
"""
import ast
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import criterion_inputs as CI   # noqa: E402

MIN_MARGIN = 1e-3
BLOCKS = []


def _recording_lsap(c):
    BLOCKS.append(np.array(c, dtype=np.float64))
    return linear_sum_assignment(c)


def _extract(path, names, ns, to_cpu=False):
    src = open(path).read()
    if to_cpu:
        src = src.replace(".to('cuda')", ".to('cpu')").replace(".cuda()", ".cpu()")
    tree = ast.parse(src)
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _reference():
    ns = {"torch": torch, "nn": nn, "F": F, "copy": copy, "linear_sum_assignment": _recording_lsap,
          "is_dist_avail_and_initialized": lambda: False, "get_world_size": lambda: 1,
          "get_arctic_item": lambda outputs, cfg, device: {}, "compute_small_loss": lambda *a, **k: {}}
    _extract(REF + "/models/matcher.py", ["ArcticMatcher", "AssemblyMatcher"], ns)
    _extract(REF + "/models/segmentation.py", ["sigmoid_focal_loss"], ns)
    _extract(REF + "/util/misc.py", ["accuracy"], ns)
    _extract(REF + "/models/actic_detr.py", ["SetArcticCriterion"], ns, to_cpu=True)
    _extract(REF + "/models/assembly_detr.py", ["SetAssemblyCriterion"], ns, to_cpu=True)
    return ns


def _margin(block):
    rows, cols = linear_sum_assignment(block)
    opt = block[rows, cols].sum()
    worst = np.inf
    for r, c in zip(rows, cols):
        b = block.copy()
        b[r, c] = np.inf
        try:
            rr, cc = linear_sum_assignment(b)
            worst = min(worst, b[rr, cc].sum() - opt)
        except ValueError:
            pass
    return worst


def _leaves(outputs):
    out = {}
    for k, v in outputs.items():
        if k == "aux_outputs":
            out[k] = [{kk: vv.clone().requires_grad_(True) for kk, vv in a.items()} for a in v]
        elif isinstance(v, dict):
            out[k] = {kk: vv.clone().requires_grad_(True) for kk, vv in v.items()}
        else:
            out[k] = v.clone().requires_grad_(True)
    return out


def _run_case(kind, case, crit, base_seed, weights):
    for seed in range(base_seed, base_seed + 200):
        make = CI.arctic_case if kind == "arctic" else CI.assembly_case
        outputs, targets, _ = make(case, seed)
        outputs = _leaves(outputs)
        del BLOCKS[:]
        err = None
        try:
            d = crit(outputs, targets, CI.ARCTIC_ARGS, {}) if kind == "arctic" else crit(outputs, targets)
        except (IndexError, RuntimeError) as e:
            d, err = None, e
        margins = np.array([_margin(b) for b in BLOCKS if b.size], np.float64)
        if err is None and margins.size and margins.min() < MIN_MARGIN:
            continue
        store = {"seed": np.int64(seed)}
        if err is not None:
            store.update(error_type=np.array(type(err).__name__), error=np.array(str(err)))
            return store
        keys = list(d.keys())
        store["keys"] = np.array(keys)
        store["values"] = np.array([float(d[k]) for k in keys], np.float64)
        if kind == "assembly":   # frames whose matched targets are not in target order: joint_valid row r != J[r]
            final = CI.sets_of(outputs)[0]
            idx = crit.matcher(final, targets)
            store["nonidentity_frames"] = np.int64(sum(bool((j != torch.arange(len(j))).any()) for _, j in idx))
        if case == "small":
            total = CI.weighted_total(d, weights)
            total.backward()
            for name in CI.heads(kind):
                store["grad_" + name] = np.stack([s[name].grad.numpy() if s[name].grad is not None
                                                  else np.zeros(tuple(s[name].shape), np.float32)
                                                  for s in CI.sets_of(outputs)])
        return store
    raise RuntimeError("no seed with margins >= %g" % MIN_MARGIN)


def main():
    ns = _reference()
    store = {}
    for n, case in enumerate(CI.ARCTIC_CASES):
        matcher = ns["ArcticMatcher"](cost_class=CI.COST_CLASS, cost_keypoint=CI.COST_KEYPOINT)
        w = CI.weight_dict(CI.ARCTIC_WEIGHTS, 5)
        crit = ns["SetArcticCriterion"](CI.ARCTIC_K, matcher, w, CI.arctic_losses(case), focal_alpha=CI.FOCAL_ALPHA)
        got = _run_case("arctic", case, crit, 100 * (n + 1), w)
        store.update({case + "__" + k: v for k, v in got.items()})
        print("arctic   %-15s seed %d keys %d" % (case, got["seed"], len(got.get("keys", []))))
    np.savez_compressed(os.path.join(HERE, "criterion_arctic.npz"), **store)

    store = {}
    for n, case in enumerate(CI.ASSEMBLY_CASES):
        matcher = ns["AssemblyMatcher"](cost_class=CI.COST_CLASS, cost_keypoint=CI.COST_KEYPOINT)
        w = CI.weight_dict(CI.ASSEMBLY_WEIGHTS, 5, extra=("_enc",))
        crit = ns["SetAssemblyCriterion"](CI.ASSEMBLY_K, matcher, w, ["labels", "cardinality", "hand_keypoint"],
                                          focal_alpha=CI.FOCAL_ALPHA, cfg=CI.ASSEMBLY_CFG)
        got = _run_case("assembly", case, crit, 1000 + 100 * n, w)
        store.update({case + "__" + k: v for k, v in got.items()})
        print("assembly %-15s seed %d %s" % (case, got["seed"], got.get("error", "keys %d" % len(got.get("keys", [])))))
    np.savez_compressed(os.path.join(HERE, "criterion_assembly.npz"), **store)


if __name__ == "__main__":
    main()
