#!/usr/bin/env python3
"""DINO criterion fixture, made by RUNNING THE REFERENCE'S SetCriterion (models/dino/dino.py:428-781) with the reference's
HungarianMatcher (models/dino/matcher.py:25-130), scipy, sigmoid_focal_loss (models/dino/utils.py), accuracy and the
distributed helpers (util/misc.py) unchanged on the seeded inputs of dino_criterion_inputs.py:

  dino_criterion.npz   per case: the seed, the loss dict's keys and values; for "small" the gradients of the weighted total
                       with respect to every matched set's heads (grad_<head> [sets, bs, Q, .]) and the denoising set's
                       (grad_dn_<head> [bs, pad, .])

As gen_cdn_prepare.py does, the definitions are taken out of their files with `ast` and executed unchanged.  They run on the
CPU: in this process only, Tensor.cuda is the identity and .to('cuda') goes to the CPU.  get_arctic_item / compute_small_loss
are stubbed to return {} (the MANO / ARCTIC terms are not part of this fixture).  The seed of each case is the first one
whose every cost block the reference hands to scipy has an assignment margin >= 1e-3 (as in gen_golden_r09.py), so that any
exact solver returns the reference's indices and ties cannot decide a case.

    UVHAND_REFERENCE=<the reference's checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dino_criterion.py
"""
import ast
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import dino_criterion_inputs as DI   # noqa: E402

MIN_MARGIN = 1e-3
BLOCKS = []


def _recording_lsap(c):
    BLOCKS.append(np.array(c, dtype=np.float64))
    return linear_sum_assignment(c)


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _cpu_only():
    """This process has no GPU: .cuda() is the identity and 'cuda' means the CPU."""
    real_to = torch.Tensor.to

    def to(self, *args, **kwargs):
        args = tuple("cpu" if a == "cuda" else a for a in args)
        if kwargs.get("device") == "cuda":
            kwargs["device"] = "cpu"
        return real_to(self, *args, **kwargs)

    torch.Tensor.to = to
    torch.Tensor.cuda = lambda self, *a, **k: self


def _reference(ref):
    import torch.distributed as dist
    ns = {"torch": torch, "nn": nn, "F": F, "dist": dist, "linear_sum_assignment": _recording_lsap,
          "get_arctic_item": lambda outputs, cfg, device: {}, "compute_small_loss": lambda *a, **k: {}}
    _extract(ref + "/util/misc.py", ["is_dist_avail_and_initialized", "get_world_size", "accuracy"], ns)
    _extract(ref + "/models/dino/utils.py", ["sigmoid_focal_loss"], ns)
    _extract(ref + "/models/dino/matcher.py", ["HungarianMatcher"], ns)
    _extract(ref + "/models/dino/dino.py", ["SetCriterion"], ns)
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


def _run_case(ns, case, base_seed):
    _, _, _, _, n_aux = DI.shape(case)
    weights = DI.weight_dict(n_aux)
    matcher = ns["HungarianMatcher"](cost_class=DI.COST_CLASS, cost_bbox=DI.COST_BBOX, cost_giou=DI.COST_GIOU,
                                     focal_alpha=DI.FOCAL_ALPHA)
    crit = ns["SetCriterion"](DI.K, matcher, weights, DI.FOCAL_ALPHA, DI.losses(case), None, None)
    crit.train(case != "eval")
    for seed in range(base_seed, base_seed + 200):
        outputs, targets, _ = DI.make(case, seed)
        outputs, targets = DI.to_device(outputs, targets, "cpu", requires_grad=True)
        del BLOCKS[:]
        d = crit(outputs, targets, DI.ARGS, {})
        margins = np.array([_margin(b) for b in BLOCKS if b.size], np.float64)
        if margins.size and margins.min() < MIN_MARGIN:
            continue
        keys = list(d.keys())
        store = {"seed": np.int64(seed), "keys": np.array(keys),
                 "values": np.array([float(d[k]) for k in keys], np.float64)}
        indices = crit.matcher(DI.sets_of(outputs)[0], targets)
        for name, which in (("index_query", 0), ("index_target", 1)):
            store[name] = np.concatenate([np.asarray(p[which], np.int64) for p in indices])
        store["index_sizes"] = np.array([len(p[0]) for p in indices], np.int64)
        if case == "small":
            DI.weighted_total(d, weights).backward()
            store.update({k: v.numpy() for k, v in DI.gradients(outputs).items()})
        return store
    raise RuntimeError("no seed with margins >= %g" % MIN_MARGIN)


def main():
    ref = os.environ.get("UVHAND_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref:
        raise SystemExit("set UVHAND_REFERENCE (or pass the path) to the reference's checkout")
    warnings.filterwarnings("ignore")        # torch.range and torch.tensor(tensor) in the reference's code
    _cpu_only()
    ns = _reference(ref)
    store = {}
    for n, case in enumerate(DI.CASES):
        got = _run_case(ns, case, 100 * (n + 1))
        store.update({case + "__" + k: v for k, v in got.items()})
        print("%-12s seed %d keys %d" % (case, got["seed"], len(got["keys"])))
    path = os.path.join(HERE, "dino_criterion.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
