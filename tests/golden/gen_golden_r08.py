#!/usr/bin/env python3
"""Matcher fixtures, made by RUNNING THE REFERENCE'S ArcticMatcher and AssemblyMatcher of models/matcher.py (needs the
reference tree and scipy):

  matcher_arctic.npz    the four ARCTIC cases of matcher_inputs.py (all valid; interleaved invalid frames, the chunk-pairing
                        quirk, with valid frames without labels; no target keypoints; no valid label -> 0)
  matcher_assembly.npz  the AssemblyHands case
  matcher_lsap.npz      scipy's linear_sum_assignment of the seeded random fp32 matrices (matcher_inputs.lsap_shapes) and
                        the optimum totals of the integer-valued tie matrices

As gen_golden_r06/r07.py do, the two class definitions are taken out of the file with `ast` and executed unchanged
(importing the module needs torchvision through util.box_ops).  Only the indices are stored, as per-frame lengths and the
concatenated query / target indices, with the seed that regenerates the inputs.  The seed is the first one whose every
frame has an assignment margin >= 1e-3: the optimum with any one matched pair forbidden, minus the optimum (fp64, from
the cost blocks the reference hands to scipy); the margins are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_r08.py
"""
import ast
import os
import sys

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")
REF_MATCHER = REF + "/models/matcher.py"

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import matcher_inputs as MI   # noqa: E402

MIN_MARGIN = 1e-3
BLOCKS = []                   # the cost blocks the reference passes to scipy, in call order


def _recording_lsap(c):
    BLOCKS.append(np.array(c, dtype=np.float64))
    return linear_sum_assignment(c)


def _reference_classes():
    tree = ast.parse(open(REF_MATCHER).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("ArcticMatcher", "AssemblyMatcher")]
    ns = {"torch": torch, "nn": nn, "linear_sum_assignment": _recording_lsap}
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF_MATCHER, "exec"), ns)
    return ns["ArcticMatcher"], ns["AssemblyMatcher"]


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
        except ValueError:                  # no assignment without that pair: it is forced
            pass
    return worst


def _run(make, matcher, base_seed):
    for seed in range(base_seed, base_seed + 200):
        outputs, targets = make(seed)
        del BLOCKS[:]
        result = matcher(outputs, targets)
        margins = np.array([_margin(b) for b in BLOCKS if b.size], np.float64)
        if margins.size == 0 or margins.min() >= MIN_MARGIN:
            return seed, result, margins
    raise RuntimeError("no seed with margins >= %g" % MIN_MARGIN)


def main():
    Arctic, Assembly = _reference_classes()
    arctic = Arctic(cost_class=MI.COST_CLASS, cost_keypoint=MI.COST_KEYPOINT)
    store = {}
    for n, case in enumerate(MI.ARCTIC_CASES):
        seed, result, margins = _run(lambda s: MI.arctic_case(case, s), arctic, 100 * (n + 1))
        lens, i, j = MI.flatten_indices(result)
        store.update({case + "_seed": np.int64(seed), case + "_lens": lens, case + "_i": i, case + "_j": j,
                      case + "_margins": margins})
        print("arctic %-13s seed %d frames %d min margin %s" % (case, seed, len(lens),
                                                                 "%.4g" % margins.min() if margins.size else "-"))
    np.savez_compressed(os.path.join(HERE, "matcher_arctic.npz"), **store)

    assembly = Assembly(cost_class=MI.COST_CLASS, cost_keypoint=MI.COST_KEYPOINT)
    seed, result, margins = _run(MI.assembly_case, assembly, 900)
    lens, i, j = MI.flatten_indices(result)
    np.savez_compressed(os.path.join(HERE, "matcher_assembly.npz"), seed=np.int64(seed), lens=lens, i=i, j=j, margins=margins)
    print("assembly seed %d frames %d min margin %.4g" % (seed, len(lens), margins.min()))

    store = {}
    for Q, T in MI.lsap_shapes():
        cost = MI.lsap_matrix(Q, T)
        rows = np.stack([linear_sum_assignment(c)[0] for c in cost])
        cols = np.stack([linear_sum_assignment(c)[1] for c in cost])
        store["rows_%d_%d" % (Q, T)], store["cols_%d_%d" % (Q, T)] = rows, cols
    for Q, T in MI.TIE_SHAPES:
        cost = MI.tie_matrix(Q, T).astype(np.float64)
        store["tie_opt_%d_%d" % (Q, T)] = np.array([c[linear_sum_assignment(c)].sum() for c in cost])
    np.savez_compressed(os.path.join(HERE, "matcher_lsap.npz"), **store)
    print("lsap: %d shapes, %d tie shapes" % (len(MI.lsap_shapes()), len(MI.TIE_SHAPES)))


if __name__ == "__main__":
    main()
