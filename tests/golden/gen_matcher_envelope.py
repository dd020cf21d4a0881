#!/usr/bin/env python3
"""tests/golden/matcher_envelope.npz: scipy's answers for the cases of matcher_envelope_inputs.py (CPU, needs scipy).

Per match case `name` (inputs regenerated from the case table's seed, so none are stored):
  name__qi, name__ti   int16 [sets, valid frames, 16]: scipy's linear_sum_assignment of every slot's cost block, -1 padding.
                       The block is the package's fp64 restatement of the reference's cost (matcher._class_cost + cdist,
                       matcher_envelope_inputs.cost_blocks) rounded to fp32, as the reference hands scipy an fp32 matrix
  name__opt            fp64 [sets, valid frames]: that assignment's total on the fp64 block
  name__cmax           fp64 [sets, valid frames]: max |C| of the block (0 for an empty one)
  name__gap            fp64 [sets, valid frames]: the uniqueness gap (see matcher_envelope_inputs; inf where no other
                       assignment exists)
  name__excluded       the share of the case's frames whose gap is under 2 min(Q, T) EPS
and per LSAP matrix kind and shape lsap_<kind>_<Q>_<T>__rows / __cols int16 [B, min(Q, T)].  The generator asserts the
exclusion cap (MAX_EXCLUDED per case, none for TIE_CASES).  scipy's, numpy's and torch's versions are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_matcher_envelope.py
"""
import os
import sys

import numpy as np
import scipy
import torch
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import matcher_envelope_inputs as EI   # noqa: E402


def solve_block(c64, classes):
    """(rows, cols, optimum, max|C|, gap) of one [Q, T] fp64 block."""
    Q, T = c64.shape
    if T == 0:
        e = np.zeros(0, np.int64)
        return e, e, 0.0, 0.0, np.inf
    c32 = c64.astype(np.float32).astype(np.float64)
    rows, cols = linear_sum_assignment(c32)
    opt = float(c64[rows, cols].sum())
    cmax = float(np.abs(c64).max())
    classes = np.asarray(classes)
    gap = np.inf
    for r, c in zip(rows, cols):
        b = c32.copy()
        b[r, classes == classes[c]] = np.inf
        try:
            rr, cc = linear_sum_assignment(b)
        except ValueError:                  # no other assignment (Q = 1 = T, ...)
            continue
        gap = min(gap, (float(c64[rr, cc].sum()) - opt) / cmax)
    return rows, cols, opt, cmax, gap


def match_answers(name):
    from uvhand_amd import matcher as M
    case = EI.MATCH_CASES[name]
    sets, targets = EI.convert(*EI.match_case(name), dtype=torch.float64)
    valid = EI.valid_frames(targets)
    sizes = EI.frame_sizes(targets)
    n, W = len(valid), max(sizes)
    qi = np.full((len(sets), n, W), -1, np.int16)
    ti = np.full((len(sets), n, W), -1, np.int16)
    opt, cmax, gap = (np.zeros((len(sets), n)) for _ in range(3))
    under = 0
    for s, outputs in enumerate(sets):
        with torch.no_grad():
            blocks = EI.cost_blocks(M, outputs, targets)
        for k, f in enumerate(valid):
            r, c, opt[s, k], cmax[s, k], gap[s, k] = solve_block(blocks[k].numpy(), EI.column_classes(targets, f))
            qi[s, k, :len(r)], ti[s, k, :len(c)] = r, c
            under += gap[s, k] < EI.bound(case["Q"], sizes[f])
    excluded = under / float(len(sets) * n)
    assert excluded <= (0.0 if name in EI.TIE_CASES else EI.MAX_EXCLUDED), (name, excluded)
    return {"qi": qi, "ti": ti, "opt": opt, "cmax": cmax, "gap": gap, "excluded": np.float64(excluded)}


def lsap_answers(kind, Q, T):
    cost = EI.lsap_matrix(kind, Q, T)
    pairs = [linear_sum_assignment(c.astype(np.float64)) for c in cost]
    return {"rows": np.stack([r for r, _ in pairs]).astype(np.int16), "cols": np.stack([c for _, c in pairs]).astype(np.int16)}


def generate():
    store = {"scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__),
             "torch_version": np.array(torch.__version__)}
    for name in EI.MATCH_CASES:
        store.update({"%s__%s" % (name, k): v for k, v in match_answers(name).items()})
    for kind in EI.LSAP_KINDS:
        for Q, T in EI.lsap_shapes():
            store.update({"lsap_%s_%d_%d__%s" % (kind, Q, T, k): v for k, v in lsap_answers(kind, Q, T).items()})
    return store


if __name__ == "__main__":
    out = generate()
    np.savez_compressed(os.path.join(HERE, "matcher_envelope.npz"), **out)
    for name in EI.MATCH_CASES:
        g = out[name + "__gap"]
        print("%-18s frames %4d  excluded %.3f  min gap %.3g" % (name, g.size, out[name + "__excluded"], g.min()))
    print("wrote matcher_envelope.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "matcher_envelope.npz")))
