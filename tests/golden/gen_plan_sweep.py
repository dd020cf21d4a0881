#!/usr/bin/env python3
"""tests/golden/plan_sweep.npz: the launch plan and workspace sizes of the built libmsda_hip.so over the sweep of
plan_sweep_inputs.py (its record() names the arrays).  CPU only; build the library first.

Regenerate only when a plan is MEANT to change — a threshold moved, a kernel added — and say so in the commit: the
fixture exists so that a change that means to keep every decision can prove it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_plan_sweep.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import plan_sweep_inputs as PS   # noqa: E402

if __name__ == "__main__":
    from uvhand_amd import _native
    out = PS.record(_native.load())
    path = os.path.join(HERE, "plan_sweep.npz")
    np.savez_compressed(path, **out)
    print("%d geometries x %d calls, %d distinct plans; wrote plan_sweep.npz: %d bytes"
          % (out["plan"].shape[0], out["plan"].shape[1], len(out["plans"]), os.path.getsize(path)))
