"""The geometry sweep behind tests/golden/plan_sweep.npz: what the D = 32 launch plan decides (msda_describe_plan) and
the workspace sizes that follow from it (msda_forward_workspace_bytes, msda_backward_workspace_bytes), over every
combination of the things the plan looks at.  Pure host logic of libmsda_hip.so: no GPU, no tensors.

The plan sees a pyramid only through S and L, so a level set here is its (S, L).  gen_plan_sweep.py records the answers;
tests/test_plan_sweep.py holds the library to them exactly."""
import ctypes

import numpy as np

M, D = 8, 32
FLAG_DETERMINISTIC, FLAG_PROLOGUE, FLAG_FORWARD_TABLE, FLAG_EXACT_NONFINITE = 1, 2, 4, 8

_C2 = [(48, 48), (24, 24), (12, 12), (6, 6)]
_C4 = [(28, 28), (14, 14), (7, 7), (4, 4)]
LEVEL_SETS = {
    "cfg2": _C2,
    "cfg4": _C4,
    "small4": [(12, 12), (6, 6), (3, 3), (2, 2)],
    "three": [(40, 40), (20, 20), (10, 10)],
    "one8x8": [(8, 8)],
}
BATCHES = (1, 2, 8, 32)
QUERIES = (1, 100, 300, 900, "S")          # "S": the encoder's Lq = S
POINTS = (1, 4, 8)

# the geometries of the GPU tests that assert on the plan: (N, shapes, M, Lq, P)
_S2 = [(8, 8), (4, 4)]
_S5 = [(8, 8), (4, 4), (2, 2), (2, 2), (1, 1)]
NAMED = [
    # test_parity_gpu.STRADDLE
    (1, _S2, 8, 4095, 4), (1, _S2, 8, 4097, 4), (1, _S2, 8, 2048, 4), (1, _S2, 8, 2049, 4), (1, _S5, 8, 8192, 4),
    (1, _S5, 8, 8193, 4), (1, _S2, 8, 384, 4), (1, _S2, 8, 385, 4), (1, _S2, 1, 16384, 4), (1, _S2, 1, 16385, 4),
    (2, _C2, 8, 3060, 4), (2, _C2, 8, 3300, 4),
    # test_dense_levels_gpu.DENSE
    (4, [(20, 20), (8, 8), (4, 8), (4, 4)], 8, 1100, 4), (4, [(20, 20), (5, 13), (3, 11), (1, 17)], 8, 1100, 4),
    (8, [(18, 18), (7, 7), (1, 1)], 8, 513, 4), (6, [(16, 16), (6, 6), (2, 3)], 8, 1023, 4), (8, [(16, 16), (4, 4)], 8, 520, 8),
    (8, [(14, 14), (7, 7), (4, 4), (2, 2), (1, 1)], 8, 1100, 2), (16, [(14, 14), (7, 7), (2, 16), (4, 4)], 8, 300, 4),
    (32, [(4, 8), (4, 4)], 8, 256, 4), (16, [(12, 12), (5, 6), (16, 1)], 8, 301, 3), (24, [(10, 10), (4, 4)], 5, 333, 4),
    # test_range_masks_gpu.BIG / test_lds_prologue_gpu.BIG
    (2, _C2, 8, 3060, 4), (32, _C4, 8, 300, 4), (32, _C4, 8, 1045, 4), (4, [(40, 40), (20, 20), (10, 10)], 8, 2100, 4),
]


def geometries():
    """[(N, S, M, L, Lq, P)], without repeats, in a fixed order."""
    out = []
    for shapes in LEVEL_SETS.values():
        S, L = sum(h * w for h, w in shapes), len(shapes)
        out += [(N, S, M, L, S if Lq == "S" else Lq, P) for N in BATCHES for Lq in QUERIES for P in POINTS]
    out += [(N, sum(h * w for h, w in shapes), m, len(shapes), Lq, P) for N, shapes, m, Lq, P in NAMED]
    return list(dict.fromkeys(out))


def plan_calls():
    """[(row_bytes, grad_value_bytes, flags, has_workspace)] of msda_describe_plan: fp32 rows; bf16 rows with a bf16 or an fp32
    grad_value — with the fused prologue fp32 only, the one kernel there is."""
    out = []
    for prologue in (0, FLAG_PROLOGUE):
        storage = ((4, 4), (2, 4)) if prologue else ((4, 4), (2, 2), (2, 4))
        out += [(rb, gb, prologue | det | exact, ws) for rb, gb in storage for det in (0, FLAG_DETERMINISTIC)
                for exact in (0, FLAG_EXACT_NONFINITE) for ws in (1, 0)]
    return out


WORKSPACE_FLAGS = tuple(range(16))         # every combination of the four flags: a superset of what the Python binding passes


def record(lib):
    """The library's answers for the whole sweep:
      geometry  int32 [G, 6]                  (N, S, M, L, Lq, P), D = 32
      calls     int32 [C, 4]                  (row_bytes, grad_value_bytes, flags, has_workspace)
      plans     str [K]                       the distinct msda_describe_plan strings
      plan      int32 [G, C]                  index into plans
      fwd_ws    uint64 [G, 16], bwd_ws same   msda_{forward,backward}_workspace_bytes for flags 0 .. 15"""
    geo, calls = geometries(), plan_calls()
    buf = ctypes.create_string_buffer(512)
    texts, plan = {}, np.zeros((len(geo), len(calls)), np.int32)
    fwd_ws, bwd_ws = (np.zeros((len(geo), len(WORKSPACE_FLAGS)), np.uint64) for _ in range(2))
    for g, (N, S, m, L, Lq, P) in enumerate(geo):
        for c, (rb, gb, flags, ws) in enumerate(calls):
            lib.msda_describe_plan(rb, gb, N, S, m, D, L, Lq, P, flags, ws, buf, len(buf))
            plan[g, c] = texts.setdefault(buf.value.decode(), len(texts))
        for f in WORKSPACE_FLAGS:
            fwd_ws[g, f] = lib.msda_forward_workspace_bytes(N, S, m, D, L, Lq, P, f)
            bwd_ws[g, f] = lib.msda_backward_workspace_bytes(N, S, m, D, L, Lq, P, f)
    return {"geometry": np.array(geo, np.int32), "calls": np.array(calls, np.int32), "plans": np.array(list(texts)),
            "plan": plan, "fwd_ws": fwd_ws, "bwd_ws": bwd_ws}
