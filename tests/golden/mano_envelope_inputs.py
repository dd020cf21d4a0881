"""Seeded models, inputs and yardsticks of the MANO envelope tests (tests/test_mano_envelope*.py): torch only, nothing read from
the reference, shared by the CPU and the GPU file.  tests/golden/mano_inputs.py (one geometry, committed fixtures) is untouched.

``model_arrays(V, nb, E, tree, seed)`` gives the keyword arguments of ``MANO.from_arrays`` for any size inside the envelope of
csrc/msda_mano.hip (1 <= V <= 8192, 1 <= nb <= 16, 0 <= E <= 8) and any of four kinematic trees; ``pose_inputs`` draws a batch
whose *full* pose (``pose_mean`` added) lies in one of the angle classes of ``ANGLES``; ``upstream`` gives the weights of the
weighted-sum loss per mode of ``UPSTREAM``; ``groups16`` lays sixteen groups over four layers of one size.  ``run_reference``
runs ``mano_reference`` and autograd on the CPU in a given dtype; ``yardsticks`` runs it in fp64 and fp32 on the same bits and
gives, per tensor, the bound of the GPU tests:

    bound = max(4 x dev32, FLOOR x scale)      dev32 = max |fp32 restatement - fp64 restatement|, scale = max |fp64 value|

Everything is fp32-representable, so both yardsticks and the kernels read the same numbers.  The full pose is exact too: the
hand mean is a multiple of 2^-6 and the pose is moved to the nearest fp32 value p for which fp32(p - mean) + mean = p holds in
real arithmetic, so the angle a class asks for is the angle that the fp32 kernels and the fp64 yardstick both see (with a
non-zero mean a hand-joint component is then a multiple of the ulp of its ``hand_pose`` entry, 2^-30 to 2^-26; the global
orient has no mean and keeps every bit).  No component of the full pose equals -1e-8, where the original's
``|r + 1e-8|`` could vanish.

Tip ids, in this order as far as E reaches: V - 1, 0, 0 again (two tips on one vertex), a vertex of the last slice other than
V - 1 (the slice's first; for V <= 65 a middle vertex), then seeded ids.  So E = 1 holds V - 1 alone, E >= 2 vertex 0 too,
E >= 3 one id twice, E >= 4 the second id of the last slice.  For V = 1 every id is 0."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mano_inputs as MI  # noqa: E402

NJ, NPF = 16, 135
KHT, KVS, KPART = 8, 64, NJ * 12 + NPF + 16 + 3          # hands per tile, vertices per slice, floats per (hand, slice) partial
FLOOR = 16 * 2.0 ** -24
NAMES = ("vertices", "joints", "g_betas", "g_global_orient", "g_hand_pose", "g_transl")
INPUTS = ("betas", "global_orient", "hand_pose", "transl")
DEPTH ={"mano": (3, 3), "chain": (15, 15), "star": (1, 1), "bushy": (4, 8)}

MODELS = [(1, 1, 0, "mano"), (63, 16, 8, "chain"), (64, 10, 5, "star"), (65, 3, 1, "bushy"), (128, 16, 0, "chain"),
          (778, 10, 5, "mano"), (8192, 16, 8, "bushy")]
MODEL_OPTIONS = {(778, 10, 5, "mano"): dict(dense_regressor=True), (63, 16, 8, "chain"): dict(zero_mean=True),
                 (65, 3, 1, "bushy"): dict(zero_mean=True)}
ANGLES = ("zero", "tiny", "small", "mid", "pi", "wide", "axis", "mixed")
MIX = ("tiny", "zero", "small", "pi", "wide", "axis", "mid")         # hand b of a mixed batch is of class MIX[b % 7]
RANGES = {"tiny": (1e-7, 1e-5), "small": (1e-4, 1e-2), "mid": (0.05, 3.1), "pi": (math.pi - 1e-4, math.pi + 1e-4),
          "wide": (3.2, 9.5), "axis": (0.05, 3.1)}
BATCHES = (1, 7, 8, 9, 17)
UPSTREAM = ("both", "vertices", "joints", "tips", "one_group")
SMALL, LARGE = (65, 3, 1, "bushy"), (8192, 16, 8, "bushy")
BATCH_MODELS = (SMALL, (778, 10, 5, "mano"))
UPSTREAM_MODELS = ((64, 10, 5, "star"), (128, 16, 0, "chain"))
GROUP_MODELS = (SMALL, LARGE)
GROUP_B = [0, 0, 1, 8, 9, 0, 17, 3, 0, 8, 1, 2, 16, 5, 0, 0]
GROUP_TREES = ("chain", "star", "mano")                  # layers 1 to 3 of a sixteen-group call; layer 0 is the named model
GROUP_BCAST_BETAS = (3, 6, 11)
GROUP_TRANSL_ONE, GROUP_ORIENT_ONE, ONE_GROUP = 4, 7, 6
# every single-call case (model, angles, B, upstream) that a GPU test compares with fp64, once each
MODEL_CASES = [(m, a, 9, "both") for m in MODELS for a in ANGLES]
BATCH_CASES = [(m, "mixed", B, "both") for m in BATCH_MODELS for B in BATCHES]
UPSTREAM_CASES = [(m, "mixed", 9, u) for m in UPSTREAM_MODELS for u in UPSTREAM if u != "one_group"]
SINGLE_CASES = list(dict.fromkeys(MODEL_CASES + BATCH_CASES + UPSTREAM_CASES))


# ---- models -------------------------------------------------------------------------------------------------------------------
def depth_of(parents):
    d = [0] * len(parents)
    for j in range(1, len(parents)):
        d[j] = d[parents[j]] + 1
    return max(d)


def tree(name, seed):
    if name == "mano":
        return list(MI.PARENTS)
    if name == "chain":
        return [-1] + list(range(NJ - 1))
    if name == "star":
        return [-1] + [0] * (NJ - 1)
    g = torch.Generator().manual_seed(seed)
    while True:
        parents = [-1] + [int(torch.randint(max(0, j - 4), j, (1,), generator=g)) for j in range(1, NJ)]
        if DEPTH["bushy"][0] <= depth_of(parents) <= DEPTH["bushy"][1]:
            return parents


def tip_ids(V, E, seed):
    if V == 1:
        return [0] * E
    first = (V - 1) // KVS * KVS
    in_last = first if 0 < first < V - 1 else V // 2
    g = torch.Generator().manual_seed(seed)
    rest = torch.randint(0, V, (8,), generator=g).tolist()
    return ([V - 1, 0, 0, in_last] + rest)[:E]


def model_arrays(V, nb, E, tree_name, seed, dense_regressor=False, zero_mean=False):
    """The keyword arguments of uvhand_amd.mano.MANO.from_arrays, fp32, in smplx's layouts (posedirs [135, 3 V])."""
    g = torch.Generator().manual_seed(seed)
    f64 = dict(generator=g, dtype=torch.float64)
    parents = tree(tree_name, seed + 1)
    J = torch.zeros(NJ, 3, dtype=torch.float64)
    for j in range(1, NJ):
        J[j] = J[parents[j]] + torch.tensor([0.025, 0.0, 0.0], dtype=torch.float64) + 0.008 * torch.randn(3, **f64)
    owner = torch.randint(0, NJ, (V,), generator=g)
    v_template = J[owner] + torch.randn(V, 3, **f64) * torch.tensor([0.01, 0.006, 0.006], dtype=torch.float64)
    d2 = ((v_template[:, None, :] - J[None, :, :]) ** 2).sum(-1)
    lbs_weights = torch.softmax(-d2 / 2e-4, dim=1)
    if dense_regressor:
        J_regressor = torch.rand(NJ, V, **f64) + 0.1
        J_regressor = J_regressor / J_regressor.sum(1, keepdim=True)
    else:
        J_regressor = torch.zeros(NJ, V, dtype=torch.float64)
        k = min(12, V)
        for j in range(NJ):
            near = torch.argsort(d2[:, j])[:k]
            w = torch.rand(k, **f64) + 0.1
            J_regressor[j, near] = w / w.sum()
    shapedirs = 0.004 * torch.randn(V, 3, nb, **f64)
    posedirs = 0.003 * torch.randn(NPF, 3 * V, **f64)
    steps = torch.randint(1, 17, (45,), generator=g) * (2 * torch.randint(0, 2, (45,), generator=g) - 1)
    hand_mean = torch.zeros(45, dtype=torch.float64) if zero_mean else steps.double() / 64
    faces = torch.randint(0, V, (4, 3), generator=g)
    f = lambda t: t.float().contiguous()  # noqa: E731
    return dict(v_template=f(v_template), shapedirs=f(shapedirs), posedirs=f(posedirs), J_regressor=f(J_regressor),
                lbs_weights=f(lbs_weights), parents=torch.tensor(parents), pose_mean=f(torch.cat([torch.zeros(3), hand_mean])),
                faces=faces, extra_joints_idxs=torch.tensor(tip_ids(V, E, seed + 2), dtype=torch.long))


def check_model(arrays, V, nb, E, tree_name, dense_regressor=False, zero_mean=False):
    """Raises ValueError where a model does not hold what its name says."""
    def need(ok, what):
        if not ok:
            raise ValueError("mano envelope model %s: %s" % ((V, nb, E, tree_name), what))
    need(all(arrays[k].dtype == torch.float32 for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights",
                                                        "pose_mean")), "fp32 tensors")
    need(tuple(arrays["v_template"].shape) == (V, 3) and tuple(arrays["shapedirs"].shape) == (V, 3, nb)
         and tuple(arrays["posedirs"].shape) == (NPF, 3 * V) and tuple(arrays["J_regressor"].shape) == (NJ, V)
         and tuple(arrays["lbs_weights"].shape) == (V, NJ) and tuple(arrays["pose_mean"].shape) == (48,), "shapes")
    w, r = arrays["lbs_weights"].double(), arrays["J_regressor"].double()
    need(bool((w >= 0).all()) and float((w.sum(1) - 1).abs().max()) < 1e-6, "lbs_weights rows sum to 1")
    need(bool((r >= 0).all()) and float((r.sum(1) - 1).abs().max()) < 1e-6, "J_regressor rows are convex")
    nz = int((r > 0).sum(1).max())
    need(nz == V if dense_regressor else nz <= min(12, V), "J_regressor density")
    parents = arrays["parents"].tolist()
    need(len(parents) == NJ and parents[0] == -1 and all(0 <= parents[j] < j for j in range(1, NJ)), "parents")
    lo, hi = DEPTH[tree_name]
    need(lo <= depth_of(parents) <= hi, "tree depth")
    mean = arrays["pose_mean"]
    need(not bool(mean[:3].any()) and bool(mean[3:].any()) != zero_mean, "pose_mean")
    need(torch.equal(mean * 64, (mean * 64).round()), "pose_mean is a multiple of 2^-6")
    tips = arrays["extra_joints_idxs"].tolist()
    need(len(tips) == E and all(0 <= t < V for t in tips), "tip ids in range")
    if V == 1:
        need(all(t == 0 for t in tips), "V = 1 tips")
        return
    need(E < 1 or V - 1 in tips, "tip at V - 1")
    need(E < 2 or 0 in tips, "tip at vertex 0")
    need(E < 3 or len(set(tips)) < len(tips), "two tips on one vertex")
    first = (V - 1) // KVS * KVS
    need(E < 4 or V <= KVS + 1 or any(first <= t < V - 1 for t in tips), "a second tip in the last slice")


_MODELS = {}


def model(key, layer=0):
    """The arrays of a model of MODELS (cached); ``layer`` 1 to 3: the other layers of its sixteen-group call."""
    if (key, layer) not in _MODELS:
        V, nb, E, t = key
        seed = 7000 + 16 * MODELS.index(key) + 4 * layer
        if layer == 0:
            _MODELS[key, layer] = model_arrays(V, nb, E, t, seed, **MODEL_OPTIONS.get(key, {}))
        else:
            _MODELS[key, layer] = model_arrays(V, nb, E, GROUP_TREES[layer - 1], seed, zero_mean=layer == 2)
    return _MODELS[key, layer]


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _class_pose(cls, g, n):
    """[n, 16, 3] fp64 axis-angles of one class."""
    f64 = dict(generator=g, dtype=torch.float64)
    if cls == "zero":
        return torch.zeros(n, NJ, 3, dtype=torch.float64)
    lo, hi = RANGES[cls]
    u = torch.rand(n, NJ, 1, **f64)
    if cls in ("tiny", "small"):                                     # log-uniform; the move to an exact pose stays under hi
        angle = torch.exp(math.log(1.01 * lo) + (math.log(0.99 * hi) - math.log(1.01 * lo)) * u)
    else:
        angle = lo + (hi - lo) * u
    if cls == "wide":
        angle[:, 0], angle[:, 5] = 9.0, 7.5                          # past 2 pi
    if cls == "axis":
        which = torch.randint(0, 3, (n, NJ), generator=g)
        sign = 2.0 * torch.randint(0, 2, (n, NJ, 1), generator=g) - 1.0
        return torch.nn.functional.one_hot(which, 3).double() * angle * sign
    d = torch.randn(n, NJ, 3, **f64)
    return d / d.norm(dim=-1, keepdim=True) * angle


def full_pose(angles, B, seed):
    g = torch.Generator().manual_seed(seed)
    if B == 0:
        return torch.zeros(0, 48, dtype=torch.float64)
    if angles != "mixed":
        return _class_pose(angles, g, B).view(B, 48)
    return torch.cat([_class_pose(MIX[b % len(MIX)], g, 1) for b in range(B)]).view(B, 48)


def pose_inputs(arrays, angles, B, seed):
    """fp32 ``dict(betas, global_orient, hand_pose, transl)`` whose full pose is of class ``angles``, and that full pose."""
    mean = arrays["pose_mean"].double()
    full = full_pose(angles, B, seed).float().double()
    for _ in range(8):
        pose = (full - mean).float()
        exact = pose.double() + mean
        if torch.equal(exact.float().double(), exact):
            break
        full = exact.float().double()
    else:
        raise ValueError("no fp32 pose whose sum with the mean is exact")
    full = exact.float()
    if bool((full == torch.tensor(-1e-8, dtype=torch.float32)).any()):
        raise ValueError("a pose component of -1e-8")
    g = torch.Generator().manual_seed(seed + 1)
    nb = arrays["shapedirs"].shape[-1]
    betas = (1.5 * torch.randn(B, nb, generator=g, dtype=torch.float64)).float()
    transl = (0.1 * torch.randn(B, 3, generator=g, dtype=torch.float64)).float()
    return dict(betas=betas, global_orient=pose[:, :3].contiguous(), hand_pose=pose[:, 3:].contiguous(), transl=transl), full


def joint_angles(full):
    """[B, 16] angles of an fp32 full pose, in fp64."""
    return full.double().view(-1, NJ, 3).norm(dim=-1)


def upstream(arrays, B, mode, seed):
    """fp32 weights (w_vertices or None, w_joints or None) of the weighted-sum loss."""
    V, E = arrays["v_template"].shape[0], arrays["extra_joints_idxs"].numel()
    g = torch.Generator().manual_seed(seed)
    wv = torch.randn(B, V, 3, generator=g, dtype=torch.float64).float()
    wj = torch.randn(B, NJ + E, 3, generator=g, dtype=torch.float64).float()
    if mode == "tips":
        wj[:, :NJ] = 0
    return {"both": (wv, wj), "vertices": (wv, None), "joints": (None, wj), "tips": (None, wj), "none": (None, None)}[mode]


def tips_as_vertex_weights(arrays, wj):
    """The vertex weights that a ``tips`` upstream amounts to: its rows scattered (added, in tip order) into zeros."""
    wv = torch.zeros(wj.shape[0], arrays["v_template"].shape[0], 3, dtype=wj.dtype)
    for e, v in enumerate(arrays["extra_joints_idxs"].tolist()):
        wv[:, v] += wj[:, NJ + e]
    return wv


# ---- yardsticks ---------------------------------------------------------------------------------------------------------------
def run_reference(layer_arrays, inputs, weights, dtype):
    """``mano_reference`` (through ``MANO(...).to(dtype)`` on the CPU) and autograd: a dict of NAMES; a gradient that the loss does
    not reach is zero, ``g_transl`` without transl is None."""
    from uvhand_amd.mano import MANO
    layer = MANO.from_arrays(**layer_arrays).to(dtype)
    leaves = {k: None if inputs.get(k) is None else inputs[k].to(dtype).clone().requires_grad_(True) for k in INPUTS}
    out = layer(**leaves)
    res = dict(vertices=out.vertices.detach(), joints=out.joints.detach())
    terms = [(o * w.to(dtype)).sum() for o, w in zip((out.vertices, out.joints), weights) if w is not None]
    live = [k for k in INPUTS if leaves[k] is not None]
    grads = torch.autograd.grad(sum(terms), [leaves[k] for k in live], allow_unused=True) if terms else [None] * len(live)
    for k in INPUTS:
        res["g_" + k] = None
    for k, gr in zip(live, grads):
        res["g_" + k] = torch.zeros_like(leaves[k]).detach() if gr is None else gr
    return res


def yardsticks(layer_arrays, inputs, weights):
    """(fp64 results, fp32 results, {name: (dev32, scale, bound)}) on the same bits."""
    f64 = run_reference(layer_arrays, inputs, weights, torch.float64)
    f32 = run_reference(layer_arrays, inputs, weights, torch.float32)
    table = {}
    for n in NAMES:
        if f64[n] is None or f64[n].numel() == 0:
            continue
        dev32 = float((f32[n].double() - f64[n]).abs().max())
        scale = float(f64[n].abs().max())
        table[n] = (dev32, scale, max(4 * dev32, FLOOR * scale))
    return f64, f32, table


_CASES = {}


def case(key, angles, B, mode="both"):
    """A single-call case, built once: dict(arrays, inputs, full, weights, f64, f32, bounds)."""
    k = (key, angles, B, mode)
    if k not in _CASES:
        arrays = model(key)
        seed = 9000 + 1000 * MODELS.index(key) + 32 * ANGLES.index(angles) + B
        inputs, full = pose_inputs(arrays, angles, B, seed)
        weights = upstream(arrays, B, mode, seed + 500)
        f64, f32, bounds = yardsticks(arrays, inputs, weights)
        _CASES[k] = dict(arrays=arrays, inputs=inputs, full=full, weights=weights, f64=f64, f32=f32, bounds=bounds)
    return _CASES[k]


def groups16(key):
    """Sixteen groups over four layers of the size of ``key``: dict(layers, groups); a group is dict(layer, B, inputs, weights).
    Groups of GROUP_BCAST_BETAS have betas of batch 1, odd groups have no transl, group GROUP_TRANSL_ONE has transl of batch 1
    and group GROUP_ORIENT_ONE a global orient of batch 1.  Empty groups have batch 0 in every input."""
    k = (key, "groups16")
    if k not in _CASES:
        layers = [model(key, l) for l in range(4)]
        groups = []
        for i, B in enumerate(GROUP_B):
            l = (i + i // 4) % 4
            seed = 20000 + 1000 * MODELS.index(key) + 16 * i
            inputs, _ = pose_inputs(layers[l], "mixed" if i % 3 else "mid", B, seed)
            if B and i in GROUP_BCAST_BETAS:
                inputs["betas"] = inputs["betas"][:1].contiguous()
            if i % 2:
                inputs["transl"] = None
            if i == GROUP_TRANSL_ONE:
                inputs["transl"] = inputs["transl"][:1].contiguous()
            if i == GROUP_ORIENT_ONE:
                inputs["global_orient"] = inputs["global_orient"][:1].contiguous()
            groups.append(dict(layer=l, B=B, inputs=inputs, weights=upstream(layers[l], B, "both", seed + 500)))
        _CASES[k] = dict(layers=layers, groups=groups)
    return _CASES[k]


def group_yardsticks(key, i, live=True):
    """``yardsticks`` of group i of ``groups16(key)``; ``live`` False: no upstream gradient reaches it (``one_group``)."""
    k = (key, "groups16", i, live)
    if k not in _CASES:
        c = groups16(key)
        grp = c["groups"][i]
        _CASES[k] = yardsticks(c["layers"][grp["layer"]], grp["inputs"], grp["weights"] if live else (None, None))
    return _CASES[k]
