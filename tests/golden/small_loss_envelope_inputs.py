"""Seeded inputs of the small-loss and object-layer envelope tests (tests/test_small_loss_envelope*.py): torch and numpy only,
nothing read from the reference, shared by the CPU and the GPU file.

``node_case(dims, flags, contact, seed, edge)`` builds the 15 per-set inputs of the loss node of csrc/msda_small_loss.hip
directly for ``dims = (S, B, J, NV, KO, NB, L)``, with the ``gt`` dict and ``meta_info``; no MANO and no object model are
involved.  ``stub_models(inputs)`` gives a ``pre_process_models`` whose hands and object layer hand those tensors back, so that
``small_loss_reference(..., dtype=torch.float64)`` is the node's yardstick with the vertices, joints, ``v`` and ``kp3d`` as
autograd leaves (``reference_run``).  ``object_case(model_dims, groups, seed)`` builds a synthetic ``construct_obj_tensors``
dict and the per-group inputs of ``objects_many``.

The builder conditions its inputs, verifies the conditions on what it returns and raises ``ValueError`` where one does not
hold, so that the tests compare every output element:
  smoothing sign    every element of every consecutive-frame difference of v + cam_t (fp64, camera term included) has magnitude
                    >= 1e-4: the L1 gradient is a sign, and an fp32 rounding (about 2e-6 at z of order 20) cannot flip it.  The
                    builder moves the offending elements of the later frame by 8e-4 before it checks.
  contact distance  every contact that the gates keep has hand-object distance >= 1e-3 (at 0 the gradient is NaN)
  small angle       no predicted or target axis-angle lies within 1 % of the 1e-6 switch to the series
  threshold gate    ``dist > 3e-3`` is decided in fp32 as the original does; ``yardstick_gt`` hands the fp64 run ``dist`` values
                    already resolved by that comparison to 0 (contact) or 1 (none), so the neighbours of float32(3e-3) test the
                    kernel's comparison and not the yardstick's dtype."""
import types

import numpy as np
import torch

IMG_RES = 224
INPUT_NAMES = ("root_l", "root_r", "root_o", "pose_l", "pose_r", "betas_l", "betas_r", "rot", "rad", "vert_l", "vert_r",
               "jnt_l", "jnt_r", "obj_v", "obj_kp")
SMOOTH_MIN, CONTACT_MIN, SWITCH = 1e-4, 1e-3, 1e-6
F32_GATE = np.float32(3e-3)
F32_MIN_S = np.float32(0.1)

# ---- the cases of the issue ---------------------------------------------------------------------------------------------------
SHAPE_DIMS = [(1, 2, 1, 1, 2, 1, 1), (2, 3, 21, 100, 32, 10, 50), (1, 3, 21, 128, 32, 10, 85), (1, 3, 21, 129, 32, 10, 86),
              (1, 2, 21, 256, 32, 10, 256), (1, 2, 21, 257, 32, 10, 257), (1, 2, 32, 778, 64, 16, 300),
              (1, 2, 21, 1024, 32, 10, 5), (1, 2, 21, 64, 32, 10, 65536), (8, 2, 21, 200, 32, 10, 120),
              (3, 33, 21, 300, 32, 10, 200)]
FLAG_DIMS = (2, 6, 21, 100, 32, 10, 50)
FLAGS = ("is_valid0", "left0", "right0", "both0", "half", "last_only", "first_only", "jv_l0", "partial")
SMALL_DIMS = (1, 4, 21, 100, 32, 10, 50)
CONTACTS = ("none", "one_hand", "one_frame", "vertex0", "threshold", "half_flag")
EDGES = ("s_eq", "s_small", "s_ulp", "pose0", "pose5e-7", "pose2e-6", "pose3.1", "pose6.0", "gt_pose0", "rad_rot0")
NV1024, SETS8 = "shape-1x2x21x1024x32x10x5", "shape-8x2x21x200x32x10x120"


def _node_table():
    t = {}
    for i, d in enumerate(SHAPE_DIMS):
        t["shape-" + "x".join(map(str, d))] = dict(dims=d, contact="full" if d[3] == 1024 else "random", seed=2000 + i)
    for i, f in enumerate(FLAGS):
        t["flags-" + f] = dict(dims=FLAG_DIMS, flags=f, seed=2100 + i)
    for i, c in enumerate(CONTACTS):
        t["contact-" + c] = dict(dims=SMALL_DIMS, contact=c, seed=2200 + i)
    for i, e in enumerate(EDGES):
        t["edge-" + e] = dict(dims=SMALL_DIMS, edge=e, seed=2300 + i)
    return t


NODE_CASES = _node_table()
OBJECT_MODELS = [(1, 1, 0, 0, 0, 0, 0), (2, 255, 1, 1, 0, 0, 1), (3, 257, 300, 8, 8, 16, 16), (1, 20000, 4096, 32, 32, 128, 128)]
# the sixteen-group call on OBJECT_MODELS[2]: (B, len, transl); a zero-size group first, in the middle and last
SIXTEEN = [(0, 1, True), (1, 257, False), (2, 2, True), (5, 255, False), (3, 256, True), (1, 100, False), (7, 17, True),
           (0, 33, False), (2, 1, True), (4, 128, False), (1, 129, True), (6, 200, False), (3, 64, True), (2, 257, False),
           (5, 3, True), (0, 50, False)]


# ---- loss node ------------------------------------------------------------------------------------------------------------------
def _aa(g, n, lo=0.2, hi=2.0):
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    return d * (lo + (hi - lo) * torch.rand(n, 1, generator=g))


def _dirs(g, n, norm):
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return (d / d.norm(dim=1, keepdim=True) * norm).float()


def _root(g, B):
    return torch.stack([0.4 + 0.5 * torch.rand(B, generator=g), 0.1 * torch.randn(B, generator=g),
                        0.1 * torch.randn(B, generator=g)], 1)


def cam_t64(root, K):
    """weak_perspective_to_perspective in fp64 from the fp32 inputs."""
    root, K = root.double(), K.double()
    f = (K[:, 0, 0] + K[:, 1, 1]) / 2.0
    return torch.stack([root[:, 1], root[:, 2], 2 * f / (IMG_RES * torch.clamp(root[:, 0], 0.1) + 1e-9)], -1)


def _set_flags(gt, flags, B, J, g):
    one, zero = torch.ones(B), torch.zeros(B)
    if flags == "is_valid0":
        gt["is_valid"] = zero
    elif flags == "left0":
        gt["left_valid"] = zero
    elif flags == "right0":
        gt["right_valid"] = zero
    elif flags == "both0":
        gt["left_valid"], gt["right_valid"] = zero, zero.clone()
    elif flags == "half":                           # sums non-zero, .long().bool() keeps nothing
        for k in ("is_valid", "left_valid", "right_valid"):
            gt[k] = 0.5 * one
        for s in ("l", "r"):
            gt["joints_valid_" + s] = 0.5 * torch.ones(B, J)
    elif flags == "last_only":
        gt["is_valid"] = zero.clone()
        gt["is_valid"][B - 1] = 1.0
    elif flags == "first_only":
        gt["is_valid"] = zero.clone()
        gt["is_valid"][0] = 1.0
    elif flags == "jv_l0":
        gt["joints_valid_l"] = torch.zeros(B, J)
    elif flags == "partial":                        # the pattern of small_loss_inputs.py
        gt["is_valid"] = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.5, 1.0] * B)[:B]
        gt["left_valid"] = torch.tensor([1.0, 0.5, 1.0, 0.0, 1.0, 1.0] * B)[:B]
        gt["right_valid"] = torch.tensor([0.0, 1.0, 1.0, 1.0, 1.0, 0.5] * B)[:B]
        for s in ("l", "r"):
            gt["joints_valid_" + s] = (torch.rand(B, J, generator=g) > 0.3).float()
    elif flags != "all":
        raise KeyError(flags)


def _set_contact(gt, contact, B, NV, L, g):
    far = lambda: 4e-3 + 2e-3 * torch.rand(B, NV, generator=g)  # noqa: E731
    if contact == "none":
        gt["dist.ro"], gt["dist.lo"] = far(), far()
    elif contact == "one_hand":
        gt["dist.lo"] = far()
    elif contact == "one_frame":
        for k in ("ro", "lo"):
            d = far()
            d[1] = gt["dist." + k][1]
            gt["dist." + k] = d
    elif contact == "vertex0":
        for k in ("ro", "lo"):
            gt["dist." + k] = torch.full((B, NV), 1e-3)
            gt["idx." + k] = torch.zeros(B, NV, dtype=torch.long)
    elif contact == "full":                         # every hand vertex in contact, both hands on the same few object vertices
        for k in ("ro", "lo"):
            gt["dist." + k] = torch.full((B, NV), 1e-3)
    elif contact == "threshold":                    # the three fp32 neighbours of float32(3e-3) in vertices 0, 1, 2
        for k in ("ro", "lo"):
            d = far()
            d[:, 0] = float(np.nextafter(F32_GATE, np.float32(0)))
            d[:, 1] = float(F32_GATE)
            d[:, 2] = float(np.nextafter(F32_GATE, np.float32(1)))
            gt["dist." + k] = d
    elif contact == "half_flag":                    # frame 1's left flag is 0.5 while it has contacts
        gt["left_valid"] = gt["left_valid"].clone()
        gt["left_valid"][1] = 0.5
    elif contact != "random":
        raise KeyError(contact)


def _set_edge(inputs, gt, edge, g):
    if edge is None:
        return
    for x in inputs:
        B = x[0].shape[0]
        if edge in ("s_eq", "s_small", "s_ulp"):
            s = {"s_eq": F32_MIN_S, "s_small": np.float32(0.05), "s_ulp": np.nextafter(F32_MIN_S, np.float32(1))}[edge]
            for h in range(3):
                x[h][0, 0] = float(s)
                x[h][B - 1, 0] = float(s)
        elif edge.startswith("pose"):
            norm = float(edge[4:])
            for h in (3, 4):                        # frame 0: every joint; frame 1: joint 5 only
                x[h][0] = (_dirs(g, 16, norm) if norm else torch.zeros(16, 3)).reshape(48)
                x[h][1, 15:18] = (_dirs(g, 1, norm) if norm else torch.zeros(1, 3)).reshape(3)
        elif edge == "rad_rot0":
            x[7].zero_()
            x[8].zero_()
    if edge == "gt_pose0":
        for s in ("l", "r"):
            gt["mano.pose." + s][0] = 0.0
            gt["mano.pose." + s][1, 15:18] = 0.0
    elif edge not in ("s_eq", "s_small", "s_ulp", "rad_rot0") and not edge.startswith("pose"):
        raise KeyError(edge)


def _condition_smoothing(x, K):
    """Move elements of the later frame so that no consecutive-frame difference of v + cam_t is within 4e-4 of zero."""
    ct = cam_t64(x[2], K)
    v = x[13].double()
    for b in range(1, v.shape[0]):
        d = (v[b - 1] + ct[b - 1]) - (v[b] + ct[b])
        bad = d.abs() < 4 * SMOOTH_MIN
        v[b] = torch.where(bad, v[b] - torch.where(d >= 0, 1.0, -1.0) * 8 * SMOOTH_MIN, v[b])
    x[13] = v.float()


def node_case(dims, flags="all", contact="random", seed=0, edge=None):
    """dict(dims, inputs [S][15] fp32, gt, meta, weights [S, 19]); see the module docstring for the conditions."""
    S, B, J, NV, KO, NB, L = dims
    g = torch.Generator().manual_seed(seed)
    gt = {}
    for s in ("l", "r"):
        gt["mano.pose." + s] = _aa(g, 16 * B).view(B, 48)
        gt["mano.beta." + s] = torch.randn(B, NB, generator=g)
        gt["mano.j3d.cam." + s] = 0.05 * torch.randn(B, J, 3, generator=g)
        gt["mano.j2d.norm." + s] = 0.5 * torch.randn(B, J, 2, generator=g)
        gt["mano.cam_t.wp." + s] = _root(g, B)
        gt["joints_valid_" + s] = torch.ones(B, J)
    gt["object.kp3d.cam"] = 0.1 * torch.randn(B, KO, 3, generator=g)
    gt["object.kp2d.norm.t"] = 0.5 * torch.randn(B, KO // 2, 2, generator=g)
    gt["object.kp2d.norm.b"] = 0.5 * torch.randn(B, KO - KO // 2, 2, generator=g)
    gt["object.rot"] = _aa(g, B)
    gt["object.radian"] = 0.5 * torch.rand(B, generator=g)
    gt["object.cam_t.wp"] = _root(g, B)
    gt["is_valid"], gt["left_valid"], gt["right_valid"] = torch.ones(B), torch.ones(B), torch.ones(B)
    for k in ("ro", "lo"):
        gt["dist." + k] = 6e-3 * torch.rand(B, NV, generator=g)
        gt["idx." + k] = torch.randint(0, L, (B, NV), generator=g)
    f = 900.0 + 200.0 * torch.rand(B, generator=g)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = f, f * (1.0 + 0.05 * torch.rand(B, generator=g))
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = IMG_RES / 2, IMG_RES / 2, 1.0
    _set_flags(gt, flags, B, J, g)
    _set_contact(gt, contact, B, NV, L, g)
    inputs = []
    for _ in range(S):
        inputs.append([_root(g, B), _root(g, B), _root(g, B), _aa(g, 16 * B).view(B, 48), _aa(g, 16 * B).view(B, 48),
                       torch.randn(B, NB, generator=g), torch.randn(B, NB, generator=g), _aa(g, B),
                       0.5 * torch.rand(B, generator=g), 0.05 * torch.randn(B, NV, 3, generator=g),
                       0.05 * torch.randn(B, NV, 3, generator=g), 0.05 * torch.randn(B, J, 3, generator=g),
                       0.05 * torch.randn(B, J, 3, generator=g), 0.08 * torch.randn(B, L, 3, generator=g),
                       0.1 * torch.randn(B, KO, 3, generator=g)])
    _set_edge(inputs, gt, edge, g)
    for x in inputs:
        _condition_smoothing(x, K)
    weights = torch.randn(S, 19, generator=g).abs() + 0.5
    case = dict(dims=tuple(dims), inputs=inputs, gt=gt, meta={"intrinsics": K, "query_names": [None] * B}, weights=weights)
    check_node_case(case)
    return case


def named_node_case(name):
    return node_case(**NODE_CASES[name])


def check_node_case(case):
    """Raise ValueError unless the module docstring's conditions hold for what ``case`` carries."""
    gt, K = case["gt"], case["meta"]["intrinsics"]
    gate = gt["is_valid"].double()
    poses = [gt["mano.pose.l"], gt["mano.pose.r"]]
    for s, x in enumerate(case["inputs"]):
        ct = [cam_t64(x[h], K) for h in range(3)]
        v = x[13].double() + ct[2][:, None, :]
        if v.shape[0] > 1 and float((v[:-1] - v[1:]).abs().min()) < SMOOTH_MIN:
            raise ValueError("set %d: a smoothing difference is below %g" % (s, SMOOTH_MIN))
        for h, key, flag in ((1, "ro", "right_valid"), (0, "lo", "left_valid")):
            keep = (gt["dist." + key] <= torch.tensor(F32_GATE)) & ((gt[flag].double() * gate) == 1)[:, None]
            if float((gt[flag] * gt["is_valid"]).sum()) == 0 or not bool(keep.any()):
                continue
            vo = torch.gather(v, 1, gt["idx." + key][:, :, None].repeat(1, 1, 3))
            d = (vo - (x[9 + h].double() + ct[h][:, None, :])).norm(dim=2)
            if float(d[keep].min()) < CONTACT_MIN:
                raise ValueError("set %d: a kept contact is closer than %g" % (s, CONTACT_MIN))
        poses += [x[3], x[4]]
    for p in poses:
        n = p.double().reshape(-1, 3).norm(dim=1)
        if bool(((n > 0.99 * SWITCH) & (n < 1.01 * SWITCH)).any()):
            raise ValueError("an axis-angle lies within 1 % of the small-angle switch")


def yardstick_gt(gt):
    """``gt`` for the fp64 run: the contact gate resolved by the original's fp32 comparison (0 = contact, 1 = none)."""
    out = dict(gt)
    for k in ("dist.ro", "dist.lo"):
        assert gt[k].dtype == torch.float32
        out[k] = torch.where(gt[k] > torch.tensor(F32_GATE), 1.0, 0.0).double()
    return out


def pred_of(x):
    """The first nine inputs in get_arctic_item's structure."""
    return [[x[0], x[1], x[2]], [x[3], x[4]], [x[5], x[6]], [x[7], x[8]]]


def stub_models(x):
    """pre_process_models whose hands return (x[9..12]) and whose object layer returns (x[13], x[14]) whatever they are given."""
    def hand(v, j):
        return lambda **kw: types.SimpleNamespace(vertices=v, joints=j)
    head = types.SimpleNamespace(forward=lambda *a, **kw: {"v": x[13], "kp3d": x[14]})
    return {"mano_l": hand(x[9], x[11]), "mano_r": hand(x[10], x[12]), "arti_head": head}


def reference_run(small_loss_reference, case, s, dtype):
    """Set ``s`` through the stubbed restatement in ``dtype``: (values [19], the 15 input gradients) under the case's upstream
    weights.  fp64 is the yardstick (on yardstick_gt); fp32 is the original's arithmetic."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in case["inputs"][s]]
    gt = yardstick_gt(case["gt"]) if dtype == torch.float64 else case["gt"]
    d = small_loss_reference(pred_of(leaves), gt, case["meta"], stub_models(leaves), IMG_RES, dtype=dtype)
    vals = torch.stack([v.reshape(-1)[0] for v in d.values()])
    (vals * case["weights"][s].to(dtype)).sum().backward()          # a NaN term still hands its weight down
    return vals.detach(), [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]


# ---- models past the node's limits, for the dispatch tests ----------------------------------------------------------------------
def resized_mano_arrays(arrays, V, NB, n_extra):
    """MANO.from_arrays keywords of mano_inputs.model_arrays with V vertices (rows repeated), NB betas and n_extra tips."""
    v0, nb0 = arrays["v_template"].shape[0], arrays["shapedirs"].shape[-1]
    idx = torch.arange(V) % v0
    out = dict(arrays)
    out["v_template"] = arrays["v_template"][idx]
    sd = arrays["shapedirs"][idx]
    out["shapedirs"] = torch.cat([sd, 0.5 * sd[..., :1].repeat(1, 1, NB - nb0)], -1) if NB > nb0 else sd[..., :NB]
    out["posedirs"] = arrays["posedirs"].view(-1, v0, 3)[:, idx].reshape(-1, 3 * V)
    jr = torch.zeros(arrays["J_regressor"].shape[0], V, dtype=arrays["J_regressor"].dtype)
    jr[:, :min(v0, V)] = arrays["J_regressor"][:, :min(v0, V)]
    out["J_regressor"] = jr
    out["lbs_weights"] = arrays["lbs_weights"][idx]
    out["faces"] = arrays["faces"] % V
    out["extra_joints_idxs"] = (torch.arange(n_extra) * 37 + 11) % V
    return out


# ---- object layer ---------------------------------------------------------------------------------------------------------------
def object_model(model_dims, seed):
    """construct_obj_tensors' dict (fp32, metres) for (n_obj, Lm, NS, NBt, NBb, NKt, NKb).  Rows past an object's v_len have
    part id 0 (padding, transformed as the bottom part) and keep non-zero coordinates, so that a kernel which took them for the
    top part would show; parts_ids holds 0, 1 and 2 wherever Lm allows."""
    n, Lm, NS, NBt, NBb, NKt, NKb = model_dims
    g = torch.Generator().manual_seed(seed)
    v_len = [Lm] + [max(1, Lm - 3 - 5 * i) for i in range(1, n)]
    if n == 1 and Lm > 2:
        v_len[0] = Lm - 2
    v = 0.08 * torch.randn(n, Lm, 3, generator=g)
    parts = 1 + (torch.rand(n, Lm, generator=g) < 0.5).long()
    mask = torch.ones(n, Lm)
    for i, ln in enumerate(v_len):
        parts[i, ln:] = 0
        mask[i, ln:] = 0.0
    r = lambda k: 0.1 * torch.randn(n, k, 3, generator=g)  # noqa: E731
    return {"names": ["obj%d" % i for i in range(n)], "parts_ids": parts, "v": v, "v_sub": 0.08 * torch.randn(n, NS, 3, generator=g),
            "parts_sub_ids": 1 + (torch.rand(n, NS, generator=g) < 0.5).long(), "v_len": torch.tensor(v_len, dtype=torch.long),
            "f": torch.randint(0, min(v_len), (n, 8, 3), generator=g), "f_len": torch.full((n,), 8, dtype=torch.long),
            "diameter": 0.1 + 0.2 * torch.rand(n, generator=g), "mask": mask, "bbox_top": r(NBt), "bbox_bottom": r(NBb),
            "kp_top": r(NKt), "kp_bottom": r(NKb), "mocap_top": [], "mocap_bottom": [],
            "z_axis": torch.tensor([[0.0, 0.0, -1.0]])}


def object_case(model_dims, groups, seed):
    """(obj_tensors, [dict(angles [B, 1], global_orient [B, 3], transl [B, 3] | None, obj_idx [B], len)]) for groups
    [(B, len, transl?)]."""
    ot = object_model(model_dims, seed)
    g = torch.Generator().manual_seed(seed + 1)
    out = []
    for B, ln, tr in groups:
        out.append(dict(angles=0.1 + torch.rand(B, 1, generator=g), global_orient=_aa(g, B, 0.2, 2.5),
                        transl=0.1 * torch.randn(B, 3, generator=g) if tr else None,
                        obj_idx=torch.randint(0, model_dims[0], (B,), generator=g), len=int(ln)))
    check_object_case(out)
    return ot, out


def check_object_case(groups):
    for grp in groups:
        for t in (grp["angles"].reshape(-1, 1), grp["global_orient"]):
            n = t.double().norm(dim=1)
            if bool(((n > 0.99 * SWITCH) & (n < 1.01 * SWITCH)).any()):
                raise ValueError("an axis-angle lies within 1 % of the small-angle switch")


# ---- the *_supported predicates at each limit and one past it (asserted by the CPU and the GPU file) ---------------------------
NODE_BASE = (1, 2, 21, 778, 32, 10, 300)
OBJECT_BASE = (11, 300, 600, 8, 8, 16, 16)


def _with(base, **kw):
    names = ("S", "B", "J", "NV", "KO", "NB", "L") if len(base) == 7 and base is NODE_BASE else \
        ("n_obj", "Lm", "NS", "NBt", "NBb", "NKt", "NKb")
    d = dict(zip(names, base))
    d.update(kw)
    return tuple(d[n] for n in names)


NODE_PREDICATE = [(NODE_BASE, True), (_with(NODE_BASE, B=0), True)] + \
    [(_with(NODE_BASE, **{k: v}), ok) for k, v, ok in (
        ("S", 8, True), ("S", 9, False), ("S", 0, False), ("J", 32, True), ("J", 33, False), ("J", 0, False),
        ("NV", 1024, True), ("NV", 1025, False), ("NV", 0, False), ("KO", 64, True), ("KO", 66, False), ("KO", 65, False),
        ("KO", 31, False), ("KO", 0, False), ("KO", 2, True), ("NB", 16, True), ("NB", 17, False), ("NB", 0, False),
        ("L", 65536, True), ("L", 65537, False), ("L", 0, False), ("B", -1, False))]
OBJECT_PREDICATE = [(OBJECT_BASE, True), ((1, 1, 0, 0, 0, 0, 0), True)] + \
    [(_with(OBJECT_BASE, **kw), ok) for kw, ok in (
        (dict(n_obj=64), True), (dict(n_obj=65), False), (dict(n_obj=0), False), (dict(Lm=65536), True),
        (dict(Lm=65537), False), (dict(Lm=0), False), (dict(NS=4096), True), (dict(NS=4097), False),
        (dict(NBt=32, NBb=32), True), (dict(NBt=33, NBb=32), False), (dict(NBt=64, NBb=0), True), (dict(NBt=0, NBb=65), False),
        (dict(NKt=128, NKb=128), True), (dict(NKt=128, NKb=129), False), (dict(NKt=0, NKb=256), True), (dict(NS=-1), False))]


# ---- tolerances (tests/test_small_loss_envelope_gpu.py's docstring has the measurements they come from) ------------------------
CEILING = {"node_values": 1e-4, "node_grads": 1e-3, "object_values": 1e-5, "object_grads": 1e-4}
TOL = {"node_values": 3e-5, "node_grads": 5e-4, "object_values": 2e-6, "object_grads": 3e-6}
assert all(TOL[k] <= CEILING[k] for k in CEILING)


def scalar_errors(got, ref):
    """Per-term relative error of two [19] vectors with NaN for NaN required: the largest error over the finite terms (a term
    whose reference is 0 must be exactly 0: its error is then infinite)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (got, ref)
    keep = ~torch.isnan(ref)
    err = (got[keep] - ref[keep]).abs() / ref[keep].abs()
    err = torch.where(got[keep] == ref[keep], torch.zeros_like(err), err)
    return float(err.max()) if err.numel() else 0.0
