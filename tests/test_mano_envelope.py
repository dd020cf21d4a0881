"""The MANO layer over its whole envelope, on the CPU: the conditions of the seeded builder
(tests/golden/mano_envelope_inputs.py), the angle classes on the fp32 full pose, the bound of every case that
tests/test_mano_envelope_gpu.py compares (4 x the fp32 restatement's deviation from the fp64 one, floor 16 * 2^-24 of the
tensor's largest magnitude; printed as MEASURED-CPU), ``msda_mano_supported`` and ``msda_mano_workspace_bytes`` at each limit
and one past it, and the argument refusals of the C entry points.  Only the last three need the HIP library."""
import ctypes
import math
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import mano_envelope_inputs as EI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.mano import MANO  # noqa: E402

ERR_ARGUMENT = 1


def _library():
    try:
        return _native.load()
    except (RuntimeError, OSError) as e:
        pytest.skip("the HIP library does not load here: %s" % e)


# ---- the case table -----------------------------------------------------------------------------------------------------------
def test_case_table_is_the_issues():
    assert EI.MODELS == [(1, 1, 0, "mano"), (63, 16, 8, "chain"), (64, 10, 5, "star"), (65, 3, 1, "bushy"),
                         (128, 16, 0, "chain"), (778, 10, 5, "mano"), (8192, 16, 8, "bushy")]
    assert EI.MODEL_OPTIONS[(778, 10, 5, "mano")] == dict(dense_regressor=True)
    assert EI.ANGLES == ("zero", "tiny", "small", "mid", "pi", "wide", "axis", "mixed") and sorted(EI.MIX) == sorted(EI.ANGLES[:7])
    assert EI.BATCHES == (1, 7, 8, 9, 17) and EI.UPSTREAM == ("both", "vertices", "joints", "tips", "one_group")
    assert EI.GROUP_B == [0, 0, 1, 8, 9, 0, 17, 3, 0, 8, 1, 2, 16, 5, 0, 0] and sum(EI.GROUP_B) == 70
    assert len(EI.MODEL_CASES) == 56 and len(EI.BATCH_CASES) == 10 and len(EI.UPSTREAM_CASES) == 8
    assert len(EI.SINGLE_CASES) == 70                    # four cases are in two tables
    assert (EI.KHT, EI.KVS, EI.KPART) == (8, 64, 346) and EI.FLOOR == 16 * 2.0 ** -24
    assert max(B for _, _, B, _ in EI.SINGLE_CASES) <= 17 and max(EI.GROUP_B) <= 17


@pytest.mark.parametrize("key", EI.MODELS)
def test_models_hold_their_conditions(key):
    arrays = EI.model(key)
    EI.check_model(arrays, *key, **EI.MODEL_OPTIONS.get(key, {}))
    assert MANO.from_arrays(**arrays)._dims() == key[:3]
    if key in EI.GROUP_MODELS:
        for l in (1, 2, 3):
            EI.check_model(EI.model(key, l), *key[:3], EI.GROUP_TREES[l - 1], zero_mean=l == 2)
    tips = arrays["extra_joints_idxs"].tolist()
    if key == (8192, 16, 8, "bushy"):
        assert tips[:4] == [8191, 0, 0, 8128]
    if key == (65, 3, 1, "bushy"):
        assert tips == [64]                              # the one vertex of the tail slice is a fingertip


def test_trees():
    assert EI.depth_of(EI.tree("chain", 0)) == 15 and EI.depth_of(EI.tree("star", 0)) == 1 and EI.depth_of(EI.tree("mano", 0)) == 3
    for seed in range(20):
        p = EI.tree("bushy", seed)
        assert p[0] == -1 and all(0 <= p[j] < j for j in range(1, 16)) and 4 <= EI.depth_of(p) <= 8
    assert EI.tree("bushy", 3) == EI.tree("bushy", 3)


def test_check_model_raises_on_a_broken_condition():
    key = (64, 10, 5, "star")
    for name, change in (("lbs_weights", lambda a: a["lbs_weights"][3].mul_(1.01)),
                         ("J_regressor", lambda a: a["J_regressor"][0].mul_(0.9)),
                         ("parents", lambda a: a["parents"].__setitem__(5, 5)),
                         ("depth", lambda a: a["parents"].__setitem__(5, 4)),
                         ("tip", lambda a: a["extra_joints_idxs"].__setitem__(0, 7))):
        arrays = {k: v.clone() for k, v in EI.model(key).items()}
        change(arrays)
        with pytest.raises(ValueError, match=name):
            EI.check_model(arrays, *key)


# ---- the angle classes --------------------------------------------------------------------------------------------------------
def _check_class(cls, full, angles):
    """One hand's fp32 full pose [48] and its 16 angles against what class ``cls`` is for."""
    lo, hi = angles.min().item(), angles.max().item()
    if cls == "zero":
        assert not bool(full.any())
    elif cls == "tiny":
        assert 5e-8 < lo and hi < 1e-5
    elif cls == "small":
        assert 1e-4 <= lo and hi <= 1e-2
    elif cls in ("mid", "axis"):
        assert 0.05 - 1e-6 <= lo and hi <= 3.1 + 1e-6
        if cls == "axis":
            assert bool(((full.view(16, 3) != 0).sum(1) == 1).all())
    elif cls == "pi":
        assert math.pi - 1.01e-4 <= lo and hi <= math.pi + 1.01e-4
    else:
        assert 3.2 - 1e-6 <= lo and hi <= 9.5 + 1e-6 and hi > 2 * math.pi


@pytest.mark.parametrize("key", [(64, 10, 5, "star"), (63, 16, 8, "chain"), (8192, 16, 8, "bushy")])
@pytest.mark.parametrize("angles", EI.ANGLES)
def test_angle_classes_hold_on_the_fp32_full_pose(angles, key):
    c = EI.case(key, angles, 9)
    x, full, mean = c["inputs"], c["full"], c["arrays"]["pose_mean"]
    assert full.dtype == torch.float32 and all(t.dtype == torch.float32 for t in x.values())
    pose = torch.cat([x["global_orient"], x["hand_pose"]], 1)
    assert torch.equal(pose.double() + mean.double(), full.double())       # exact in real arithmetic ...
    assert torch.equal(pose + mean, full)                                  # ... and therefore in fp32
    assert not bool((full == torch.tensor(-1e-8, dtype=torch.float32)).any())
    th = EI.joint_angles(full)
    for b in range(9):
        _check_class(EI.MIX[b % 7] if angles == "mixed" else angles, full[b], th[b])
    if angles == "zero":
        assert torch.equal(x["hand_pose"], -mean[3:].expand(9, -1)) and not bool(x["global_orient"].any())
        assert bool(mean[3:].any()) != (key in EI.MODEL_OPTIONS)
    if angles == "mixed":
        assert {EI.MIX[b % 7] for b in range(8)} == set(EI.ANGLES[:7])      # one tile of 8 hands holds every class


def test_builder_refuses_the_component_the_original_cannot_divide_by():
    arrays = dict(EI.model((64, 10, 5, "star")))
    orig = EI.full_pose
    try:
        EI.full_pose = lambda angles, B, seed: torch.full((B, 48), -1e-8, dtype=torch.float64)
        arrays["pose_mean"] = torch.zeros(48)
        with pytest.raises(ValueError, match="-1e-8"):
            EI.pose_inputs(arrays, "tiny", 2, 1)
    finally:
        EI.full_pose = orig


# ---- the bound of every compared case -----------------------------------------------------------------------------------------
def _check_and_print(label, f64, bounds):
    for n in EI.NAMES:
        if f64[n] is None or f64[n].numel() == 0:
            assert n not in bounds
            continue
        dev32, scale, bound = bounds[n]
        print("MEASURED-CPU %s %s dev32 %.2e scale %.2e rel %.2e" % (label, n, dev32, scale, dev32 / (scale + 1e-300)))
        assert bool(torch.isfinite(f64[n]).all()), n
        assert math.isfinite(dev32), n                   # the fp32 restatement itself produced no NaN
        assert math.isfinite(scale) and (scale > 0) == bool(f64[n].any()), n
        assert bound == max(4 * dev32, EI.FLOOR * scale)


@pytest.mark.parametrize("key,angles,B,mode", EI.SINGLE_CASES,
                         ids=["%dx%dx%d%s-%s-B%d-%s" % (k + (a, B, m)) for k, a, B, m in EI.SINGLE_CASES])
def test_bound_of_every_single_call_case(key, angles, B, mode):
    c = EI.case(key, angles, B, mode)
    assert set(c["bounds"]) == set(EI.NAMES)
    _check_and_print("%s %s B%d %s" % ("x".join(map(str, key)), angles, B, mode), c["f64"], c["bounds"])
    E = key[2]
    assert torch.equal(c["f64"]["joints"][:, 16:], c["f64"]["vertices"][:, c["arrays"]["extra_joints_idxs"]])
    if mode == "joints" and E == 0:
        assert bool(c["f64"]["g_betas"].any())           # the J path alone
    if mode == "tips" and E == 0:
        assert all(not bool(c["f64"]["g_" + k].any()) for k in EI.INPUTS)


@pytest.mark.parametrize("key", EI.GROUP_MODELS)
def test_bound_of_every_group_of_sixteen(key):
    c = EI.groups16(key)
    assert [g["B"] for g in c["groups"]] == EI.GROUP_B and {g["layer"] for g in c["groups"]} == {0, 1, 2, 3}
    assert {g["layer"] for g in c["groups"] if g["B"]} == {0, 1, 2, 3}
    for i, g in enumerate(c["groups"]):
        x = g["inputs"]
        if g["B"] == 0:
            assert all(t is None or t.shape[0] == 0 for t in x.values())
            continue
        assert x["betas"].shape[0] == (1 if i in EI.GROUP_BCAST_BETAS else g["B"])
        assert (x["transl"] is None) == bool(i % 2)
        assert x["global_orient"].shape[0] == (1 if i == EI.GROUP_ORIENT_ONE else g["B"]) and x["hand_pose"].shape[0] == g["B"]
        if i == EI.GROUP_TRANSL_ONE:
            assert x["transl"].shape[0] == 1 and g["B"] > 1
        f64, _, bounds = EI.group_yardsticks(key, i)
        _check_and_print("%s group%d" % ("x".join(map(str, key)), i), f64, bounds)
        assert f64["g_betas"].shape == x["betas"].shape and f64["g_global_orient"].shape == x["global_orient"].shape
    dead, _, bounds = EI.group_yardsticks(key, 3, live=False)
    assert all(not bool(dead["g_" + k].any()) for k in EI.INPUTS if dead["g_" + k] is not None)
    assert all(bounds["g_" + k][2] == 0.0 for k in ("betas", "global_orient", "hand_pose"))


# ---- the library's predicates and refusals ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ok", [((1, 10, 5), True), ((8192, 10, 5), True), ((0, 10, 5), False), ((8193, 10, 5), False),
                                     ((778, 1, 5), True), ((778, 16, 5), True), ((778, 0, 5), False), ((778, 17, 5), False),
                                     ((778, 10, 0), True), ((778, 10, 8), True), ((778, 10, -1), False), ((778, 10, 9), False),
                                     ((1, 1, 0), True), ((8192, 16, 8), True)])
def test_mano_supported_limits(dims, ok):
    _library()
    assert _native.mano_supported(*dims) is ok
    assert (_native.mano_workspace_bytes(dims, [3]) > 0) is ok


@pytest.mark.parametrize("V", [1, 64, 65, 8192])
def test_workspace_bytes(V):
    _library()
    group_B = [9, 0, 17, 1]
    slices = -(-V // EI.KVS)
    assert _native.mano_workspace_bytes((V, 16, 8), group_B) == sum(B * slices * EI.KPART * 4 for B in group_B)
    assert _native.mano_workspace_bytes((V, 1, 0), [0]) == 0
    assert _native.mano_workspace_bytes((V, 16, 8), [1, -1]) == 0 and _native.mano_workspace_bytes((V, 16, 8), [1] * 17) == 0


P = 0x10000                                               # a fake device address: nothing below reaches a kernel


def _call(lib, backward, V=65, nb=3, E=1, n_layers=1, index=None, layer=(0,), B=(9,)):
    VP = ctypes.c_void_p
    ptrs = lambda n: ctypes.cast((VP * n)(*([P] * n)), VP)  # noqa: E731
    ints = lambda v: ctypes.cast((ctypes.c_int * len(v))(*v), VP)  # noqa: E731
    index = (EI.tree("chain", 0) + [V - 1] * E) * n_layers if index is None else index
    n = len(B)
    geo = [V, nb, E, n_layers, ptrs(7 * n_layers), ints(index), n, ints(list(layer)), ints(list(B)), None]
    if backward:
        return lib.msda_mano_backward_f32(*geo, ptrs(4 * n), ptrs(2 * n), ptrs(4 * n), P, 1 << 40, None)
    return lib.msda_mano_forward_f32(*geo, ptrs(4 * n), ptrs(2 * n), None)


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("case", ["root", "self_parent", "tip_is_V", "negative_B", "five_layers", "seventeen_groups",
                                  "V0", "V8193", "nb0", "nb17", "E9"])
def test_argument_refusals(case, backward):
    lib = _library()
    chain = EI.tree("chain", 0)
    kw = {"root": dict(index=[0] + chain[1:] + [64]),
          "self_parent": dict(index=chain[:7] + [7] + chain[8:] + [64]),
          "tip_is_V": dict(index=chain + [65]),
          "negative_B": dict(layer=(0, 0), B=(9, -1)),
          "five_layers": dict(n_layers=5, layer=(0, 4), B=(1, 1)),
          "seventeen_groups": dict(layer=[0] * 17, B=[1] * 17),
          "V0": dict(V=0, E=0), "V8193": dict(V=8193), "nb0": dict(nb=0), "nb17": dict(nb=17), "E9": dict(E=9)}[case]
    n0 = lib.msda_launch_count()
    assert _call(lib, backward, **kw) == ERR_ARGUMENT
    assert lib.msda_last_error().decode().startswith("msda_mano")
    assert lib.msda_launch_count() == n0
