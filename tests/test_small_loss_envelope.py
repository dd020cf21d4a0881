"""The small-loss node and the object layer over their whole envelope, on the CPU: the conditions of the seeded builder
(tests/golden/small_loss_envelope_inputs.py), the stubbed fp64 yardstick against ``small_loss_reference`` on real models, the
fp32 restatement (the original's arithmetic) against the fp64 yardstick inside the bounds that the kernels get in
tests/test_small_loss_envelope_gpu.py, and the ``*_supported`` predicates at each limit and one past it."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err

sys.path.insert(0, GOLDEN)
import mano_inputs as MI  # noqa: E402
import small_loss_envelope_inputs as EI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.mano import MANO  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors, object_tensors_reference  # noqa: E402
from uvhand_amd.small_loss import KEYS, small_loss_reference  # noqa: E402

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = EI.named_node_case(name)
    return _CASES[name]


def _library():
    try:
        return _native.load()
    except (RuntimeError, OSError) as e:
        pytest.skip("the HIP library does not load here: %s" % e)


def test_case_table_is_the_issues():
    assert len(EI.SHAPE_DIMS) == 11 and len(EI.FLAGS) == 9 and len(EI.CONTACTS) == 6 and len(EI.EDGES) == 10
    assert len(EI.NODE_CASES) == 36 and EI.NV1024 in EI.NODE_CASES and EI.SETS8 in EI.NODE_CASES
    for c in EI.NODE_CASES.values():
        assert len(c["dims"]) == 7 and c["dims"][0] <= 8


@pytest.mark.parametrize("name", list(EI.NODE_CASES))
def test_builder_conditions_hold(name):
    c = case(name)
    EI.check_node_case(c)
    S, B, J, NV, KO, NB, L = c["dims"]
    assert len(c["inputs"]) == S and all(len(x) == 15 and all(t.dtype == torch.float32 for t in x) for x in c["inputs"])
    shapes = [(B, 3)] * 3 + [(B, 48)] * 2 + [(B, NB)] * 2 + [(B, 3), (B,)] + [(B, NV, 3)] * 2 + [(B, J, 3)] * 2 + [(B, L, 3), (B, KO, 3)]
    assert all([tuple(t.shape) for t in x] == shapes for x in c["inputs"])
    for k in ("ro", "lo"):
        assert int(c["gt"]["idx." + k].min()) >= 0 and int(c["gt"]["idx." + k].max()) < L
    y = EI.yardstick_gt(c["gt"])
    for k in ("dist.ro", "dist.lo"):
        assert y[k].dtype == torch.float64 and set(y[k].unique().tolist()) <= {0.0, 1.0}
        assert torch.equal(y[k] == 0, c["gt"][k] <= torch.tensor(EI.F32_GATE))


def test_builder_cases_reach_what_they_are_for():
    c = case(EI.NV1024)                                         # 2 x 1024 contacts staged, all on five object vertices
    for k in ("ro", "lo"):
        assert bool((c["gt"]["dist." + k] < 3e-3).all()) and sorted(c["gt"]["idx." + k].unique().tolist()) == [0, 1, 2, 3, 4]
    d = case("contact-threshold")["gt"]["dist.ro"].numpy()
    gate = EI.F32_GATE
    assert (d[:, 0] < gate).all() and (d[:, 1] == gate).all() and (d[:, 2] > gate).all()
    assert (d[:, 0] == np.nextafter(gate, np.float32(0))).all() and (d[:, 2] == np.nextafter(gate, np.float32(1))).all()
    # the fp64 comparison would drop the vertex at float32(3e-3) that the fp32 one keeps: the yardstick is handed the fp32 answer
    assert float(gate) > 3e-3 and float(EI.yardstick_gt(case("contact-threshold")["gt"])["dist.ro"][0, 1]) == 0.0
    assert float(case("edge-s_eq")["inputs"][0][2][0, 0]) == float(np.float32(0.1))
    assert float(case("edge-s_ulp")["inputs"][0][0][0, 0]) == float(np.nextafter(np.float32(0.1), np.float32(1)))
    for e, n in (("pose5e-7", 5e-7), ("pose2e-6", 2e-6), ("pose3.1", 3.1), ("pose6.0", 6.0), ("pose0", 0.0)):
        got = case("edge-" + e)["inputs"][0][3][0].view(16, 3).double().norm(dim=1)
        assert torch.allclose(got, torch.full_like(got, n), rtol=1e-6, atol=0), e
    half = case("flags-half")["gt"]
    assert float(half["is_valid"].sum()) != 0 and not bool(half["is_valid"].long().bool().any())


def test_builder_raises_on_a_broken_condition():
    c = EI.named_node_case("shape-2x3x21x100x32x10x50")
    x = c["inputs"][1]
    ct = EI.cam_t64(x[2], c["meta"]["intrinsics"])
    x[13][1, 7, 2] = float(x[13][0, 7, 2].double() + ct[0, 2] - ct[1, 2])          # a smoothing difference of about 0
    with pytest.raises(ValueError, match="smoothing"):
        EI.check_node_case(c)
    c = EI.named_node_case("contact-vertex0")
    x = c["inputs"][0]
    K = c["meta"]["intrinsics"]
    x[10][2, 3] = (x[13][2, 0].double() + EI.cam_t64(x[2], K)[2] - EI.cam_t64(x[1], K)[2]).float()   # right hand on the vertex
    with pytest.raises(ValueError, match="contact"):
        EI.check_node_case(c)
    c = EI.named_node_case("edge-pose5e-7")
    c["inputs"][0][4][1, 15:18] = torch.tensor([1e-6, 0.0, 0.0])
    with pytest.raises(ValueError, match="switch"):
        EI.check_node_case(c)
    _, groups = EI.object_case(EI.OBJECT_MODELS[2], [(2, 10, True)], 5)
    groups[0]["global_orient"][1] = torch.tensor([0.0, 1.005e-6, 0.0])
    with pytest.raises(ValueError, match="switch"):
        EI.check_object_case(groups)


def test_object_builder():
    for dims in EI.OBJECT_MODELS:
        ot, groups = EI.object_case(dims, [(2, dims[1], True), (1, 1, False)], 3)
        layer = ObjectTensors.from_arrays(ot)
        assert layer._dims() == dims
        if dims[1] > 2:
            assert sorted(ot["parts_ids"].unique().tolist()) == [0, 1, 2]
        assert int(ot["v_len"].max()) <= dims[1] and groups[1]["transl"] is None
        out = object_tensors_reference(layer.obj_tensors, groups[0]["angles"].double(), groups[0]["global_orient"].double(),
                                       groups[0]["transl"].double(), groups[0]["obj_idx"], groups[0]["len"])
        assert tuple(out["v"].shape) == (2, dims[1], 3) and tuple(out["kp3d"].shape) == (2, dims[5] + dims[6], 3)
    assert len(EI.SIXTEEN) == 16 and [g[0] for g in EI.SIXTEEN if g[0] == 0] == [0, 0, 0]
    assert EI.SIXTEEN[0][0] == 0 and EI.SIXTEEN[7][0] == 0 and EI.SIXTEEN[15][0] == 0
    assert {g[1] for g in EI.SIXTEEN} >= {1, 255, 256, 257} and {g[2] for g in EI.SIXTEEN[::2]} == {True}


def test_stubbed_yardstick_equals_the_restatement_on_real_models():
    """The stubs add nothing: the 19 terms from tensors that the real MANO and object layer produced are those of the real run."""
    pred, gt, meta = SI.case_inputs("all_valid")
    m = {"mano_l": MANO.from_arrays(**MI.model_arrays("left", dtype=torch.float32), is_rhand=False),
         "mano_r": MANO.from_arrays(**MI.model_arrays("right", dtype=torch.float32)),
         "arti_head": ObjectTensors.from_arrays(SI.obj_arrays())}
    real = small_loss_reference(pred, gt, meta, m, SI.IMG_RES, dtype=torch.float64)
    x = [t.double() for t in SI.flat_pred(pred)]
    x[8] = x[8].reshape(-1)
    for side, p, b in (("l", x[3], x[5]), ("r", x[4], x[6])):
        out = m["mano_" + side](betas=b, hand_pose=p[:, 3:], global_orient=p[:, :3])
        x += [out.vertices.double()]
    for side, p, b in (("l", x[3], x[5]), ("r", x[4], x[6])):
        out = m["mano_" + side](betas=b, hand_pose=p[:, 3:], global_orient=p[:, :3])
        x += [out.joints.double()]
    obj = m["arti_head"].forward(x[8].view(-1, 1), x[7], None, meta["query_names"])
    x += [obj["v"].double(), obj["kp3d"].double()]
    assert SI.IMG_RES == EI.IMG_RES
    stub = small_loss_reference(EI.pred_of(x), gt, meta, EI.stub_models(x), EI.IMG_RES, dtype=torch.float64)
    assert list(stub) == list(real) == list(KEYS)
    for k in KEYS:
        assert torch.equal(stub[k], real[k]), k


_YARD = {}


def yardstick(name, s):
    if (name, s) not in _YARD:
        _YARD[name, s] = EI.reference_run(small_loss_reference, case(name), s, torch.float64)
    return _YARD[name, s]


@pytest.mark.parametrize("name", list(EI.NODE_CASES))
def test_fp32_restatement_within_the_kernels_bounds(name):
    c = case(name)
    worst_v = worst_g = 0.0
    for s in range(c["dims"][0]):
        ref_v, ref_g = yardstick(name, s)
        got_v, got_g = EI.reference_run(small_loss_reference, c, s, torch.float32)
        worst_v = max(worst_v, EI.scalar_errors(got_v, ref_v))
        for a, r in zip(got_g, ref_g):
            assert bool(torch.isfinite(r).all())
            worst_g = max(worst_g, rel_err(a.double().numpy(), r.numpy()))
    print("MEASURED-CPU %s values %.2e grads %.2e" % (name, worst_v, worst_g))
    assert worst_v < EI.TOL["node_values"] and worst_g < EI.TOL["node_grads"]


def test_half_flags_yardstick_is_nan_where_the_masks_are_empty():
    """Every flag 0.5: each vector_loss's mask has a non-zero sum and keeps no frame, so its mean is over nothing: NaN, with a
    zero gradient.  The pose, shape and articulation inputs reach only such terms."""
    v, g = yardstick("flags-half", 0)
    nan = {k for k, x in zip(KEYS, v) if bool(torch.isnan(x))}
    assert nan == {k for k in KEYS if k.split("/")[-2] in ("pose", "beta", "cam_t", "transl") or k.startswith("loss/object/")
                   and not k.endswith("smoothing")} | {"loss/mano/transl/l", "loss/object/transl"}
    for i in (3, 4, 5, 6, 7, 8):
        assert not bool(g[i].any()), EI.INPUT_NAMES[i]
    assert all(bool(torch.isfinite(t).all()) for t in g) and bool(g[13].any()) and bool(g[11].any())


def test_one_frame_raises_in_the_restatement():
    """B = 1: the original's obj_smt_loss reads v[1]."""
    c = EI.node_case((1, 1, 21, 100, 32, 10, 50), seed=2400)
    with pytest.raises(IndexError):
        EI.reference_run(small_loss_reference, c, 0, torch.float64)


@pytest.mark.parametrize("dims,ok", EI.NODE_PREDICATE)
def test_small_loss_supported_limits(dims, ok):
    _library()
    assert _native.small_loss_supported(*dims) is ok
    assert (_native.small_loss_workspace_bytes(*dims) > 0) is ok


@pytest.mark.parametrize("dims,ok", EI.OBJECT_PREDICATE)
def test_object_supported_limits(dims, ok):
    _library()
    assert _native.object_supported(*dims) is ok
