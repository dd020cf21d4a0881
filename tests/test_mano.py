"""MANO drop-in on the CPU: the fp64 torch restatement against the manopth fixtures (gen_golden_r13.py), the smplx-style
construction and argument conventions.  Tolerance: the restatement is fp64 and manopth's quaternion Rodrigues agrees with
smplx's formula to ~1e-8 relative (the 1e-8 inside the norm), so 1e-6."""
import sys
import types

import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import mano_inputs as MI  # noqa: E402
from uvhand_amd.mano import MANO, lbs_reference, mano_many  # noqa: E402

TOL = 1e-6


def _layer(side="right", flat=False, **kw):
    return MANO.from_arrays(**MI.model_arrays(side, flat), **kw).double()


@pytest.mark.parametrize("fixture,flat", [("mano_mean", False), ("mano_flat", True)])
@pytest.mark.parametrize("side", ["right", "left"])
def test_restatement_matches_manopth(fixture, flat, side):
    z = load_golden(fixture)
    m = _layer(side, flat)
    leaves = [torch.from_numpy(z["%s/%s" % (side, k)]).requires_grad_(True) for k in ("betas", "global_orient", "hand_pose")]
    out = m(*leaves)
    assert rel_err(out.vertices.detach().numpy(), z[side + "/vertices"]) < TOL
    assert rel_err(out.joints[:, :16].detach().numpy(), z[side + "/joints"]) < TOL
    seed = next(s for sd, f, s in MI.FIXTURE_CASES.values() if sd == side and f == flat)
    wv, wj = MI.upstream(seed + 100, MI.FIXTURE_B)
    ((out.vertices * wv).sum() + (out.joints[:, :16] * wj).sum()).backward()
    for leaf, key in zip(leaves, ("betas", "global_orient", "hand_pose")):
        assert rel_err(leaf.grad.numpy(), z["%s/grad_%s" % (side, key)]) < TOL, key


def _smplx_standin(side="right"):
    """An object with smplx MANO's attribute names (as build_mano_aa makes it, create_transl=True)."""
    a = MI.model_arrays(side, dtype=torch.float32)
    m = types.SimpleNamespace(**{k: v for k, v in a.items() if k not in ("faces", "extra_joints_idxs")})
    m.faces_tensor = a["faces"]
    m.vertex_joint_selector = types.SimpleNamespace(extra_joints_idxs=a["extra_joints_idxs"])
    g = torch.Generator().manual_seed(3)
    m.betas = torch.nn.Parameter(torch.randn(1, 10, generator=g))
    m.global_orient = torch.nn.Parameter(torch.randn(1, 3, generator=g))
    m.hand_pose = torch.nn.Parameter(torch.randn(1, 45, generator=g))
    m.transl = torch.nn.Parameter(torch.randn(1, 3, generator=g))
    m.is_rhand = side == "right"
    return m


def test_from_smplx_copies_by_name():
    src = _smplx_standin("left")
    m = MANO.from_smplx(src)
    for name in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "pose_mean"):
        assert torch.equal(getattr(m, name), getattr(src, name)), name
    assert torch.equal(m.parents, src.parents) and torch.equal(m.faces_tensor, src.faces_tensor)
    assert m.faces.shape == (1538, 3)
    assert torch.equal(m.extra_joints_idxs, src.vertex_joint_selector.extra_joints_idxs)
    for name in ("betas", "global_orient", "hand_pose", "transl"):
        assert torch.equal(getattr(m, name).data, getattr(src, name).data), name
    assert m.is_rhand is False
    assert torch.equal(m.hand_mean, src.pose_mean[3:])


def test_absent_arguments_use_parameters():
    m = MANO.from_smplx(_smplx_standin())
    out = m()
    ref = m(m.betas, m.global_orient, m.hand_pose, m.transl)
    assert torch.equal(out.vertices, ref.vertices) and torch.equal(out.joints, ref.joints)
    assert out.betas is m.betas and out.hand_pose is m.hand_pose
    hp = torch.zeros(1, 45)
    assert not torch.equal(m(hand_pose=hp).vertices, out.vertices)


def test_betas_broadcast_and_summed_gradient():
    m = _layer()
    betas, go, hp = MI.pose_inputs(21, 5)
    b1 = betas[:1].clone().requires_grad_(True)
    out = m(b1, go, hp)
    out.vertices.sum().backward()
    bx = betas[:1].expand(5, -1).clone().requires_grad_(True)
    ref = m(bx, go, hp)
    assert torch.allclose(out.vertices, ref.vertices, rtol=0, atol=1e-12)
    ref.vertices.sum().backward()
    assert torch.allclose(b1.grad, bx.grad.sum(0, keepdim=True), rtol=1e-10, atol=1e-12)


def test_transl_applied():
    m = _layer()
    betas, go, hp = MI.pose_inputs(22, 3)
    t = torch.tensor([[0.1, -0.2, 0.3]], dtype=torch.float64).expand(3, -1)
    a, b = m(betas, go, hp), m(betas, go, hp, transl=t)
    assert torch.allclose(b.vertices - a.vertices, t[:, None, :].expand_as(a.vertices), atol=1e-12)
    assert torch.allclose(b.joints - a.joints, t[:, None, :].expand_as(a.joints), atol=1e-12)


def test_fingertips_are_configured_vertices():
    m = _layer()
    betas, go, hp = MI.pose_inputs(23, 2)
    out = m(betas, go, hp, return_full_pose=True)
    assert out.joints.shape == (2, 21, 3)
    assert torch.equal(out.joints[:, 16:], out.vertices[:, MI.TIPS])
    assert torch.allclose(out.full_pose, torch.cat([go, hp], 1) + m.pose_mean)


def test_lbs_zero_pose_is_rest_shape():
    a = MI.model_arrays("right", True)
    betas = torch.zeros(1, 10, dtype=torch.float64)
    verts, joints = lbs_reference(betas, torch.zeros(1, 48, dtype=torch.float64), a["v_template"], a["shapedirs"], a["posedirs"],
                                  a["J_regressor"], MI.PARENTS, a["lbs_weights"])
    assert torch.allclose(verts[0], a["v_template"], atol=1e-12)
    assert torch.allclose(joints[0], a["J_regressor"] @ a["v_template"], atol=1e-12)


def test_many_on_cpu_matches_single_calls():
    r, l = _layer("right"), _layer("left")
    cases = [MI.pose_inputs(30 + i, b) for i, b in enumerate((2, 3))]
    outs = mano_many([(r,) + cases[0], (l,) + cases[1]])
    for o, lay, c in zip(outs, (r, l), cases):
        ref = lay(*c)
        assert torch.equal(o.vertices, ref.vertices) and torch.equal(o.joints, ref.joints)
