"""Seeded synthetic MANO models and inputs of the MANO fixtures (gen_golden_r13.py) and of tests/test_mano*.py.  No MANO model
data is committed: the model here has MANO's sizes (778 vertices, 16 joints, 10 betas, 135 pose directions), its kinematic
tree, lbs_weights rows that sum to 1, J_regressor rows that are sparse convex combinations of vertices near each joint, a
hand-like template and a non-zero hand mean; left and right use different seeds.  Shared by the generator and the tests, so
nothing at test time reads the reference."""
import torch

V, NJ, NB, NPF = 778, 16, 10, 135
PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
TIPS = [744, 320, 443, 554, 671]             # smplx's MANO fingertip vertex ids: thumb, index, middle, ring, pinky
SEEDS = {"right": 1301, "left": 1302}
FIXTURE_B = 4
FIXTURE_CASES = {"right_mean": ("right", False, 1311), "left_mean": ("left", False, 1312),
                 "right_flat": ("right", True, 1313), "left_flat": ("left", True, 1314)}


def _rest_joints(g, sign):
    """A wrist at the origin, five fingers of three joints along +x, spread in z (mirrored for the left hand)."""
    J = torch.zeros(NJ, 3, dtype=torch.float64)
    for f in range(5):
        base = torch.tensor([0.07, 0.0, sign * (-0.03 + 0.015 * f)], dtype=torch.float64)
        for k in range(3):
            J[1 + 3 * f + k] = base + torch.tensor([0.025 * k, 0.0, 0.0], dtype=torch.float64)
    return J + 0.003 * torch.randn(NJ, 3, generator=g, dtype=torch.float64)


def model_arrays(side, flat_hand_mean=False, dtype=torch.float64):
    """The keyword arguments of uvhand_amd.mano.MANO.from_arrays, in smplx's layouts (posedirs [135, 3 V])."""
    g = torch.Generator().manual_seed(SEEDS[side])
    J = _rest_joints(g, 1.0 if side == "right" else -1.0)
    owner = torch.randint(0, NJ, (V,), generator=g)
    v_template = J[owner] + torch.randn(V, 3, generator=g, dtype=torch.float64) * torch.tensor([0.01, 0.006, 0.006],
                                                                                                dtype=torch.float64)
    d2 = ((v_template[:, None, :] - J[None, :, :]) ** 2).sum(-1)
    lbs_weights = torch.softmax(-d2 / 2e-4, dim=1)
    J_regressor = torch.zeros(NJ, V, dtype=torch.float64)
    for j in range(NJ):
        near = torch.argsort(d2[:, j])[:12]
        w = torch.rand(12, generator=g, dtype=torch.float64) + 0.1
        J_regressor[j, near] = w / w.sum()
    shapedirs = 0.004 * torch.randn(V, 3, NB, generator=g, dtype=torch.float64)
    posedirs = 0.003 * torch.randn(NPF, 3 * V, generator=g, dtype=torch.float64)
    hand_mean = 0.25 * torch.randn(45, generator=g, dtype=torch.float64)
    faces = torch.randint(0, V, (1538, 3), generator=g)
    pose_mean = torch.cat([torch.zeros(3, dtype=torch.float64), torch.zeros(45, dtype=torch.float64) if flat_hand_mean
                           else hand_mean])
    f = lambda t: t.to(dtype)  # noqa: E731
    return dict(v_template=f(v_template), shapedirs=f(shapedirs), posedirs=f(posedirs), J_regressor=f(J_regressor),
                lbs_weights=f(lbs_weights), parents=torch.tensor(PARENTS), pose_mean=f(pose_mean), faces=faces,
                extra_joints_idxs=torch.tensor(TIPS))


def hand_mean(side):
    return model_arrays(side)["pose_mean"][3:]


def axis_angles(g, n, lo=0.2, hi=2.5):
    """n axis-angles [n, 3] with random directions and angles in [lo, hi] (kept away from 0)."""
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    return d * (lo + (hi - lo) * torch.rand(n, 1, generator=g, dtype=torch.float64))


def pose_inputs(seed, B, lo=0.2, hi=2.5, mean=None):
    """(betas [B, 10], global_orient [B, 3], hand_pose [B, 45]) in fp64.  With ``mean`` (the layer's hand mean), the hand pose
    is drawn so that the full pose hand_pose + mean has the angles in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    betas = 1.5 * torch.randn(B, NB, generator=g, dtype=torch.float64)
    go = axis_angles(g, B, lo, hi)
    full = axis_angles(g, 15 * B, lo, hi).view(B, 45)
    hp = full - (mean.double() if mean is not None else 0.0)
    return betas, go, hp


def upstream(seed, B, dtype=torch.float64):
    """Seeded weights of the fixtures' weighted sum: (w_vertices [B, V, 3], w_joints [B, 16, 3])."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, V, 3, generator=g, dtype=torch.float64).to(dtype), torch.randn(B, NJ, 3, generator=g,
                                                                                        dtype=torch.float64).to(dtype)
