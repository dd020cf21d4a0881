"""Seeded synthetic ARCTIC objects, predictions and targets of the small-loss fixtures (gen_golden_r14.py) and of
tests/test_small_loss*.py.  No ARCTIC object data is committed: the 11 objects here have the reference's names, template lengths
of a few hundred vertices (different for each object), 300 + 300 sub-vertices, 8 + 8 bbox corners and 16 + 16 keypoints, in
metres, with top / bottom part ids.  The MANO models are those of mano_inputs.py.  Shared by the generator and the tests, so
nothing at test time reads the reference."""
import torch

OBJECTS = ["capsulemachine", "box", "ketchup", "laptop", "microwave", "mixer", "notebook", "espressomachine", "waffleiron",
           "scissors", "phone"]
NS, NB_BOX, NKP, NV, NJ = 300, 8, 16, 778, 21
IMG_RES = 224
FIXTURE_B = 6
CASES = {"all_valid": 1401, "left_invalid": 1402, "right_invalid": 1403, "partial": 1404, "no_contact": 1405,
         "small_s": 1406, "tiny_angles": 1407}


def obj_arrays(seed=1400, lengths=None, n_faces=64):
    """construct_obj_tensors' dict for the synthetic objects (fp32, metres)."""
    g = torch.Generator().manual_seed(seed)
    n = len(OBJECTS)
    if lengths is None:
        lengths = [200 + 17 * i + int(torch.randint(0, 9, (1,), generator=g)) for i in range(n)]
    Lm = max(lengths)
    v = torch.zeros(n, Lm, 3)
    parts = torch.zeros(n, Lm, dtype=torch.long)
    mask = torch.zeros(n, Lm)
    for i, L in enumerate(lengths):
        v[i, :L] = 0.08 * torch.randn(L, 3, generator=g)
        parts[i, :L] = 1 + (v[i, :L, 2] < 0).long()          # top (1) above z = 0, bottom (2) below
        mask[i, :L] = 1.0
    sub_top = 0.08 * torch.randn(n, NS, 3, generator=g).abs() * torch.tensor([1.0, 1.0, 1.0])
    sub_bottom = -0.08 * torch.randn(n, NS, 3, generator=g).abs()
    v_sub = torch.cat([sub_top, sub_bottom], 1)
    parts_sub = torch.cat([torch.ones(n, NS, dtype=torch.long), 2 * torch.ones(n, NS, dtype=torch.long)], 1)
    f = torch.randint(0, min(lengths), (n, n_faces, 3), generator=g)
    return {"names": list(OBJECTS), "parts_ids": parts, "parts_sub_ids": parts_sub, "v": v, "v_sub": v_sub,
            "v_len": torch.tensor(lengths, dtype=torch.long), "f": f, "f_len": torch.full((n,), n_faces, dtype=torch.long),
            "diameter": 0.1 + 0.2 * torch.rand(n, generator=g), "mask": mask,
            "bbox_top": 0.1 * torch.randn(n, NB_BOX, 3, generator=g), "bbox_bottom": 0.1 * torch.randn(n, NB_BOX, 3, generator=g),
            "kp_top": 0.1 * torch.randn(n, NKP, 3, generator=g), "kp_bottom": 0.1 * torch.randn(n, NKP, 3, generator=g),
            "mocap_top": [], "mocap_bottom": [], "z_axis": torch.tensor([[0.0, 0.0, -1.0]])}


def _aa(g, n, lo=0.2, hi=2.0):
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    return d * (lo + (hi - lo) * torch.rand(n, 1, generator=g))


def case_inputs(case, B=FIXTURE_B, seed=None, objects=None, obj_seed=1400):
    """(pred, gt, meta_info) in fp32 on the CPU: pred in get_arctic_item's structure ([root_l, root_r, root_o], [pose_l,
    pose_r], [betas_l, betas_r], [rot, rad])."""
    g = torch.Generator().manual_seed(CASES.get(case, 1400) if seed is None else seed)
    names = [OBJECTS[int(i)] for i in torch.randint(0, len(OBJECTS), (B,), generator=g)] if objects is None else objects
    ot = obj_arrays(obj_seed)
    min_len = int(min(ot["v_len"][OBJECTS.index(n)] for n in names))

    def root(bs):
        return torch.stack([0.4 + 0.5 * torch.rand(bs, generator=g), 0.1 * torch.randn(bs, generator=g),
                            0.1 * torch.randn(bs, generator=g)], 1)
    pred_root = [root(B) for _ in range(3)]
    pose = [_aa(g, 16 * B).view(B, 48) for _ in range(2)]
    betas = [torch.randn(B, 10, generator=g) for _ in range(2)]
    rot = _aa(g, B)
    rad = 0.5 * torch.rand(B, 1, generator=g)
    gt = {}
    for s in ("l", "r"):
        gt["mano.pose." + s] = _aa(g, 16 * B).view(B, 48)
        gt["mano.beta." + s] = torch.randn(B, 10, generator=g)
        gt["mano.j3d.cam." + s] = 0.05 * torch.randn(B, NJ, 3, generator=g)
        gt["mano.j2d.norm." + s] = 0.5 * torch.randn(B, NJ, 2, generator=g)
        gt["mano.cam_t.wp." + s] = root(B)
        gt["joints_valid_" + s] = torch.ones(B, NJ)
    gt["object.kp3d.cam"] = 0.1 * torch.randn(B, 2 * NKP, 3, generator=g)
    gt["object.kp2d.norm.t"] = 0.5 * torch.randn(B, NKP, 2, generator=g)
    gt["object.kp2d.norm.b"] = 0.5 * torch.randn(B, NKP, 2, generator=g)
    gt["object.rot"] = _aa(g, B)
    gt["object.radian"] = 0.5 * torch.rand(B, generator=g)
    gt["object.cam_t.wp"] = root(B)
    gt["is_valid"], gt["left_valid"], gt["right_valid"] = torch.ones(B), torch.ones(B), torch.ones(B)
    for k in ("ro", "lo"):
        gt["dist." + k] = 6e-3 * torch.rand(B, NV, generator=g)
        gt["idx." + k] = torch.randint(0, min_len, (B, NV), generator=g)
    f = 900.0 + 200.0 * torch.rand(B, generator=g)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = f, f * (1.0 + 0.05 * torch.rand(B, generator=g))
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = IMG_RES / 2, IMG_RES / 2, 1.0
    if case == "left_invalid":
        gt["left_valid"] = torch.zeros(B)
    elif case == "right_invalid":
        gt["right_valid"] = torch.zeros(B)
    elif case == "partial":
        gt["is_valid"] = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.5, 1.0] * B)[:B]
        gt["left_valid"] = torch.tensor([1.0, 0.5, 1.0, 0.0, 1.0, 1.0] * B)[:B]
        gt["right_valid"] = torch.tensor([0.0, 1.0, 1.0, 1.0, 1.0, 0.5] * B)[:B]
        for s in ("l", "r"):
            gt["joints_valid_" + s] = (torch.rand(B, NJ, generator=g) > 0.3).float()
    elif case == "no_contact":
        for k in ("ro", "lo"):
            gt["dist." + k] = 4e-3 + 2e-3 * torch.rand(B, NV, generator=g)
    elif case == "small_s":
        for r in pred_root:
            r[::2, 0] = 0.02 + 0.05 * torch.rand(r[::2, 0].shape, generator=g)
    elif case == "tiny_angles":
        for p in pose:
            p[0] = 0.0
            p[1, :24] = 3e-7 * torch.randn(24, generator=g)
        rot[0] = 0.0
        rot[1] = 2e-7
        rad[0] = 0.0
    pred = [pred_root, pose, betas, [rot, rad]]
    meta = {"intrinsics": K, "query_names": names}
    return pred, gt, meta


def flat_pred(pred):
    return list(pred[0]) + list(pred[1]) + list(pred[2]) + list(pred[3])


def unflat_pred(t):
    return [list(t[0:3]), list(t[3:5]), list(t[5:7]), list(t[7:9])]


PRED_NAMES = ("root_l", "root_r", "root_o", "pose_l", "pose_r", "betas_l", "betas_r", "rot", "rad")


def upstream(seed):
    """Seeded weights of the 19 terms in the fixtures' weighted sum."""
    return torch.randn(19, generator=torch.Generator().manual_seed(seed)).abs() + 0.5
