"""Seeded synthetic inputs of the arctic_pre_process fixtures (gen_pre_process.py) and of tests/test_pre_process*.py, built on
small_loss_inputs.py (synthetic objects, MANO parameters, intrinsics) and arctic_eval_inputs.py (MANO models, camera-space
clouds).  Per frame: ``kp_cano`` is the posed bottom keypoints of the frame's synthetic object; ``object.kp3d.full.b`` is a
random rigid motion of it plus N(0, 1e-3 m) noise; ``object.kp2d.norm.b`` is the projection through K of ``kp_cano + t_true``
with ``t_true.z`` in [0.6, 1.2] m and 0.3 px of noise, normalised by process_data's 224; ``mano.j3d.full.*`` are free draws.
``check_case`` asserts, in fp64 from the data alone, what the tests rely on: every fit has a positive determinant and its
smallest singular value is above 0.05 of the largest.  Shared by the generator and the tests: nothing at test time reads the
reference."""
import torch

import arctic_eval_inputs as EI
import small_loss_inputs as SI
from uvhand_amd.object_tensors import object_tensors_reference

IMG_RES = 224
CASES = {"all_valid": 2301, "partial": 2302, "one_object": 2303}
DF_SEED = 2350
DF_SHAPES = ((778, 1029), (5, 4097), (300, 37), (1, 1))          # (NV, L) of the distance-field tests, B = 3
DF_CHUNK = 1024                                                   # targets the kernel stages in LDS at a time
MIN_RATIO = 0.05
NEAR_TIE, NEAR_TIE_SHARE = 2.0 ** -20, 1e-3


def random_rotations(n, g):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    return q * torch.sign(torch.linalg.det(q))[:, None, None]


def fit_inputs(kp_cano, K, g, noise=1e-3, px_noise=0.3, J=SI.NJ):
    """(object.kp3d.full.b, object.kp2d.norm.b, mano.j3d.full.r, mano.j3d.full.l, t_true) in fp32 for fp32 ``kp_cano [B, NK, 3]``."""
    B, NK, _ = kp_cano.shape
    kc = kp_cano.double()
    R, T = random_rotations(B, g), 0.3 * torch.randn(B, 1, 3, generator=g, dtype=torch.float64)
    kp_full = (kc - T) @ R + noise * torch.randn(B, NK, 3, generator=g, dtype=torch.float64)          # kp_cano = R kp_full + T
    t_true = torch.stack([0.1 * torch.randn(B, generator=g, dtype=torch.float64), 0.1 * torch.randn(B, generator=g, dtype=torch.float64),
                          0.6 + 0.6 * torch.rand(B, generator=g, dtype=torch.float64)], dim=1)
    cam = (kc + t_true[:, None, :]) @ K.double().transpose(1, 2)
    px = cam[..., :2] / cam[..., 2:] + px_noise * torch.randn(B, NK, 2, generator=g, dtype=torch.float64)
    joints = [(0.1 * torch.randn(B, J, 3, generator=g) + torch.tensor([0.2, -0.1, 0.8])) for _ in range(2)]
    return kp_full.float(), (2.0 * px / IMG_RES - 1.0).float(), joints[0], joints[1], t_true.float()


def case_inputs(case, B=SI.FIXTURE_B, lengths=None, seed=None):
    """(targets, meta_info) in fp32 on the CPU, as the dataset hands them to arctic_pre_process."""
    seed = CASES[case] if seed is None else seed
    g = torch.Generator().manual_seed(seed + 5)
    objects = [SI.OBJECTS[3]] * B if case == "one_object" else None
    _, gt, meta = SI.case_inputs(case if case in SI.CASES else "all_valid", B=B, seed=seed, objects=objects)
    ot = SI.obj_arrays(lengths=lengths)
    idx = torch.tensor([SI.OBJECTS.index(n) for n in meta["query_names"]])
    max_len = int(ot["v_len"][idx].max())
    o = object_tensors_reference(ot, gt["object.radian"].view(-1, 1), gt["object.rot"], None, idx, max_len)
    kp_cano = o["kp3d"][:, o["kp3d"].shape[1] // 2:]
    targets = {k: gt[k] for k in ("mano.pose.r", "mano.beta.r", "mano.pose.l", "mano.beta.l", "object.rot", "object.radian",
                                   "is_valid", "left_valid", "right_valid")}
    (targets["object.kp3d.full.b"], targets["object.kp2d.norm.b"], targets["mano.j3d.full.r"], targets["mano.j3d.full.l"],
     _) = fit_inputs(kp_cano, meta["intrinsics"], g)
    return targets, dict(meta)


def kp_cano_of(targets, meta, lengths=None):
    ot = SI.obj_arrays(lengths=lengths)
    idx = torch.tensor([SI.OBJECTS.index(n) for n in meta["query_names"]])
    o = object_tensors_reference(ot, targets["object.radian"].view(-1, 1), targets["object.rot"], None, idx, int(ot["v_len"][idx].max()))
    return o["kp3d"][:, o["kp3d"].shape[1] // 2:]


def fit_conditioning(kp_full, kp_cano):
    """fp64, from the data alone: (det of V U^T, s1 / s0, s2 / s0) per frame of H = sum (a - mean a)(b - mean b)^T."""
    a, b = kp_full.double(), kp_cano.double()
    H = (a - a.mean(1, keepdim=True)).transpose(1, 2) @ (b - b.mean(1, keepdim=True))
    U, S, Vh = torch.linalg.svd(H)
    return torch.linalg.det(Vh.transpose(1, 2) @ U.transpose(1, 2)), S[:, 1] / S[:, 0], S[:, 2] / S[:, 0]


def check_case(targets, meta, lengths=None):
    det, r1, r2 = fit_conditioning(targets["object.kp3d.full.b"], kp_cano_of(targets, meta, lengths))
    assert (det > 0).all(), det
    assert (r2 > MIN_RATIO).all() and (r1 > MIN_RATIO).all(), (r1, r2)
    return float(r1.min()), float(r2.min())


def mirrored(kp_full):
    return kp_full * torch.tensor([1.0, 1.0, -1.0])


def collinear(kp_cano, g):
    """(kp_full, kp_cano) on one line each: no unique rotation."""
    B, NK, _ = kp_cano.shape
    s = torch.randn(B, NK, 1, generator=g)
    return s * torch.tensor([0.05, 0.02, -0.03]), s * torch.tensor([0.01, 0.06, 0.02])


def df_inputs(seed, B, NV, L):
    """(hand_r, hand_l, obj) camera-space clouds in fp32, shaped as arctic_eval_inputs.nn_inputs' (object 0.15 m, hands 0.06 m)."""
    (obj, hand_r), = EI.nn_inputs(seed, B, L, NV, pairs=1)
    g = torch.Generator().manual_seed(seed + 1)
    hand_l = hand_r + 0.04 * torch.randn(B, 1, 3, generator=g) + 0.01 * torch.randn(B, NV, 3, generator=g)
    return hand_r, hand_l.float(), obj


def df_lengths(L):
    """Per-frame v_len values of a B = 3 test at object length L: 1, L and both sides of every LDS chunk boundary below L."""
    vals = [1, L]
    for c in range(DF_CHUNK, L + 1, DF_CHUNK):
        vals += [c - 1, c, c + 1]
    vals = sorted({v for v in vals if 1 <= v <= L})
    return [vals[i:i + 3] + [vals[-1]] * (3 - len(vals[i:i + 3])) for i in range(0, len(vals), 3)]


def df_yardstick(hand_r, hand_l, obj, v_len):
    """fp64 brute force per field, on the clouds' device: {field: (argmin index, distance, relative gap of the two smallest
    squared distances, mask of the rows that search)} with the length rule applied to the candidates."""
    B, L, _ = obj.shape
    dev = obj.device
    v_len = v_len.to(dev).clamp(0, L)
    o = obj.double()
    out = {}
    for s, hand in (("r", hand_r.double()), ("l", hand_l.double())):
        for name, src, trg, n_trg in (("%so" % s, hand, o, v_len), ("o%s" % s, o, hand, torch.full_like(v_len, hand.shape[1]))):
            N2 = trg.shape[1]
            ar = torch.arange(N2, device=dev)
            first, best, gap = [], [], []
            for b in range(B):                                  # one frame at a time: [N1, N2] fp64
                d = ((src[b, :, None, :] - trg[b, None, :, :]) ** 2).sum(-1)
                d = torch.where(ar[None, :] >= n_trg[b], torch.full_like(d, float("inf")), d)
                if N2 > 1:
                    two = torch.topk(d, 2, dim=1, largest=False).values
                    g = (two[:, 1] - two[:, 0]) / two[:, 1].clamp(min=1e-300)
                    gap.append(torch.where(torch.isfinite(two[:, 1]), g, torch.ones_like(g)))
                else:
                    gap.append(torch.ones_like(d[:, 0]))
                m = d.min(dim=1).values
                first.append(torch.where(d == m[:, None], ar, N2).min(dim=1).values)
                best.append(m.sqrt())
            first = torch.stack(first)
            searches = (v_len > 0)[:, None].expand_as(first) if name.endswith("o") \
                else torch.arange(L, device=dev)[None, :] < v_len[:, None]
            out[name] = (first, torch.stack(best), torch.stack(gap), searches)
    return out


def assert_fields(fields, hand_r, hand_l, obj, v_len, dist_min=0.0, dist_max=float("inf")):
    """``fields`` (dist.* / idx.* of distance_fields or of a finished step) against fp64 brute force on the same clouds: the
    index equals the fp64 argmin except where the two nearest squared distances lie within 2^-20 relative (at most 1e-3 of the
    searching rows); the distance is within 6 x 2^-24 relative of the fp64 distance at the returned index (the squared
    distance is granted 8 by tests/test_arctic_eval_gpu.py; the root halves that and adds one rounding of its own, counted
    as 2); rows that do not search hold exactly clamp(0) and index 0.  Returns (rows left out, rows that search)."""
    clouds = {"r": hand_r, "l": hand_l, "o": obj}
    skipped = total = 0
    for name, (first, dist, gap, searches) in df_yardstick(hand_r, hand_l, obj, v_len).items():
        idx, got = fields["idx." + name], fields["dist." + name]
        assert idx.dtype == torch.int64 and got.dtype == torch.float32 and idx.shape == first.shape == got.shape, name
        hard = (gap < NEAR_TIE) & searches
        skipped, total = skipped + int(hard.sum()), total + int(searches.sum())
        ok = searches & ~hard
        assert torch.equal(idx[ok], first[ok]), name
        rest = torch.zeros((), dtype=torch.float32).clamp(dist_min, dist_max).item()
        assert (idx[~searches] == 0).all() and (got[~searches] == rest).all(), name
        src, trg = clouds[name[0]].double(), clouds[name[1]].double()
        at = (src - torch.gather(trg, 1, idx[..., None].expand(-1, -1, 3))).norm(dim=2).clamp(dist_min, dist_max)
        assert ((got.double() - at).abs()[searches] <= 6 * 2.0 ** -24 * at[searches]).all(), name
    assert skipped <= NEAR_TIE_SHARE * total, (skipped, total)
    return skipped, total


def assert_matches_fixture(z, case, targets, meta, device_type="cpu", tol=2e-4):
    """A finished step against pre_process.npz: keys and their order, dtypes and shapes exactly; the stored values within
    ``tol`` relative to the key's largest value (integers exactly).  Returns the number of values compared."""
    assert list(targets.keys()) == list(z[case + "/targets_keys"])
    assert list(meta.keys()) == list(z[case + "/meta_keys"]) + ["fit_status"]
    seen = 0
    for where, d in (("targets/", targets), ("meta/", meta)):
        for k, v in d.items():
            name = "%s/dtype/%s%s" % (case, where, k)
            if name not in z:
                assert not torch.is_tensor(v) or k == "fit_status", k
                continue
            if torch.is_tensor(v):
                assert v.device.type == device_type, k
                v = v.detach().cpu().numpy()
            assert str(v.dtype) == str(z[name]) and tuple(v.shape) == tuple(z["%s/shape/%s%s" % (case, where, k)]), k
            data = "%s/data/%s%s" % (case, where, k)
            if data not in z:
                continue
            seen += 1
            if z[data].dtype.kind == "f":
                err = float(abs(v.astype("float64") - z[data]).max() / abs(z[data]).max())
                assert err < tol, (k, err)
            else:
                assert (v == z[data]).all(), k
    return seen


FIT_FIXTURE_KEYS = {"transl": "object.cam_t", "j3d_cam_r": "mano.j3d.cam.r", "j3d_cam_l": "mano.j3d.cam.l", "cam_t_r": "mano.cam_t.r",
                    "cam_t_l": "mano.cam_t.l", "cam_t_wp_r": "mano.cam_t.wp.r", "cam_t_wp_l": "mano.cam_t.wp.l",
                    "cam_t_wp_o": "object.cam_t.wp"}


def fit_call_inputs(targets, meta, models, lengths=None):
    """The eight tensors fit_targets takes for a case, in fp32: the canonical keypoints and joints come from the torch
    restatements of the object and MANO layers."""
    from uvhand_amd.mano import mano_many
    pr, pl = targets["mano.pose.r"], targets["mano.pose.l"]
    with torch.no_grad():
        hr, hl = mano_many([(models["mano_r"], targets["mano.beta.r"], pr[:, :3], pr[:, 3:]),
                            (models["mano_l"], targets["mano.beta.l"], pl[:, :3], pl[:, 3:])])
    return [targets["object.kp3d.full.b"], kp_cano_of(targets, meta, lengths), targets["object.kp2d.norm.b"], meta["intrinsics"],
            targets["mano.j3d.full.r"], targets["mano.j3d.full.l"], hr.joints, hl.joints]


def fixture_deviation(z, models, fit_reference):
    """Per fit output that process_data stores: the largest deviation, over the fixture cases, of the reference-run fp32
    fixture from the fp64 restatement on the same fp32 inputs, relative to the output's largest value."""
    dev = {k: 0.0 for k in FIT_FIXTURE_KEYS}
    for case in CASES:
        targets, meta = case_inputs(case)
        out, _ = fit_reference(*[t.double() for t in fit_call_inputs(targets, meta, models)])
        for k, fk in FIT_FIXTURE_KEYS.items():
            name = "%s/data/targets/%s" % (case, fk)
            if name in z:
                ref, got = out[k].numpy(), z[name].astype("float64")
                dev[k] = max(dev[k], float(abs(got - ref).max() / abs(ref).max()))
    return dev
