"""ARCTIC small losses and object layer on the CPU: the torch restatements against the fixtures of the reference's own
compute_small_loss / ObjectTensors (gen_golden_r14.py), key order, the pinned reference behaviours, ``from_reference`` and the
criterion hook.  Tolerances: the restatement in fp64 against the fp32 reference: 2e-4 relative on values and gradients (the
reference's fp32 rounding, the projection divides by z of order 10); the fp32 restatement matches to the same bound."""
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import mano_inputs as MI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd.mano import MANO  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors, axis_angle_to_quaternion, object_tensors_reference  # noqa: E402
from uvhand_amd.small_loss import KEYS, ArcticSmallLoss, compute_small_loss, small_loss_reference  # noqa: E402

TOL = 2e-4


def models(dtype=torch.float32):
    return {"mano_l": MANO.from_arrays(**MI.model_arrays("left", dtype=torch.float32), is_rhand=False),
            "mano_r": MANO.from_arrays(**MI.model_arrays("right", dtype=torch.float32)),
            "arti_head": ObjectTensors.from_arrays(SI.obj_arrays())}


def _case(z, case, dtype):
    pred = [torch.from_numpy(z["%s/pred/%s" % (case, n)]).to(dtype).requires_grad_(True) for n in SI.PRED_NAMES]
    gt = {k.split("/", 2)[2]: torch.from_numpy(z[k]) for k in z if k.startswith(case + "/gt/")}
    meta = {"intrinsics": torch.from_numpy(z[case + "/K"]), "query_names": [SI.OBJECTS[i] for i in z[case + "/obj_idx"]]}
    return pred, gt, meta


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", list(SI.CASES))
def test_restatement_matches_reference(case, dtype):
    z = load_golden("small_loss")
    pred, gt, meta = _case(z, case, dtype)
    d = small_loss_reference(SI.unflat_pred(pred), gt, meta, models(), SI.IMG_RES, dtype=dtype)
    assert list(d) == list(z[case + "/keys"]) == list(KEYS)
    for k in KEYS:
        ref = z["%s/loss/%s" % (case, k)]
        assert d[k].shape == ref.shape, k
        assert rel_err(d[k].detach().double().numpy(), ref) < TOL, (k, d[k], ref)
    w = SI.upstream(SI.CASES[case] + 100).to(dtype)
    sum(w[i] * d[k].sum() for i, k in enumerate(KEYS)).backward()
    for name, leaf in zip(SI.PRED_NAMES, pred):
        g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        assert rel_err(g.double().numpy(), z["%s/grad/%s" % (case, name)]) < TOL, name


def test_object_restatement_matches_reference():
    z = load_golden("small_loss")
    pred, _, meta = _case(z, "all_valid", torch.float64)
    out = models()["arti_head"].forward(pred[8].view(-1, 1), pred[7], None, meta["query_names"])
    assert list(out) == list(z["object/keys"])
    for k, v in out.items():
        ref = z["object/" + k]
        assert tuple(v.shape) == ref.shape, k
        assert rel_err(v.detach().double().numpy(), ref.astype(np.float64)) < 1e-5, k


def test_compute_small_loss_cpu_is_the_restatement():
    pred, gt, meta = SI.case_inputs("partial")
    a = compute_small_loss(pred, gt, meta, models(), SI.IMG_RES)
    b = small_loss_reference(pred, gt, meta, models(), SI.IMG_RES)
    assert list(a) == list(b) == list(KEYS)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def test_pinned_behaviours():
    pred, gt, meta = SI.case_inputs("partial")
    # a 0.5 flag counts as invalid in vector_loss: cam_t/l is the mean over frames with left_valid == 1 only
    rl = pred[0][0].double()
    keep = gt["left_valid"].long().bool()
    want = ((rl - gt["mano.cam_t.wp.l"].double()) ** 2)[keep].mean()
    d = small_loss_reference(pred, gt, meta, models(), SI.IMG_RES, dtype=torch.float64)
    assert torch.allclose(d["loss/mano/cam_t/l"], want.view(-1))
    # s below min_s = 0.1: zero gradient into s
    pred, gt, meta = SI.case_inputs("small_s")
    leaves = [t.clone().requires_grad_(True) for t in SI.flat_pred(pred)]
    d = small_loss_reference(SI.unflat_pred(leaves), gt, meta, models(), SI.IMG_RES, dtype=torch.float64)
    (d["loss/object/kp2d"].sum() + d["loss/object/v3d_smoothing"]).backward()      # root_o reaches these through cam_t only
    assert (leaves[2].grad[::2, 0] == 0).all() and (leaves[2].grad[1::2, 0] != 0).all()
    # no contact within 3 mm: loss/cd is 0-d zero with a zero gradient; skipped blocks are [1] zeros
    pred, gt, meta = SI.case_inputs("no_contact")
    d = small_loss_reference(pred, gt, meta, models(), SI.IMG_RES)
    assert d["loss/cd"].shape == () and float(d["loss/cd"]) == 0.0
    pred, gt, meta = SI.case_inputs("left_invalid")
    d = small_loss_reference(pred, gt, meta, models(), SI.IMG_RES)
    assert all(float(d[k]) == 0.0 for k in KEYS[:5]) and float(d["loss/mano/transl/l"]) == 0.0


def test_quaternion_small_angle_series():
    a = torch.tensor([[0.0, 0.0, 0.0], [3e-7, 0.0, 0.0], [0.5, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    q = axis_angle_to_quaternion(a)
    assert torch.allclose(q[1, 1], torch.tensor(3e-7 * (0.5 - 9e-14 / 48), dtype=torch.float64))
    q.sum().backward()
    assert torch.isfinite(a.grad).all()


def test_object_max_len_and_obj_idx():
    ot = ObjectTensors.from_arrays(SI.obj_arrays())
    names = ["box", "phone", "box"]
    idx, max_len = ot.obj_index(names)
    assert max_len == max(int(ot.obj_tensors["v_len"][SI.OBJECTS.index(n)]) for n in names)
    go, ang = 0.3 * torch.randn(3, 3), torch.rand(3, 1)
    a = ot(ang, go, None, names)
    b = ot(ang, go, None, None, obj_idx=idx, max_len=max_len)
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        ot(ang, go, None, None, obj_idx=idx)
    with pytest.raises(ValueError):
        ot.obj_index(["not-an-object"])
    t = ot(ang, go, 0.01 * torch.ones(3, 3), names)            # transl in metres
    assert torch.allclose(t["v"] - a["v"], torch.full_like(a["v"], 0.01), atol=1e-6)
    tmpl = ot.forward_template(names)
    assert list(tmpl) == ["diameter", "f", "f_len", "v_len", "v", "mask", "v_sub", "parts_ids", "parts_sub_ids"]
    r = object_tensors_reference(ot.obj_tensors, ang, go, None, idx, max_len)
    assert all(torch.equal(a[k], r[k]) for k in a)


def test_from_reference_copies_obj_tensors():
    src = types.SimpleNamespace(obj_tensors=SI.obj_arrays(), dev=None)
    ot = ObjectTensors.from_reference(src)
    for k, v in src.obj_tensors.items():
        if torch.is_tensor(v):
            assert torch.equal(ot.obj_tensors[k], v), k
    assert ot.obj_tensors["names"] == SI.OBJECTS


def _outputs(g, B, Q=8, K=14):
    return {"pred_logits": torch.randn(B, Q, K, generator=g), "pred_cams": [torch.randn(B, Q, 3, generator=g) * 0.1 + 0.5,
                                                                            torch.randn(B, Q, 3, generator=g) * 0.1 + 0.5],
            "pred_mano_params": [torch.randn(B, Q, 48, generator=g) * 0.3, torch.randn(B, Q, 10, generator=g)],
            "pred_obj_params": [torch.rand(B, Q, 1, generator=g), torch.randn(B, Q, 3, generator=g) * 0.3]}


def test_many_equals_per_set_calls():
    g = torch.Generator().manual_seed(5)
    _, gt, meta = SI.case_inputs("partial")
    sets = [_outputs(g, SI.FIXTURE_B) for _ in range(3)]
    cfg = types.SimpleNamespace(hand_idx=[12, 13])
    args = types.SimpleNamespace(img_res=SI.IMG_RES, device="cpu")
    sl = ArcticSmallLoss(models(), cfg)
    many = sl.many(sets, gt, meta, args, ["", "_0", "_1"])
    for d, o, sfx in zip(many, sets, ["", "_0", "_1"]):
        one = sl(o, gt, meta, args, sfx)
        assert list(d) == list(one) == [k + sfx for k in KEYS]
        assert all(torch.equal(d[k], one[k]) for k in d)


def test_criterion_hook_keeps_key_order():
    from uvhand_amd.criterion import SetArcticCriterion

    g = torch.Generator().manual_seed(6)
    _, gt, meta = SI.case_inputs("all_valid")
    B = SI.FIXTURE_B
    final = _outputs(g, B)
    final["aux_outputs"] = [_outputs(g, B) for _ in range(2)]
    targets = dict(gt, labels=[torch.tensor([1, 12, 13]) for _ in range(B)])
    cfg = types.SimpleNamespace(hand_idx=[12, 13])
    args = types.SimpleNamespace(img_res=SI.IMG_RES, device="cpu")
    matcher = types.SimpleNamespace(cost_class=2.0, cost_keypoint=5.0)
    matcher.__call__ = None
    sl = ArcticSmallLoss(models(), cfg)
    calls = []

    def per_set(o, t, m, a, sfx):
        calls.append(sfx)
        return sl(o, t, m, a, sfx)

    c_many = SetArcticCriterion(14, matcher, {}, [], cfg=cfg, small_loss=sl)
    c_one = SetArcticCriterion(14, matcher, {}, [], cfg=cfg, small_loss=per_set)
    from uvhand_amd import criterion as C
    orig = C.arctic_set_losses
    C.arctic_set_losses = lambda *a, **k: {"loss_ce": torch.zeros(())}
    try:
        matcher_fn = lambda o, t: None  # noqa: E731
        c_many.matcher = c_one.matcher = matcher_fn
        a = c_many._forward_reference(final, targets, args, meta)
        b = c_one._forward_reference(final, targets, args, meta)
    finally:
        C.arctic_set_losses = orig
    assert calls == ["", "_0", "_1"]
    assert list(a) == list(b)
    assert all(torch.equal(a[k], b[k]) for k in a)
