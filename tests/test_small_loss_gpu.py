"""ARCTIC small losses and object layer on the MI355X (csrc/msda_small_loss.hip).

Tolerances.  Fixture parity (the fp32 reference, fp32 kernels): 2e-4 relative, as the CPU restatement.  At realistic size
(6 sets, 32 frames, a padded object of 4000 rows) against the fp64 restatement: values 1e-4 relative; gradients 1e-3 relative
(the fp32 projection divides by z of order 10, and the smoothing sum has 4000 x 3 terms per frame pair whose L1 gradient
is a sign: an fp32 rounding that flips the sign of a near-zero difference moves that element's gradient by 2 g)."""
import sys
import types

import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import mano_inputs as MI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd.mano import MANO  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors, object_tensors_reference, objects_many  # noqa: E402
from uvhand_amd.small_loss import KEYS, ArcticSmallLoss, small_loss_many, small_loss_reference  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def models(lengths=None):
    return {"mano_l": MANO.from_arrays(**MI.model_arrays("left", dtype=torch.float32), is_rhand=False).to(DEV),
            "mano_r": MANO.from_arrays(**MI.model_arrays("right", dtype=torch.float32)).to(DEV),
            "arti_head": ObjectTensors.from_arrays(SI.obj_arrays(lengths=lengths)).to(DEV)}


def _dev(pred, gt, meta):
    pred = [[t.to(DEV) for t in grp] for grp in pred]
    gt = {k: v.to(DEV) for k, v in gt.items()}
    meta = dict(meta, intrinsics=meta["intrinsics"].to(DEV))
    return pred, gt, meta


def _leaves(pred):
    return SI.unflat_pred([t.detach().clone().requires_grad_(True) for t in SI.flat_pred(pred)])


def _run(preds, gt, meta, m, w):
    preds = [_leaves(p) for p in preds]
    ds = small_loss_many(preds, gt, meta, m, SI.IMG_RES)
    total = sum(w[i] * d[k].sum() for d in ds for i, k in enumerate(KEYS))
    total.backward()
    return ds, [[t.grad if t.grad is not None else torch.zeros_like(t) for t in SI.flat_pred(p)] for p in preds]


def _case(z, case):
    pred = SI.unflat_pred([torch.from_numpy(z["%s/pred/%s" % (case, n)]) for n in SI.PRED_NAMES])
    gt = {k.split("/", 2)[2]: torch.from_numpy(z[k]) for k in z if k.startswith(case + "/gt/")}
    meta = {"intrinsics": torch.from_numpy(z[case + "/K"]), "query_names": [SI.OBJECTS[i] for i in z[case + "/obj_idx"]]}
    return _dev(pred, gt, meta)


@pytest.mark.parametrize("case", list(SI.CASES))
def test_fixture_parity(case):
    z = load_golden("small_loss")
    pred, gt, meta = _case(z, case)
    w = SI.upstream(SI.CASES[case] + 100).to(DEV)
    (d,), (g,) = _run([pred], gt, meta, models(), w)
    assert list(d) == list(KEYS)
    for k in KEYS:
        ref = z["%s/loss/%s" % (case, k)]
        # the one deviation: a skipped hand block gives [1] zeros where the reference gives 0-d ones
        assert tuple(d[k].shape) == (() if k in ("loss/object/v3d_smoothing", "loss/cd") else (1,)), k
        assert rel_err(d[k].detach().double().cpu().numpy().reshape(ref.shape), ref) < 2e-4, (k, d[k], ref)
    for name, t in zip(SI.PRED_NAMES, g):
        assert rel_err(t.double().cpu().numpy(), z["%s/grad/%s" % (case, name)]) < 2e-4, name


def test_object_layer_parity_and_grad():
    ot = ObjectTensors.from_arrays(SI.obj_arrays()).to(DEV)
    g = torch.Generator().manual_seed(9)
    names = [SI.OBJECTS[i] for i in torch.randint(0, 11, (16,), generator=g)]
    ang = (torch.rand(16, 1, generator=g)).to(DEV).requires_grad_(True)
    go = (0.8 * torch.randn(16, 3, generator=g)).to(DEV).requires_grad_(True)
    tr = (0.1 * torch.randn(16, 3, generator=g)).to(DEV).requires_grad_(True)
    out = ot(ang, go, tr, names)
    idx, max_len = ot.obj_index(names)
    ref = object_tensors_reference(ot.obj_tensors, ang.double(), go.double(), tr.double(), idx, max_len)
    ws = {k: torch.randn(out[k].shape, generator=g).to(DEV) for k in ("v", "v_sub", "bbox3d", "kp3d")}
    sum((out[k] * ws[k]).sum() for k in ws).backward()
    got = [t.grad.clone() for t in (ang, go, tr)]
    for t in (ang, go, tr):
        t.grad = None
    sum((ref[k] * ws[k].double()).sum() for k in ws).backward()
    for k in ws:
        assert rel_err(out[k].detach().double().cpu().numpy(), ref[k].detach().cpu().numpy()) < 1e-5, k
    for a, t in zip(got, (ang, go, tr)):
        assert rel_err(a.double().cpu().numpy(), t.grad.cpu().numpy()) < 1e-4


def _big(seed=21, S=6, B=32, L=4000):
    """A window-32 step: 6 sets sharing targets, objects padded to about 4000 rows."""
    lengths = [L - 37 * i for i in range(11)]
    pred, gt, meta = SI.case_inputs("partial", B=B, seed=seed, obj_seed=1400)
    g = torch.Generator().manual_seed(seed + 1)
    gt["idx.ro"] = torch.randint(0, L - 400, gt["idx.ro"].shape, generator=g)
    gt["idx.lo"] = torch.randint(0, L - 400, gt["idx.lo"].shape, generator=g)
    gt["idx.ro"][:, :40] = 7                                     # many hand vertices on one object vertex
    gt["dist.ro"][:, :40] = 1e-3
    preds = [pred]
    for s in range(1, S):
        p, _, _ = SI.case_inputs("partial", B=B, seed=seed + 10 * s, objects=meta["query_names"])
        preds.append(p)
    preds = [_dev(p, gt, meta)[0] for p in preds]
    _, gt, meta = _dev(pred, gt, meta)
    return preds, gt, meta, models(lengths)


def test_realistic_size_against_fp64():
    preds, gt, meta, m = _big()
    w = SI.upstream(7).to(DEV)
    ds, gs = _run(preds, gt, meta, m, w)
    for p, d, g in zip(preds, ds, gs):
        leaves = [t.detach().double().requires_grad_(True) for t in SI.flat_pred(p)]
        r = small_loss_reference(SI.unflat_pred(leaves), gt, meta, m, SI.IMG_RES, dtype=torch.float64)
        sum(w[i].double() * r[k].sum() for i, k in enumerate(KEYS)).backward()
        for k in KEYS:
            assert rel_err(d[k].detach().double().cpu().numpy(), r[k].detach().reshape(d[k].shape).cpu().numpy()) < 1e-4, k
        for name, a, leaf in zip(SI.PRED_NAMES, g, leaves):
            ref = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            assert rel_err(a.double().cpu().numpy(), ref.cpu().numpy()) < 1e-3, name


def test_grouped_equals_per_set_and_runs_are_bitwise():
    preds, gt, meta, m = _big()
    w = SI.upstream(8).to(DEV)
    d1, g1 = _run(preds, gt, meta, m, w)
    d2, g2 = _run(preds, gt, meta, m, w)
    for s, p in enumerate(preds):
        (d3,), (g3,) = _run([p], gt, meta, m, w)
        for k in KEYS:
            assert torch.equal(d1[s][k], d2[s][k]) and torch.equal(d1[s][k], d3[k]), k
        for a, b, c in zip(g1[s], g2[s], g3):
            assert torch.equal(a, b) and torch.equal(a, c)


def test_no_host_sync_with_obj_idx():
    preds, gt, meta, m = _big()
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    meta = dict(meta, obj_idx=idx, max_len=max_len)
    w = SI.upstream(9).to(DEV)
    _run(preds, gt, meta, m, w)                      # warm-up: conversions, library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run(preds, gt, meta, m, w)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_launch_counts():
    from torch.profiler import ProfilerActivity, profile

    preds, gt, meta, m = _big()
    w = SI.upstream(10).to(DEV)
    _run(preds, gt, meta, m, w)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _run(preds, gt, meta, m, w)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert count("sl_part_kernel") == 1 and count("sl_final_kernel") == 1 and count("sl_bwd_kernel") == 1
    assert count("obj_fwd_kernel") == 1 and count("obj_bwd_kernel") == 1
    assert count("mano_fwd_kernel") == 1


def test_graph_capture_matches_eager():
    preds, gt, meta, m = _big(S=2, B=8)
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    meta = dict(meta, obj_idx=idx, max_len=max_len)
    w = SI.upstream(11).to(DEV)
    leaves = [_leaves(p) for p in preds]
    flat = [t for p in leaves for t in SI.flat_pred(p)]

    def step():
        ds = small_loss_many(leaves, gt, meta, m, SI.IMG_RES)
        total = sum(w[i] * d[k].sum() for d in ds for i, k in enumerate(KEYS))
        return torch.autograd.grad(total, flat, allow_unused=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        if a is None:
            assert b is None
        else:
            assert torch.equal(a, b)


@pytest.mark.parametrize("trigger", ["env", "fp64", "autocast", "limits"])
def test_fallbacks_give_the_restatement(trigger, monkeypatch):
    pred, gt, meta = _dev(*SI.case_inputs("partial"))
    m = models()
    if trigger == "env":
        monkeypatch.setenv("MSDA_SMALL_LOSS_FUSED", "0")
    if trigger == "fp64":
        pred = [[t.double() for t in grp] for grp in pred]
    preds = [pred] * (9 if trigger == "limits" else 1)
    if trigger == "autocast":
        with torch.autocast("cuda", dtype=torch.bfloat16):
            d = small_loss_many(preds, gt, meta, m, SI.IMG_RES)[0]
            r = small_loss_reference(pred, gt, meta, m, SI.IMG_RES)
    else:
        d = small_loss_many(preds, gt, meta, m, SI.IMG_RES)[0]
        r = small_loss_reference(pred, gt, meta, m, SI.IMG_RES)
    assert list(d) == list(KEYS)
    for k in KEYS:
        assert torch.equal(d[k], r[k]), k


def test_object_fallback_env(monkeypatch):
    ot = ObjectTensors.from_arrays(SI.obj_arrays()).to(DEV)
    names = ["box", "laptop"]
    ang, go = torch.rand(2, 1, device=DEV), torch.randn(2, 3, device=DEV)
    idx, L = ot.obj_index(names)
    monkeypatch.setenv("MSDA_OBJECT_FUSED", "0")
    a = objects_many([(ot, ang, go, None, idx, L)])[0]
    r = object_tensors_reference(ot.obj_tensors, ang, go, None, idx, L)
    assert all(torch.equal(a[k], r[k]) for k in a)


def test_criterion_step_without_host_sync():
    import criterion_inputs as CI
    from uvhand_amd.criterion import SetArcticCriterion
    from uvhand_amd.matcher import ArcticMatcher

    outputs, targets, _ = CI.arctic_case("full", 3)
    bs, Q = outputs["pred_logits"].shape[:2]
    outputs, targets = CI.to_device(outputs, targets, DEV, True)
    g = torch.Generator().manual_seed(12)
    leaf = lambda t: t.to(DEV).requires_grad_(True)  # noqa: E731
    for o in [outputs] + outputs["aux_outputs"]:
        o["pred_cams"] = [leaf(torch.randn(bs, Q, 3, generator=g) * 0.1 + 0.5), leaf(torch.randn(bs, Q, 3, generator=g) * 0.1 + 0.5)]
        o["pred_mano_params"] = [leaf(torch.randn(bs, Q, 48, generator=g) * 0.3), leaf(torch.randn(bs, Q, 10, generator=g))]
        o["pred_obj_params"] = [leaf(torch.rand(bs, Q, 1, generator=g)), leaf(torch.randn(bs, Q, 3, generator=g) * 0.3)]
    _, gt, meta = _dev(*SI.case_inputs("partial", B=bs, seed=13))
    gt["is_valid"] = targets["is_valid"]
    targets = dict(gt, **targets)
    m = models()
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    meta = dict(meta, obj_idx=idx, max_len=max_len)
    cfg = types.SimpleNamespace(hand_idx=[12, 13])
    args = types.SimpleNamespace(img_res=SI.IMG_RES, device=DEV)
    crit = SetArcticCriterion(CI.ARCTIC_K, ArcticMatcher(CI.COST_CLASS, CI.COST_KEYPOINT), {}, ["labels", "cardinality"],
                              focal_alpha=CI.FOCAL_ALPHA, cfg=cfg, small_loss=ArcticSmallLoss(m, cfg))
    sum(v.sum() for v in crit(outputs, targets, args, meta).values()).backward()          # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = crit(outputs, targets, args, meta)
        sum(v.sum() for v in losses.values()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert [k for k in losses if k.startswith("loss/")][:19] == list(KEYS)
