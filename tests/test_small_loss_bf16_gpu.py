"""The ARCTIC small losses under bf16 autocast with MSDA_SMALL_LOSS_BF16=1, on the MI355X.

No tolerance: the nodes call the C ABI on fp32 tensors, so a bf16 autocast region changes none of their bits, and the grouped
selection widens bf16 predictions exactly.  Every claim is equality with the fp32 route outside autocast, which
tests/test_small_loss*_gpu.py and tests/test_mano*_gpu.py hold to fp64."""
import sys
import types

import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import criterion_inputs as CI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from test_small_loss_gpu import _big, _case, _dev, _leaves, models  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.mano import mano_many  # noqa: E402
from uvhand_amd.object_tensors import objects_many  # noqa: E402
from uvhand_amd.small_loss import KEYS, ArcticSmallLoss, small_loss_many  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KNOB = "MSDA_SMALL_LOSS_BF16"
BF16, FP16 = torch.bfloat16, torch.float16
SOURCES = ("pred_cams", "pred_mano_params", "pred_obj_params")


class _Region:
    """torch.autocast("cuda", dtype) or, for dtype None, no region."""

    def __init__(self, dtype):
        self.ctx = torch.autocast("cuda", dtype=dtype) if dtype is not None else None

    def __enter__(self):
        return self.ctx.__enter__() if self.ctx is not None else None

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc) if self.ctx is not None else False


def _inputs(case):
    if case == "big":
        return _big(S=2, B=8)
    pred, gt, meta = _case(load_golden("small_loss"), case)
    return [pred], gt, meta, models()


# ---- the three nodes on fp32 inputs ---------------------------------------------------------------------------------------------
def _loss_node(preds, gt, meta, m, amp):
    """(values, gradients, library launches) of small_loss_many + backward on fresh leaves."""
    w = SI.upstream(31).to(DEV)
    leaves = [_leaves(p) for p in preds]
    n0 = _native.launch_count()
    with _Region(amp):
        ds = small_loss_many(leaves, gt, meta, m, SI.IMG_RES)
        total = sum(w[i] * d[k].sum() for d in ds for i, k in enumerate(KEYS))
    total.backward()
    grads = [t.grad for p in leaves for t in SI.flat_pred(p)]
    return [d[k] for d in ds for k in KEYS], grads, _native.launch_count() - n0


def _mano_node(preds, gt, meta, m, amp):
    leaves = [_leaves(p) for p in preds]
    calls = []
    for (_, pose, shape, _) in leaves:
        calls.append((m["mano_l"], shape[0], pose[0][:, :3], pose[0][:, 3:]))
        calls.append((m["mano_r"], shape[1], pose[1][:, :3], pose[1][:, 3:]))
    n0 = _native.launch_count()
    with _Region(amp):
        outs = mano_many(calls)
    vals = [t for o in outs for t in (o.vertices, o.joints)]
    g = torch.Generator().manual_seed(32)
    sum((v * torch.randn(v.shape, generator=g).to(DEV)).sum() for v in vals).backward()
    grads = [t.grad for p in leaves for t in (p[1][0], p[1][1], p[2][0], p[2][1])]
    return vals, grads, _native.launch_count() - n0


def _object_node(preds, gt, meta, m, amp):
    leaves = [_leaves(p) for p in preds]
    obj = m["arti_head"]
    idx, max_len = obj.obj_index(meta["query_names"])
    n0 = _native.launch_count()
    with _Region(amp):
        outs = objects_many([(obj, p[3][1].view(-1, 1), p[3][0].reshape(-1, 3), None, idx, max_len) for p in leaves])
    vals = [o[k] for o in outs for k in ("v", "v_sub", "bbox3d", "kp3d")]
    g = torch.Generator().manual_seed(33)
    sum((v * torch.randn(v.shape, generator=g).to(DEV)).sum() for v in vals).backward()
    grads = [t.grad for p in leaves for t in p[3]]
    return vals, grads, _native.launch_count() - n0


NODES = {"small_loss_many": _loss_node, "mano_many": _mano_node, "objects_many": _object_node}


@pytest.mark.parametrize("case", list(SI.CASES) + ["big"])
@pytest.mark.parametrize("node", list(NODES))
def test_node_under_bf16_autocast_is_bitwise_the_fp32_route(node, case, monkeypatch):
    args = _inputs(case)
    monkeypatch.delenv(KNOB, raising=False)
    vals, grads, n = NODES[node](*args, None)
    assert n > 0
    monkeypatch.setenv(KNOB, "1")
    vals_amp, grads_amp, n_amp = NODES[node](*args, BF16)
    assert n_amp == n                                                    # fails without the knob's route: 0 launches
    for a, b in zip(vals, vals_amp):
        assert b.dtype == torch.float32 and torch.equal(a, b)
    for a, b in zip(grads, grads_amp):
        assert (a is None and b is None) or (b.dtype == torch.float32 and torch.equal(a, b))


@pytest.mark.parametrize("node", list(NODES))
@pytest.mark.parametrize("knob, amp", [("0", BF16), (None, BF16), ("1", FP16)])
def test_node_keeps_the_restatement(node, knob, amp, monkeypatch):
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, knob)
    assert NODES[node](*_inputs("partial"), amp)[2] == 0


# ---- the criterion step ---------------------------------------------------------------------------------------------------------
def _attach_sources(sets, bs, Q, dtype, seed=12):
    """bf16-valued pred_cams / pred_mano_params / pred_obj_params leaves of `dtype` on every set (the construction of
    test_small_loss_gpu.test_criterion_step_without_host_sync, rounded to bf16)."""
    g = torch.Generator().manual_seed(seed)
    leaf = lambda t: t.to(BF16).to(dtype).to(DEV).requires_grad_(True)  # noqa: E731
    for o in sets:
        o["pred_cams"] = [leaf(torch.randn(bs, Q, 3, generator=g) * 0.1 + 0.5), leaf(torch.randn(bs, Q, 3, generator=g) * 0.1 + 0.5)]
        o["pred_mano_params"] = [leaf(torch.randn(bs, Q, 48, generator=g) * 0.3), leaf(torch.randn(bs, Q, 10, generator=g))]
        o["pred_obj_params"] = [leaf(torch.rand(bs, Q, 1, generator=g)), leaf(torch.randn(bs, Q, 3, generator=g) * 0.3)]


def _source_leaves(sets):
    return [t for o in sets for k in SOURCES for t in o[k]]


def _criterion_case(dtype):
    from uvhand_amd.criterion import SetArcticCriterion
    from uvhand_amd.matcher import ArcticMatcher

    outputs, targets, _ = CI.arctic_case("full", 3)
    bs, Q = outputs["pred_logits"].shape[:2]
    outputs, targets = CI.to_device(outputs, targets, DEV, True)
    sets = [outputs] + outputs["aux_outputs"]
    _attach_sources(sets, bs, Q, dtype)
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
    return crit, outputs, sets, targets, args, meta


def _criterion_step(crit, outputs, sets, targets, args, meta, amp):
    for t in _source_leaves(sets):
        t.grad = None
    with _Region(amp):
        losses = crit(outputs, targets, args, meta)
        total = sum(v.sum() for v in losses.values())
    total.backward()
    return losses, [t.grad for t in _source_leaves(sets)]


def _small_keys(n_sets):
    return [k + sfx for sfx in [""] + ["_%d" % i for i in range(n_sets - 1)] for k in KEYS]


def test_criterion_step_under_bf16_autocast(monkeypatch):
    # the yardstick: the same step outside autocast, knob off, on .float() copies of the leaves
    monkeypatch.delenv(KNOB, raising=False)
    ref_losses, ref_grads = _criterion_step(*_criterion_case(torch.float32), None)
    case = _criterion_case(BF16)
    off_losses, _ = _criterion_step(*case, BF16)                      # knob off under autocast: the restatement (with syncs)
    monkeypatch.setenv(KNOB, "1")
    _criterion_step(*case, BF16)                                      # warm-up: conversions, library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses, grads = _criterion_step(*case, BF16)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert list(losses) == list(ref_losses) == list(off_losses)
    small = _small_keys(len(case[2]))
    assert all(k in losses for k in small)
    for k in losses:
        if k in small:
            assert losses[k].dtype == torch.float32 and torch.equal(losses[k], ref_losses[k]), k
        else:                                                         # the DETR keys: untouched by the knob
            assert torch.equal(losses[k], off_losses[k]) or (torch.isnan(losses[k]).all() and torch.isnan(off_losses[k]).all()), k
    for t, g, r in zip(_source_leaves(case[2]), grads, ref_grads):
        assert g.dtype == BF16 and g.shape == t.shape
        assert torch.equal(g, r.to(BF16))


def _small_many_step(S, B, Q, dtype, amp, seed=14):
    """(forward launches, backward launches) of one ArcticSmallLoss.many step over S sets."""
    g = torch.Generator().manual_seed(seed)
    sets = [{"pred_logits": (torch.randn(B, Q, CI.ARCTIC_K, generator=g) * 2).to(DEV)} for _ in range(S)]
    _attach_sources(sets, B, Q, dtype)
    _, gt, meta = _dev(*SI.case_inputs("partial", B=B, seed=13))
    m = models()
    cfg = types.SimpleNamespace(hand_idx=[12, 13])
    args = types.SimpleNamespace(img_res=SI.IMG_RES, device=DEV)
    n0 = _native.launch_count()
    with _Region(amp):
        dicts = ArcticSmallLoss(m, cfg).many(sets, gt, meta, args, ["_%d" % s for s in range(S)])
        total = sum(v.sum() for d in dicts for v in d.values())
    n1 = _native.launch_count()
    total.backward()
    return n1 - n0, _native.launch_count() - n1


@pytest.mark.parametrize("S", [1, 3])
def test_launch_count_drops_by_the_grouped_selection(S, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    F, G = _small_many_step(S, 8, 40, torch.float32, None)
    assert F > S and G > S                             # S selections next to the MANO, object and loss launches
    monkeypatch.setenv(KNOB, "1")
    assert _small_many_step(S, 8, 40, BF16, BF16) == (F - (S - 1), G - (S - 1))


def test_graph_capture_of_the_autocast_step_matches_eager(monkeypatch):
    """The device work of the criterion step (match, matched losses, the small losses over bf16 predictions) under bf16
    autocast, captured once and replayed: the eager step's gradients, bit for bit."""
    from uvhand_amd import criterion as C
    from uvhand_amd import matcher as M

    monkeypatch.setenv(KNOB, "1")
    S, B, Q = 2, 8, 40
    g = torch.Generator().manual_seed(15)
    sets = [{k: v.to(DEV).requires_grad_(True) for k, v in CI._arctic_set(g, B, Q).items()} for _ in range(S)]
    _attach_sources(sets, B, Q, BF16)
    labels = [[12, 3], [13], [12, 13, 5], [7], [13, 12], [12], [2, 13], [12, 13]]
    targets = {"labels": labels, "keypoints": [torch.rand(len(lab), CI.ARCTIC_D, generator=g).to(DEV) for lab in labels],
               "is_valid": torch.ones(B, device=DEV)}
    _, gt, meta = _dev(*SI.case_inputs("partial", B=B, seed=13))
    gt["is_valid"] = targets["is_valid"]
    m = models()
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    meta = dict(meta, obj_idx=idx, max_len=max_len)
    cfg = types.SimpleNamespace(hand_idx=[12, 13])
    args = types.SimpleNamespace(img_res=SI.IMG_RES, device=DEV)
    small = ArcticSmallLoss(m, cfg)
    packed = M.pack_targets(targets, DEV)
    nb = torch.full((1,), float(sum(len(lab) for lab in labels)), device=DEV)
    leaves = [t for o in sets for t in (o["pred_logits"], o["pred_hand_key"], o["pred_obj_key"])] + _source_leaves(sets)

    def step():
        with torch.autocast("cuda", dtype=BF16):
            res = M.match(sets, packed, CI.COST_CLASS, CI.COST_KEYPOINT)
            out = C.set_losses(sets, packed, res, nb, "arctic", CI.FOCAL_ALPHA)
            dicts = small.many(sets, gt, meta, args, ["", "_0"])
            total = out.losses.nan_to_num().sum() + sum(v.sum() for d in dicts for v in d.values())
        return torch.autograd.grad(total, leaves, allow_unused=True)

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
    assert sum(g is not None for g in eager) >= 6 * S
    for t, a, b in zip(leaves, eager, out):
        if a is None:
            assert b is None
        else:
            assert a.dtype == t.dtype and torch.equal(a, b)
