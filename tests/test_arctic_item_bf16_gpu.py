"""The grouped, dtype-generic query selection on the MI355X (csrc/msda_arctic_item.hip: msda_arctic_item_many_*).

No tolerance: the grouped kernels share the per-set kernel's device functions, so fp32 sources give its bits; bf16 sources give
the fp32 kernel's outputs on ``sources.float()`` (a bf16 widens exactly) and its gradients rounded to bf16 once."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import smoother_inputs as SI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.arctic_item import get_arctic_item, get_arctic_item_many, get_arctic_item_reference  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GROUPS = ("pred_cams", "pred_mano_params", "pred_obj_params")
KNOB = "MSDA_SMALL_LOSS_BF16"


def _to(o, dtype=torch.float32, requires_grad=False, odd=False):
    """The outputs on the device with sources of `dtype`; odd: each source a contiguous view that starts at element 1 of
    its own buffer, so that a bf16 source is 2-byte aligned and no more."""
    def src(t):
        t = t.to(DEV).to(dtype)
        if odd:
            buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)
            buf[1:] = t.reshape(-1)
            t = buf[1:].view(t.shape)
            assert t.is_contiguous() and t.data_ptr() % 4 == 2
        return t.requires_grad_(requires_grad)
    return {"pred_logits": o["pred_logits"].to(DEV), **{k: [src(t) for t in o[k]] for k in GROUPS}}


def _leaves(o):
    return [t for k in GROUPS for t in o[k]]


def _weights(seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    ws = [torch.randn(5, w, generator=g) for w in SI.ARCTIC_WIDTHS]
    return [None if i in skip else w for i, w in enumerate(ws)]


def _backward(res, weights):
    """Gradients of sum_i <res_i, w_i> (None: that output takes no part), rows of the weights cut to the batch."""
    total = sum((t * w[:t.shape[0]].to(DEV)).sum() for t, w in zip(res, weights) if w is not None)
    total.backward()


def _f32_kernel(o, weights):
    """The per-set fp32 kernel on the sources widened to fp32: (outputs, source gradients)."""
    f = {"pred_logits": o["pred_logits"], **{k: [t.detach().float().requires_grad_(True) for t in o[k]] for k in GROUPS}}
    res = SI.flatten(get_arctic_item(f, SI.Cfg()))
    _backward(res, weights)
    return res, [t.grad for t in _leaves(f)]


def _sets(case, n):
    cases = [SI.ITEM_CASES[(SI.ITEM_CASES.index(case) + i) % len(SI.ITEM_CASES)] for i in range(n)]
    return cases, [_to(SI.item_outputs(c), requires_grad=True) for c in cases]


# ---- fp32 sources: the grouped launch against the per-set kernel -------------------------------------------------------------
@pytest.mark.parametrize("n_sets", [1, 7])
@pytest.mark.parametrize("case", SI.ITEM_CASES)
def test_fp32_grouped_equals_per_set_kernel(case, n_sets):
    z = load_golden("arctic_item")
    cases, sets = _sets(case, n_sets)
    n0 = _native.launch_count()
    many = get_arctic_item_many(sets, SI.Cfg())
    assert _native.launch_count() - n0 == 1
    weights = [_weights(40 + s) for s in range(n_sets)]
    total = sum((t * w.to(DEV)).sum() for res, ws in zip(many, weights) for t, w in zip(SI.flatten(res), ws))
    n0 = _native.launch_count()
    total.backward()
    assert _native.launch_count() - n0 == 1
    _, idx = _native.arctic_item_many_forward([o["pred_logits"] for o in sets], [[t.detach() for t in _leaves(o)] for o in sets],
                                              12, 12, 13)
    for s, (c, o, res) in enumerate(zip(cases, sets, many)):
        one, grads = _f32_kernel(o, weights[s])
        _, idx1 = _native.arctic_item_forward(o["pred_logits"], [t.detach() for t in _leaves(o)], 12, 12, 13)
        assert torch.equal(idx[s], idx1)
        for i, (a, b) in enumerate(zip(SI.flatten(res), one)):
            assert a.dtype == torch.float32 and torch.equal(a, b), (c, i)
            assert np.array_equal(a.detach().cpu().numpy(), z["%s/out%d" % (c, i)]), (c, i)
        for t, g in zip(_leaves(o), grads):
            assert t.grad.dtype == torch.float32 and torch.equal(t.grad, g), c


# ---- bf16 sources ---------------------------------------------------------------------------------------------------------------
def _shape_case(bs, Q):
    """The fixtures' generator at another shape ("negative" indexes no fixed query), both hands on the last query of frame 0
    so that a row takes two gradients."""
    o = SI.item_outputs("negative", bs=bs, Q=Q)
    o["pred_logits"][0, Q - 1, 12:14] = 30.0
    return o


BF16_CASES = {c: (lambda c=c: SI.item_outputs(c)) for c in SI.ITEM_CASES}
BF16_CASES.update({"bs%d_q%d" % (bs, Q): (lambda bs=bs, Q=Q: _shape_case(bs, Q)) for bs in (1, 3) for Q in (1, 5, 256, 257, 300)})


def _check_bf16(o_cpu, odd=False, skip=()):
    weights = _weights(50, skip)
    runs = []
    for _ in range(2):
        o = _to(o_cpu, torch.bfloat16, requires_grad=True, odd=odd)
        (res,) = get_arctic_item_many([o], SI.Cfg())
        res = SI.flatten(res)
        _backward(res, weights)
        runs.append((res, [t.grad for t in _leaves(o)]))
    (res, grads), (res2, grads2) = runs
    want, want_grads = _f32_kernel(o, weights)
    for i, (a, b, c) in enumerate(zip(res, want, res2)):
        assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a, c), i
    for i, (t, g, g32, g2) in enumerate(zip(_leaves(o), grads, want_grads, grads2)):
        assert g.dtype == torch.bfloat16 and g.shape == t.shape, i
        assert torch.equal(g, g32.to(torch.bfloat16)), i
        assert torch.equal(g, g2), i


@pytest.mark.parametrize("case", list(BF16_CASES))
def test_bf16_sources_equal_the_fp32_kernel(case):
    _check_bf16(BF16_CASES[case]())


def test_bf16_sources_at_odd_elements():
    _check_bf16(_shape_case(3, 257), odd=True)
    _check_bf16(SI.item_outputs("same_query"), odd=True)


def test_bf16_gradient_of_one_output_absent():
    # root_r (output 1) shares hand_cam with root_l; pose_l (3) leaves only the right hand's rows of mano_pose
    _check_bf16(SI.item_outputs("same_query"), skip=(1,))
    _check_bf16(SI.item_outputs("ties"), skip=(3,))


def test_bf16_sets_grouped():
    cases, _ = _sets("ties", 7)
    sets = [_to(SI.item_outputs(c), torch.bfloat16, requires_grad=True) for c in cases]
    n0 = _native.launch_count()
    many = get_arctic_item_many(sets, SI.Cfg())
    assert _native.launch_count() - n0 == 1
    weights = [_weights(60 + s) for s in range(7)]
    total = sum((t * w.to(DEV)).sum() for res, ws in zip(many, weights) for t, w in zip(SI.flatten(res), ws))
    n0 = _native.launch_count()
    total.backward()
    assert _native.launch_count() - n0 == 1
    for o, res, ws in zip(sets, many, weights):
        want, want_grads = _f32_kernel(o, ws)
        assert all(torch.equal(a, b) for a, b in zip(SI.flatten(res), want))
        assert all(torch.equal(t.grad, g.to(torch.bfloat16)) for t, g in zip(_leaves(o), want_grads))


# ---- routes of get_arctic_item ------------------------------------------------------------------------------------------------
def _route(o, autocast=None):
    """(launches forward, launches backward, outputs) of get_arctic_item under an optional autocast dtype."""
    n0 = _native.launch_count()
    if autocast is None:
        res = SI.flatten(get_arctic_item(o, SI.Cfg()))
    else:
        with torch.autocast("cuda", dtype=autocast):
            res = SI.flatten(get_arctic_item(o, SI.Cfg()))
    n1 = _native.launch_count()
    sum(t.sum() for t in res).backward()
    return n1 - n0, _native.launch_count() - n1, res


def _reference(o, autocast=None):
    if autocast is None:
        return SI.flatten(get_arctic_item_reference(o, SI.Cfg()))
    with torch.autocast("cuda", dtype=autocast):
        return SI.flatten(get_arctic_item_reference(o, SI.Cfg()))


@pytest.mark.parametrize("route", ["bf16_sources", "bf16_autocast"])
def test_knob_off_keeps_the_restatement(route, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    amp = torch.bfloat16 if route == "bf16_autocast" else None
    o = _to(SI.item_outputs("ties"), torch.float32 if amp else torch.bfloat16, requires_grad=True)
    fwd, bwd, res = _route(o, amp)
    assert (fwd, bwd) == (0, 0)
    for a, b in zip(res, _reference(o, amp)):
        assert a.dtype == torch.float32 and torch.equal(a, b)


@pytest.mark.parametrize("route", ["bf16_sources", "bf16_autocast", "bf16_sources_bf16_autocast"])
def test_knob_on_runs_the_grouped_kernels(route, monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    amp = torch.bfloat16 if "autocast" in route else None
    o = _to(SI.item_outputs("ties"), torch.bfloat16 if "sources" in route else torch.float32, requires_grad=True)
    fwd, bwd, res = _route(o, amp)
    assert (fwd, bwd) == (1, 1)
    for a, b in zip(res, _reference(o, amp)):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    assert all(t.grad.dtype == t.dtype for t in _leaves(o))


def test_knob_on_fp16_autocast_keeps_the_restatement(monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    o = _to(SI.item_outputs("ties"), requires_grad=True)
    assert _route(o, torch.float16)[:2] == (0, 0)
    o = _to(SI.item_outputs("ties"), torch.bfloat16, requires_grad=True)
    assert _route(o, torch.float16)[:2] == (0, 0)
    with torch.autocast("cuda", dtype=torch.float16):
        n0 = _native.launch_count()
        get_arctic_item_many([o], SI.Cfg())
        assert _native.launch_count() == n0
