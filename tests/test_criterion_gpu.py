"""The HIP set criteria (csrc/msda_criterion.hip via uvhand_amd.criterion) on the GPU: the drop-ins against the reference-run
fixtures (tests/golden/gen_golden_r09.py), gradients against the fixture and the torch restatement, launch count, no host
sync, bitwise reproducibility, graph capture, the A/B knob and the status path."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import criterion_inputs as CI   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
DEV = torch.device("cuda:0")
EXACT = ("cardinality_error", "class_error")


@pytest.fixture(scope="module")
def C():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import criterion
    return criterion


def case_store(kind, case):
    d = np.load(os.path.join(GOLDEN, "criterion_%s.npz" % kind))
    return {k[len(case) + 2:]: d[k] for k in d.files if k.startswith(case + "__")}


def make_criterion(C, kind, case="full", small_loss=None):
    from uvhand_amd import matcher as M
    if kind == "arctic":
        return C.SetArcticCriterion(CI.ARCTIC_K, M.ArcticMatcher(CI.COST_CLASS, CI.COST_KEYPOINT),
                                    CI.weight_dict(CI.ARCTIC_WEIGHTS, 5), CI.arctic_losses(case),
                                    focal_alpha=CI.FOCAL_ALPHA, small_loss=small_loss or (lambda *a: {}))
    return C.SetAssemblyCriterion(CI.ASSEMBLY_K, M.AssemblyMatcher(CI.COST_CLASS, CI.COST_KEYPOINT),
                                  CI.weight_dict(CI.ASSEMBLY_WEIGHTS, 5, extra=("_enc",)),
                                  ["labels", "cardinality", "hand_keypoint"], focal_alpha=CI.FOCAL_ALPHA,
                                  cfg=CI.ASSEMBLY_CFG)


def inputs(kind, case, requires_grad=False):
    store = case_store(kind, case)
    make = CI.arctic_case if kind == "arctic" else CI.assembly_case
    outputs, targets, _ = make(case, int(store["seed"]))
    return (*CI.to_device(outputs, targets, DEV, requires_grad), store)


def run(crit, kind, outputs, targets):
    return crit(outputs, targets, CI.ARCTIC_ARGS, {}) if kind == "arctic" else crit(outputs, targets)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


def check_values(got, store, tol=1e-5):
    keys = [str(k) for k in store["keys"]]
    assert list(got.keys()) == keys
    for k, v in zip(keys, store["values"]):
        assert got[k].is_cuda and got[k].dim() == 0, k
        g = float(got[k])
        if np.isnan(v):
            assert np.isnan(g), k
        elif k.startswith(EXACT):
            assert g == v, (k, g, v)
        else:
            assert abs(g - v) <= tol * max(abs(v), 1e-30), (k, g, v)


def grads(outputs, kind):
    return {name: torch.stack([s[name].grad for s in CI.sets_of(outputs)]) for name in CI.heads(kind)}


VALUE_CASES = [("arctic", c) for c in CI.ARCTIC_CASES if c != "no_valid_label"] + [("assembly", "full"),
                                                                                  ("assembly", "small")]


@pytest.mark.parametrize("kind,case", VALUE_CASES)
def test_drop_in_matches_reference_values(C, kind, case):
    outputs, targets, store = inputs(kind, case)
    check_values(run(make_criterion(C, kind, case), kind, outputs, targets), store)


@pytest.mark.parametrize("kind", ["arctic", "assembly"])
def test_gradients_match_reference_small(C, kind):
    outputs, targets, store = inputs(kind, "small", requires_grad=True)
    crit = make_criterion(C, kind, "small")
    CI.weighted_total(run(crit, kind, outputs, targets), crit.weight_dict).backward()
    for name, g in grads(outputs, kind).items():
        assert rel(g.cpu().numpy(), store["grad_" + name]) <= 1e-5, name


@pytest.mark.parametrize("kind", ["arctic", "assembly"])
def test_window32_gradients_match_restatement_on_device(C, kind, monkeypatch):
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("MSDA_CRITERION_FUSED", fused)
        outputs, targets, _ = inputs(kind, "full", requires_grad=True)
        crit = make_criterion(C, kind)
        d = run(crit, kind, outputs, targets)
        CI.weighted_total(d, crit.weight_dict).backward()
        got[fused] = (d, grads(outputs, kind))
    (d1, g1), (d0, g0) = got["1"], got["0"]
    assert list(d1.keys()) == list(d0.keys())               # MSDA_CRITERION_FUSED=0 gives the same dict
    for k in d1:
        assert abs(float(d1[k]) - float(d0[k])) <= 1e-5 * max(abs(float(d0[k])), 1e-30), k
    for name in g1:
        assert rel(g1[name].cpu().numpy(), g0[name].cpu().numpy()) <= 1e-5, name


def test_no_valid_label_every_key_zero(C):
    outputs, targets, store = inputs("arctic", "no_valid_label")
    d = run(make_criterion(C, "arctic", "no_valid_label"), "arctic", outputs, targets)
    assert len(d) == 9 and all(float(v) == 0.0 for v in d.values())


def _step(C, kind, outputs, targets):
    from uvhand_amd import matcher as M
    sets = CI.sets_of(outputs)
    packed = M.pack_targets(targets, DEV)
    jv = C.pack_joint_valid(targets, DEV) if kind == "assembly" else None
    res = M.match(sets, packed, CI.COST_CLASS, CI.COST_KEYPOINT)
    out = C.set_losses(sets, packed, res, torch.full((1,), 7.0, device=DEV), kind, CI.FOCAL_ALPHA, CI.HAND_IDX, jv)
    return sets, out


@pytest.mark.parametrize("kind", ["arctic", "assembly"])
def test_set_losses_two_launches_no_sync(C, kind):
    from uvhand_amd import _native
    from uvhand_amd import matcher as M
    outputs, targets, _ = inputs(kind, "full", requires_grad=True)
    sets = CI.sets_of(outputs)
    packed = M.pack_targets(targets, DEV)
    jv = C.pack_joint_valid(targets, DEV) if kind == "assembly" else None
    weights = torch.rand(len(sets), 4, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = M.match(sets, packed, CI.COST_CLASS, CI.COST_KEYPOINT)
        n0 = _native.launch_count()
        out = C.set_losses(sets, packed, res, torch.full((1,), 7.0, device=DEV), kind, CI.FOCAL_ALPHA, CI.HAND_IDX, jv)
        (out.losses * weights).sum().backward()
        n1 = _native.launch_count()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert n1 - n0 == 2
    assert int(out.status.abs().sum()) == 0


def test_assembly_drop_in_forward_makes_no_sync(C):
    outputs, targets, _ = inputs("assembly", "full")
    crit = make_criterion(C, "assembly")
    run(crit, "assembly", outputs, targets)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            run(crit, "assembly", outputs, targets)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert not syncs, [str(w.message) for w in syncs]


@pytest.mark.parametrize("kind", ["arctic", "assembly"])
def test_bitwise_reproducible(C, kind):
    ref = None
    for _ in range(5):
        outputs, targets, _ = inputs(kind, "full", requires_grad=True)
        sets, out = _step(C, kind, outputs, targets)
        (out.losses * torch.arange(1, 5, device=DEV, dtype=torch.float32)).sum().backward()
        got = [out.losses.detach().clone()] + list(grads(outputs, kind).values())
        torch.cuda.synchronize()
        if ref is None:
            ref = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, ref))


def test_graph_capture_match_losses_backward(C):
    from uvhand_amd import matcher as M
    outputs, targets, _ = inputs("arctic", "full")
    sets = CI.sets_of(outputs)
    leaves = [s[k] for s in sets for k in CI.heads("arctic")]
    for t in leaves:
        t.requires_grad_(True)
    packed = M.pack_targets(targets, DEV)
    nb = torch.full((1,), 9.0, device=DEV)
    w = torch.rand(len(sets), 4, device=DEV)

    def step():
        res = M.match(sets, packed, CI.COST_CLASS, CI.COST_KEYPOINT)
        out = C.set_losses(sets, packed, res, nb, "arctic", CI.FOCAL_ALPHA)
        g = torch.autograd.grad((out.losses.nan_to_num() * w).sum(), leaves)
        return out.losses, g

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_losses, cap_grads = step()
    g = torch.Generator(device=DEV).manual_seed(5)
    with torch.no_grad():
        for o in sets:
            o["pred_logits"].copy_(torch.randn(o["pred_logits"].shape, generator=g, device=DEV) * 2)
            o["pred_hand_key"].mul_(0.5).add_(0.25)
    graph.replay()
    eager_losses, eager_grads = step()
    torch.cuda.synchronize()
    assert torch.equal(cap_losses.nan_to_num(), eager_losses.nan_to_num())
    assert all(torch.equal(a, b) for a, b in zip(cap_grads, eager_grads))


def test_status_nan_and_check_mode(C, monkeypatch):
    """A matched AssemblyHands label outside hand_idx: the reference raises (joint_valid mask); the fused path marks the
    set's status and returns nan for its loss_hand_keypoint; MSDA_CRITERION_CHECK=1 raises the reference's error."""
    from uvhand_amd import _native
    outputs, targets, store = inputs("assembly", "not_hand")
    d = run(make_criterion(C, "assembly"), "assembly", outputs, targets)
    assert np.isnan(float(d["loss_hand_keypoint"])) and np.isfinite(float(d["loss_ce"]))
    _, out = _step(C, "assembly", outputs, targets)
    assert ((out.status.cpu() & _native.CRIT_MASK_MISMATCH) != 0).all()
    monkeypatch.setenv("MSDA_CRITERION_CHECK", "1")
    with pytest.raises(IndexError) as e:
        run(make_criterion(C, "assembly"), "assembly", outputs, targets)
    assert str(e.value) == str(store["error"])


def test_enc_outputs_raise_before_launch(C):
    from uvhand_amd import _native
    outputs, targets, store = inputs("assembly", "enc")
    n0 = _native.launch_count()
    with pytest.raises(IndexError) as e:
        run(make_criterion(C, "assembly"), "assembly", outputs, targets)
    assert str(e.value) == str(store["error"]) and _native.launch_count() == n0
