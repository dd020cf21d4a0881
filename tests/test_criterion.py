"""The set criteria's torch restatement (uvhand_amd/criterion.py; the fallback the drop-ins take on the CPU) against the
reference-run fixtures (tests/golden/gen_golden_r09.py), host-side errors, packing and the always-present keys.  CPU only
(the matchers' composition needs scipy)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import criterion_inputs as CI   # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
pytest.importorskip("scipy", reason="the matchers' CPU composition solves with scipy")


@pytest.fixture(scope="module")
def C():
    from uvhand_amd import criterion
    return criterion


def fixture(kind):
    return np.load(os.path.join(GOLDEN, "criterion_%s.npz" % kind))


def case_store(kind, case):
    d = fixture(kind)
    return {k[len(case) + 2:]: d[k] for k in d.files if k.startswith(case + "__")}


def make_criterion(C, kind, case, **kw):
    from uvhand_amd import matcher as M
    if kind == "arctic":
        return C.SetArcticCriterion(CI.ARCTIC_K, M.ArcticMatcher(CI.COST_CLASS, CI.COST_KEYPOINT),
                                    CI.weight_dict(CI.ARCTIC_WEIGHTS, 5), CI.arctic_losses(case),
                                    focal_alpha=CI.FOCAL_ALPHA, small_loss=kw.pop("small_loss", lambda *a: {}), **kw)
    return C.SetAssemblyCriterion(CI.ASSEMBLY_K, M.AssemblyMatcher(CI.COST_CLASS, CI.COST_KEYPOINT),
                                  CI.weight_dict(CI.ASSEMBLY_WEIGHTS, 5, extra=("_enc",)),
                                  ["labels", "cardinality", "hand_keypoint"], focal_alpha=CI.FOCAL_ALPHA,
                                  cfg=CI.ASSEMBLY_CFG)


def run(crit, kind, outputs, targets):
    return crit(outputs, targets, CI.ARCTIC_ARGS, {}) if kind == "arctic" else crit(outputs, targets)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


def check_values(got, store, tol):
    keys = [str(k) for k in store["keys"]]
    assert list(got.keys()) == keys
    for k, v in zip(keys, store["values"]):
        g = float(got[k])
        if np.isnan(v):
            assert np.isnan(g), k
        else:
            assert abs(g - v) <= tol * max(abs(v), 1e-30), (k, g, v)


VALUE_CASES = [("arctic", c) for c in CI.ARCTIC_CASES if c != "no_valid_label"] + [("assembly", "full"),
                                                                                  ("assembly", "small")]


@pytest.mark.parametrize("kind,case", VALUE_CASES)
def test_restatement_matches_reference_values(C, kind, case):
    store = case_store(kind, case)
    make = CI.arctic_case if kind == "arctic" else CI.assembly_case
    outputs, targets, _ = make(case, int(store["seed"]))
    got = run(make_criterion(C, kind, case), kind, outputs, targets)
    check_values(got, store, 1e-6)


@pytest.mark.parametrize("kind", ["arctic", "assembly"])
def test_restatement_matches_reference_gradients(C, kind):
    store = case_store(kind, "small")
    make = CI.arctic_case if kind == "arctic" else CI.assembly_case
    outputs, targets, _ = make("small", int(store["seed"]))
    outputs, targets = CI.to_device(outputs, targets, "cpu", requires_grad=True)
    crit = make_criterion(C, kind, "small")
    CI.weighted_total(run(crit, kind, outputs, targets), crit.weight_dict).backward()
    for name in CI.heads(kind):
        got = np.stack([s[name].grad.numpy() for s in CI.sets_of(outputs)])
        assert rel(got, store["grad_" + name]) <= 1e-5, name


def test_arctic_no_valid_label_keeps_every_key(C):
    """The one change: the reference omits the DETR keys when its matcher returns 0; the drop-in returns them, all 0."""
    store = case_store("arctic", "no_valid_label")
    assert store["keys"].size == 0                      # the reference's dict (small losses stubbed): nothing
    outputs, targets, _ = CI.arctic_case("no_valid_label", int(store["seed"]))
    got = run(make_criterion(C, "arctic", "no_valid_label"), "arctic", outputs, targets)
    base = ["loss_ce", "loss_hand_keypoint", "loss_obj_keypoint"]
    assert list(got.keys()) == base + [k + s for s in ("_0", "_1") for k in base]
    assert all(float(v) == 0.0 for v in got.values())


@pytest.mark.parametrize("case", ["enc", "not_hand"])
def test_assembly_reference_errors(C, case):
    store = case_store("assembly", case)
    outputs, targets, _ = CI.assembly_case(case, int(store["seed"]))
    with pytest.raises(IndexError) as e:
        run(make_criterion(C, "assembly", case), "assembly", outputs, targets)
    assert str(e.value) == str(store["error"])


def test_small_loss_hook_and_key_order(C):
    calls = []

    def small(outputs, targets, meta_info, args, suffix):
        calls.append(suffix)
        return {"loss_mano" + suffix: outputs["pred_logits"].sum() * 0}

    store = case_store("arctic", "interleaved")
    outputs, targets, _ = CI.arctic_case("interleaved", int(store["seed"]))
    got = run(make_criterion(C, "arctic", "interleaved", small_loss=small), "arctic", outputs, targets)
    assert calls == ["", "_0", "_1"]                    # final and aux sets; interm has none (the reference's loop)
    keys = list(got.keys())
    assert keys.index("loss_mano") == 4 and keys.index("loss_mano_0") == 9 and keys[-1] == "cardinality_error_interm"


def test_pack_joint_valid_order(C):
    _, targets, _ = CI.assembly_case("full", 1)
    jv = C.pack_joint_valid(targets, "cpu")
    assert jv.dtype == torch.uint8 and tuple(jv.shape) == (sum(len(v["labels"]) for v in targets), 63)
    ref = torch.cat([v["joint_valid"] for v in targets]).view(-1, 63)
    assert torch.equal(jv.bool(), ref)


def test_set_losses_host_errors(C):
    from uvhand_amd import matcher as M
    outputs, targets, _ = CI.assembly_case("small", 3)
    packed = M.pack_targets(targets, "cpu")
    with pytest.raises(ValueError, match="joint_valid"):
        C.set_losses([outputs], packed, None, 1.0)
    with pytest.raises(ValueError, match="kind"):
        C.set_losses([outputs], packed, None, 1.0, kind="coco")
    with pytest.raises(ValueError, match="hand labels"):
        C._hand_mask([64])
    assert C._hand_mask([1, 2]) == 6 and C._hand_mask(C.ARCTIC_HANDS) == (1 << 12) | (1 << 13)


def test_fallback_on_cpu_and_knob(C, monkeypatch):
    """CPU tensors never reach the fused path; MSDA_CRITERION_FUSED=0 turns it off everywhere."""
    t = torch.zeros(2, 3, 4)
    assert not C._fusable([t], [1, 1], 2, 1)
    monkeypatch.setenv("MSDA_CRITERION_FUSED", "0")
    assert not C._fused_enabled()
    monkeypatch.setenv("MSDA_CRITERION_FUSED", "1")
    assert C._fused_enabled()
