"""The DINO criterion drop-in on the CPU (uvhand_amd.criterion.SetDinoCriterion, its torch restatement route) and
DinoHungarianMatcher against the reference-run fixture (tests/golden/gen_dino_criterion.py): key sets, values, nan placement,
the gradients of the weighted total and the matcher's index lists.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import dino_criterion_inputs as DI   # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
TOL = 1e-5


def case_store(case):
    d = np.load(os.path.join(GOLDEN, "dino_criterion.npz"))
    return {k[len(case) + 2:]: d[k] for k in d.files if k.startswith(case + "__")}


def make_criterion(case, small_loss=None):
    from uvhand_amd import criterion as C
    from uvhand_amd import matcher as M
    matcher = M.DinoHungarianMatcher(DI.COST_CLASS, DI.COST_BBOX, DI.COST_GIOU, DI.FOCAL_ALPHA)
    crit = C.SetDinoCriterion(DI.K, matcher, DI.weight_dict(DI.shape(case)[4]), DI.FOCAL_ALPHA, DI.losses(case), None, None,
                              small_loss=small_loss or (lambda *a: {}))
    return crit.train(case != "eval")


def inputs(case, device="cpu", requires_grad=False):
    store = case_store(case)
    outputs, targets, _ = DI.make(case, int(store["seed"]))
    return (*DI.to_device(outputs, targets, device, requires_grad), store)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


def check_values(got, store, tol=TOL):
    keys = [str(k) for k in store["keys"]]
    assert list(got.keys()) == keys
    for k, v in zip(keys, store["values"]):
        assert got[k].dim() == 0, k
        g = float(got[k])
        if np.isnan(v):
            assert np.isnan(g), k
        else:
            assert abs(g - v) <= tol * max(abs(v), 1e-30), (k, g, v)


@pytest.mark.parametrize("case", DI.CASES)
def test_cpu_drop_in_matches_reference_values(case):
    outputs, targets, store = inputs(case)
    check_values(make_criterion(case)(outputs, targets, DI.ARGS, {}), store)


def test_no_object_is_nan_where_the_reference_is():
    outputs, targets, store = inputs("no_object")
    got = make_criterion("no_object")(outputs, targets, DI.ARGS, {})
    nan_keys = [str(k) for k, v in zip(store["keys"], store["values"]) if np.isnan(v)]
    assert nan_keys and all(k.startswith("loss_obj_keypoint") for k in nan_keys) and "loss_obj_keypoint_dn" in nan_keys
    assert [k for k, v in got.items() if torch.isnan(v)] == nan_keys


def test_zero_denoising_keys_without_known_outputs():
    from uvhand_amd import criterion as C
    for case in ("eval", "no_dn"):
        outputs, targets, _ = inputs(case)
        got = make_criterion(case)(outputs, targets, DI.ARGS, {})
        assert list(got.keys())[:6] == list(C.DINO_ZERO_DN_KEYS)
        assert all(float(got[k]) == 0.0 for k in C.DINO_ZERO_DN_KEYS)


def test_small_gradients_match_reference():
    outputs, targets, store = inputs("small", requires_grad=True)
    crit = make_criterion("small")
    DI.weighted_total(crit(outputs, targets, DI.ARGS, {}), crit.weight_dict).backward()
    grads = DI.gradients(outputs)
    assert sorted(grads) == sorted(k for k in store if k.startswith("grad_"))
    for name, g in grads.items():
        assert np.abs(store[name]).max() > 0, name
        assert rel(g.numpy(), store[name]) <= TOL, name


@pytest.mark.parametrize("case", ["small", "interleaved"])
def test_matcher_returns_reference_indices(case):
    outputs, targets, store = inputs(case)
    crit = make_criterion(case)
    pairs = crit.matcher(DI.sets_of(outputs)[0], targets)
    assert [len(q) for q, _ in pairs] == store["index_sizes"].tolist()
    assert all(q.dtype == torch.int64 and t.dtype == torch.int64 for q, t in pairs)
    assert torch.cat([q for q, _ in pairs]).tolist() == store["index_query"].tolist()
    assert torch.cat([t for _, t in pairs]).tolist() == store["index_target"].tolist()


def test_return_indices_lists_aux_interm_final():
    outputs, targets, _ = inputs("small")
    crit = make_criterion("small")
    losses, indices = crit(outputs, targets, DI.ARGS, {}, return_indices=True)
    sets = DI.sets_of(outputs)
    assert len(indices) == len(sets)
    for got, o in zip(indices, sets[1:] + sets[:1]):
        want = crit.matcher(o, targets)
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, want))
    assert list(losses.keys()) == list(crit(outputs, targets, DI.ARGS, {}).keys())


def test_matcher_constructor_and_alpha_route():
    from uvhand_amd import matcher as M
    with pytest.raises(AssertionError):
        M.DinoHungarianMatcher(0, 0, 0)
    m = M.DinoHungarianMatcher(0, 0, 1)                      # the reference accepts a giou weight alone
    assert m.cost_keypoint == m.cost_bbox == 0 and m.focal_alpha == 0.25
    outputs, targets, _ = inputs("small")
    a = M.DinoHungarianMatcher(DI.COST_CLASS, DI.COST_BBOX, focal_alpha=0.25)(DI.sets_of(outputs)[0], targets)
    b = M.DinoHungarianMatcher(DI.COST_CLASS, 0.0, focal_alpha=0.9)(DI.sets_of(outputs)[0], targets)
    want = M.arctic_composition(DI.sets_of(outputs)[0], targets, DI.COST_CLASS, 0.0, alpha=0.9)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(b, want))
    assert len(a) == len(b)


def test_small_loss_many_covers_final_and_aux():
    class Many:
        calls = 0

        def many(self, sets, targets, meta_info, args, suffixes):
            Many.calls += 1
            return [{"loss_mano" + s: torch.tensor(float(i))} for i, s in enumerate(suffixes)]

    outputs, targets, _ = inputs("small")
    got = make_criterion("small", small_loss=Many())(outputs, targets, DI.ARGS, {})
    assert Many.calls == 1 and float(got["loss_mano"]) == 0 and float(got["loss_mano_1"]) == 2
    assert "loss_mano_interm" not in got and "loss_mano_dn" not in got


def test_enc_outputs_keep_the_reference_assertion():
    outputs, targets, _ = inputs("small")
    outputs["enc_outputs"] = [{"pred_logits": outputs["pred_logits"]}]
    with pytest.raises(AssertionError):
        make_criterion("small")(outputs, targets, DI.ARGS, {})


def test_masks_are_left_out():
    outputs, targets, _ = inputs("small")
    crit = make_criterion("small")
    crit.losses = ["labels", "masks"]
    with pytest.raises(NotImplementedError):
        crit(outputs, targets, DI.ARGS, {})
