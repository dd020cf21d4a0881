"""The ARCTIC evaluation drop-ins on the CPU (uvhand_amd/arctic_eval.py): the torch restatements against
tests/golden/arctic_eval.npz, which gen_arctic_eval.py made by running the reference's own make_output / prepare_data /
measure_error and eval functions; the evaluator against the fixture's engine-style means; the nearest neighbour's tie rule
and gradient.

Tolerances.  prepare_data tensors: 1e-5 relative (the same fp32 operations as the reference in torch; measured 0).  Metric rows
and step means: 16 x 2^-24 relative to the row's largest value (fp32 restatement against the fp32 reference: the one
difference is torch's sequential mean where the reference uses numpy's pairwise one, over 21 or B terms)."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import arctic_eval_inputs as EI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd import arctic_eval as AE  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors  # noqa: E402

TOL = 16 * 2.0 ** -24


@pytest.fixture(scope="module")
def models():
    return dict(EI.mano_models(), arti_head=ObjectTensors.from_arrays(SI.obj_arrays()))


@pytest.fixture(scope="module")
def z():
    return load_golden("arctic_eval")


def _data(case, models, flag="eval"):
    outputs, targets, meta = EI.case_inputs(case)
    return AE.prepare_data(EI.args(), outputs, targets, meta, EI.CFG, flag=flag, models=models)


@pytest.mark.parametrize("case", list(EI.CASES))
def test_make_output_keys_and_pose(case, models, z):
    outputs, targets, meta = EI.case_inputs(case)
    mo = AE.post_process_arctic_output(outputs, AE.XDict(meta), EI.args(), EI.CFG, models=models)
    assert list(mo.keys()) == list(z[case + "/mo_keys"])
    for s in ("r", "l"):
        assert mo["mano.pose." + s].shape == (SI.FIXTURE_B, 16, 3, 3)
        assert rel_err(mo["mano.pose." + s].numpy(), z["%s/mo/mano.pose.%s" % (case, s)]) < 1e-5


@pytest.mark.parametrize("case", list(EI.CASES))
def test_prepare_data_against_the_reference(case, models, z):
    data = _data(case, models)
    assert list(data.keys()) == list(z[case + "/keys"])
    seen = 0
    for k in z:
        if not k.startswith(case + "/data/"):
            continue
        got, ref = data[k.split("/data/")[1]], z[k]
        assert tuple(got.shape) == ref.shape and got.device.type == "cpu", k
        if ref.dtype.kind == "f":
            assert got.dtype == torch.float32 and rel_err(got.numpy(), ref) < 1e-5, k
        else:
            assert np.array_equal(got.numpy(), ref), k
        seen += 1
    assert seen >= (80 if case == "partial" else 60)
    # the nearest-neighbour keys are not fixtures (the generator cannot run knn_points): fp64 brute force on the same clouds
    for h in ("r", "l"):
        src, trg = data["pred.object.v.cam"].double(), data["pred.mano.v3d.cam." + h].double()
        i64, _, gap = EI.nn_yardstick(src, trg)
        assert torch.equal(data["pred.nn_idx_" + h][gap >= 2.0 ** -20], i64[gap >= 2.0 ** -20])


@pytest.mark.parametrize("case", list(EI.CASES))
def test_measure_error_against_the_reference(case, models, z):
    stats = AE.measure_error(_data(case, models), list(AE.DEFAULT_METRICS))
    assert list(stats.keys()) == list(AE.METRIC_KEYS)
    for k in AE.METRIC_KEYS:
        ref = z["%s/metric/%s" % (case, k)]
        assert isinstance(stats[k], np.ndarray) and stats[k].shape == ref.shape
        assert np.array_equal(np.isnan(stats[k]), np.isnan(ref)), k
        ok = ~np.isnan(ref)
        if k.startswith("success_rate"):
            assert np.array_equal(stats[k][ok].astype(np.float32), ref[ok].astype(np.float32))
        elif ok.any():
            assert rel_err(stats[k][ok], ref[ok]) < TOL, k
    assert np.isnan(z["no_contact/metric/cdev/ho"]).all() and np.isnan(z["partial/metric/aae"][2])


def test_fp64_restatement_and_requested_rows(models, z):
    data = _data("partial", models)
    r64 = AE.arctic_metrics_reference(data, torch.float64)
    assert r64.dtype == torch.float64 and r64.shape == (6, SI.FIXTURE_B)
    d = AE.arctic_metrics_dict(data, ["mrrpe", "aae", "mdev"])
    assert list(d) == ["mrrpe/r/l", "mrrpe/r/o", "aae"]
    with pytest.raises(NotImplementedError):
        AE.measure_error(data, ["avg_err_field"])


def test_evaluator_against_the_engine_style_means(models, z):
    ev = AE.ArcticEvaluator()
    for case in EI.SEQUENCE:
        vals = ev.update(_data(case, models))
        for i, k in enumerate(AE.METRIC_KEYS):
            ref = float(z["%s/step/%s" % (case, k)])
            ok = ~torch.isnan(vals[i])
            assert bool(ok.any()) == (ref == ref), (case, k)                  # a key dropped for this step
            if ref == ref:
                assert abs(float(vals[i][ok].double().mean()) - ref) < TOL * abs(ref), (case, k)
    assert np.isnan(z["no_contact/step/cdev/ho"])
    out = ev.compute()
    assert list(out) == list(AE.METRIC_KEYS)
    for k in AE.METRIC_KEYS:
        ref = float(z["avg/" + k])
        assert abs(out[k] - ref) < TOL * abs(ref), k
    # cdev was present in four of the five steps: its average divides by four
    assert float(ev.count[AE.METRIC_KEYS.index("cdev/ho")]) == 4 and float(ev.count[0]) == 5
    assert AE.ArcticEvaluator(["aae"]).compute() == {}


def test_models_are_required(models):
    outputs, targets, meta = EI.case_inputs("all_valid")
    AE.set_default_models(None)
    with pytest.raises(RuntimeError, match="models"):
        AE.prepare_data(EI.args(), outputs, targets, meta, EI.CFG)
    AE.set_default_models(models)
    try:
        assert "pred.nn_idx_l" in AE.prepare_data(EI.args(), outputs, targets, meta, EI.CFG)
    finally:
        AE.set_default_models(None)


def test_container():
    d = AE.XDict({"pred.a": torch.ones(2), "targets.a": [torch.zeros(1)], "meta_info.names": ["box"]})
    with pytest.raises(AssertionError):
        d["pred.a"] = 1
    d.overwrite("pred.a", torch.zeros(2))
    assert list(d.search("pred.", "")) == ["a"] and list(d.rm("pred.")) == ["targets.a", "meta_info.names"]
    assert list(AE.XDict({"a": 1}).prefix("x.")) == ["x.a"]
    with pytest.raises(AssertionError):
        d.merge({"pred.a": 2})
    assert d.to("cpu")["meta_info.names"] == ["box"] and isinstance(d.to_np()["pred.a"], np.ndarray)


def test_nn_tie_rule_and_k():
    g = torch.Generator().manual_seed(3)
    src, trg = torch.randn(2, 50, 3, generator=g), torch.randn(2, 20, 3, generator=g)
    trg[:, 11] = trg[:, 4]                                   # duplicate targets: the lowest index wins
    trg[:, 17] = trg[:, 4]
    src[:, :10] = trg[:, 4:5] + 1e-3 * torch.randn(2, 10, 3, generator=g)
    dist, idx = AE.get_NN(src, trg)
    assert dist.shape == (2, 50) and idx.shape == (2, 50) and idx.dtype == torch.int64 and dist.dtype == torch.float32
    assert (idx[:, :10] == 4).all() and not ((idx == 11) | (idx == 17)).any()
    d64 = ((src.double()[:, :, None] - trg.double()[:, None]) ** 2).sum(-1)
    assert torch.equal(torch.where(d64 == d64.min(2, keepdim=True).values, torch.arange(20), 20).min(2).values, idx)
    assert rel_err(dist.numpy(), d64.min(2).values.numpy()) < 1e-6
    trg[0, 3] = float("nan")                                 # a NaN distance never wins
    assert not (AE.get_NN(src, trg)[1][0] == 3).any()
    for k in (0, 2):
        with pytest.raises(ValueError):
            AE.get_NN(src, trg, k=k)


def test_nn_gradient_against_the_fp64_composition():
    (src, trg), = EI.nn_inputs(5, 3, 200, 60, pairs=1)
    a, b = src.clone().requires_grad_(True), trg.clone().requires_grad_(True)
    dist, idx = AE.get_NN(a, b)
    w = torch.randn(dist.shape, generator=torch.Generator().manual_seed(6))
    (dist * w).sum().backward()
    a64, b64 = src.double().requires_grad_(True), trg.double().requires_grad_(True)
    comp = ((a64 - torch.gather(b64, 1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
    (comp * w.double()).sum().backward()
    assert not idx.requires_grad
    assert rel_err(a.grad.numpy(), a64.grad.numpy()) < 1e-5 and rel_err(b.grad.numpy(), b64.grad.numpy()) < 1e-5


def test_gpu_nn_inputs_have_few_near_ties():
    """What tests/test_arctic_eval_gpu.py relies on, from the fp64 data alone: at its seeded inputs the share of source points
    whose best and second-best squared distances lie within 2^-20 relative (fp32 cannot order those) is within 0.1 %."""
    near, total = 0, 0
    for src, trg in EI.nn_inputs(EI.NN_SEED, 32, 4000, 778, dtype=torch.float64):
        _, _, gap = EI.nn_yardstick(src, trg)
        near += int((gap < 2.0 ** -20).sum())
        total += gap.numel()
    assert near <= 1e-3 * total, (near, total)


def test_gpu_success_inputs_are_clear_of_their_thresholds():
    """What tests/test_arctic_eval_gpu.py's realistic-size case relies on, from the fp64 data alone: no vertex of
    arctic_eval_inputs.BIG lies within BIG_MARGIN (1e-3 relative) of its success threshold, so an fp32 evaluation (about 2e-4
    at that depth) counts what fp64 counts; and the frames do have mixed outcomes."""
    lengths = EI.BIG_LENGTHS
    outputs, targets, meta = EI.case_inputs(lengths=lengths, **EI.BIG)
    m = dict(EI.mano_models(), arti_head=ObjectTensors.from_arrays(SI.obj_arrays(lengths=lengths)))
    mo = AE.post_process_arctic_output(outputs, AE.XDict(meta), EI.args(), EI.CFG, models=m)
    margin, dists = EI.success_margin(targets["object.v.cam"], mo["object.v.cam"], targets["object.v_len"], meta["part_ids"],
                                      meta["diameter"])
    assert float(margin.min()) > EI.BIG_MARGIN, margin
    rates = [float((d < thr).double().mean()) for d, thr in dists]
    assert sum(0 < r < 1 for r in rates) >= 16 and max(int(n) for n in targets["object.v_len"]) > 3900
