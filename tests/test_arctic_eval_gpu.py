"""The ARCTIC evaluation step on the MI355X (csrc/msda_arctic_eval.hip): nearest neighbour, metric kernel, evaluator, glue.

Tolerances.
  Nearest neighbour, against fp64 brute force at B = 32, N1 = 4000, N2 = 778, two pairs, camera-space clouds at z = 12 m: the
  index equals the fp64 argmin except where the fp64 gap between the best and second-best squared distance is below 2^-20
  relative (fp32 cannot order those; at most 0.1 % of the points, asserted from the fp64 data in test_arctic_eval.py too); the
  distance at the returned index is within 8 x 2^-24 relative of the fp64 value there (torch fp32 in the kernel's order
  measured 3.98 x 2^-24; 8 leaves a factor of two for FMA contraction).  Backward: 1e-5 relative against the fp64 composition
  (a target's sum has at most N1 terms of like size) and bitwise equal across runs.
  Metric kernel, against arctic_metrics_reference(dtype=float64) on the same inputs: NaN pattern identical; success_rate
  exactly equal on the fixture cases (the generator asserts in fp64 that no vertex is within 1e-4 relative of its
  threshold); the other five rows within 4 x the deviation of the reference-run fp32 fixture from the same fp64 values
  (same number of fp32 terms in another order, and FMA), floor 16 x 2^-24, relative to the row's largest value.  The
  deviations are measured at test time on the CPU; when this was written they were, in units of 2^-24: aae 4.88,
  mpjpe/ra/h 2.27, mrrpe/r/l 1.12, mrrpe/r/o 4.13, cdev/ho 1.61, giving the bounds 19.5 (aae), 16.5 (mrrpe/r/o) and 16 (the
  rest) x 2^-24.
  At realistic size (B = 32, objects of about 4000 rows at z of 10 to 20 m) the same bounds hold and the success counts are
  compared exactly.  There one fp32 ulp of a coordinate is 1e-6 m and a threshold is 5 to 15 mm, so an fp32 evaluation cannot
  place a vertex within about 2e-4 relative of its threshold; the seeded inputs (arctic_eval_inputs.BIG) therefore keep every
  vertex at least 2e-3 away in fp64, test_arctic_eval.py asserts 1e-3 from the fp64 data on the CPU, and the test here
  asserts the same 1e-3 on the device-made data before it compares.
  prepare_data(flag='device') against the fixture: 2e-4 relative, the bound tests/test_small_loss_gpu.py uses for the same
  MANO / object / projection chain.  The nearest-neighbour keys are not fixtures (the generator cannot run knn_points):
  nn_idx_* is held against fp64 brute force on the same clouds, equal except where the fp64 gap between the two nearest
  targets is below 2^-20 relative, and nn_dist_* within 8 x 2^-24 of the fp64 value at the returned index, as in the
  nearest-neighbour test."""
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import arctic_eval_inputs as EI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd import arctic_eval as AE  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOOR = 16 * 2.0 ** -24


def models(dev, lengths=None):
    return dict(EI.mano_models(dev), arti_head=ObjectTensors.from_arrays(SI.obj_arrays(lengths=lengths)).to(dev))


@pytest.fixture(scope="module")
def z():
    return load_golden("arctic_eval")


@pytest.fixture(scope="module")
def cpu_data():
    """prepare_data of every fixture case on the CPU (bitwise the reference's tensors, test_arctic_eval.py)."""
    m = models("cpu")
    return {case: AE.prepare_data(EI.args(), *EI.case_inputs(case), EI.CFG, flag="device", models=m) for case in EI.CASES}


@pytest.fixture(scope="module")
def bounds(z, cpu_data):
    """Per key: max(4 x the fixture's deviation from the fp64 restatement, 16 x 2^-24), measured here on the CPU."""
    dev = {k: 0.0 for k in AE.METRIC_KEYS}
    for case, data in cpu_data.items():
        r64 = AE.arctic_metrics_reference(data, torch.float64).numpy()
        for i, k in enumerate(AE.METRIC_KEYS):
            ref = z["%s/metric/%s" % (case, k)]
            ok = ~np.isnan(ref)
            if ok.any():
                dev[k] = max(dev[k], rel_err(ref[ok], r64[i][ok]))
    print("fixture deviations from fp64 (x 2^-24):", {k: round(v * 2 ** 24, 2) for k, v in dev.items()})
    return {k: max(4 * v, FLOOR) for k, v in dev.items()}


def _check_rows(vals, r64, bounds, what, v_len):
    """The kernel's rows against the fp64 restatement.  success_rate is a count over v_len rows: the counts must be equal
    (the two percentages differ in their last bit, 100 c / n being rounded once in fp64 and twice in fp32)."""
    vals, r64, v_len = vals.double().cpu().numpy(), r64.cpu().numpy(), v_len.double().cpu().numpy()
    for i, k in enumerate(AE.METRIC_KEYS):
        assert np.array_equal(np.isnan(vals[i]), np.isnan(r64[i])), (what, k)
        ok = ~np.isnan(r64[i])
        if not ok.any():
            continue
        err = rel_err(vals[i][ok], r64[i][ok])
        print("%s %-18s rel err %.3g (x 2^-24: %.2f)" % (what, k, err, err * 2 ** 24))
        if k.startswith("success_rate"):
            assert np.array_equal(np.rint(vals[i][ok] * v_len[ok] / 100), np.rint(r64[i][ok] * v_len[ok] / 100)), (what, k)
            assert err < FLOOR, (what, k, err)
        else:
            assert err < bounds[k], (what, k, err)


def test_nn_forward_against_fp64():
    pairs = [(s.to(DEV), t.to(DEV)) for s, t in EI.nn_inputs(EI.NN_SEED, 32, 4000, 778)]
    outs = AE.nn_many(pairs)
    skipped = total = 0
    for (s, t), (dist, idx) in zip(pairs, outs):
        assert dist.shape == (32, 4000) and idx.shape == (32, 4000) and idx.dtype == torch.int64
        i64, _, gap = EI.nn_yardstick(s.double(), t.double())
        hard = gap < 2.0 ** -20
        skipped += int(hard.sum())
        total += hard.numel()
        assert torch.equal(idx[~hard], i64[~hard])
        at = ((s.double() - torch.gather(t.double(), 1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
        err = ((dist.double() - at).abs() / at).max().item()
        print("nn distance rel err %.3g (x 2^-24: %.2f), near ties %d" % (err, err * 2 ** 24, int(hard.sum())))
        assert err <= 8 * 2.0 ** -24
    assert skipped <= 1e-3 * total
    one = AE.get_NN(*pairs[0])
    assert torch.equal(one[0], outs[0][0]) and torch.equal(one[1], outs[0][1])


def test_nn_tie_rule_on_duplicate_targets():
    g = torch.Generator().manual_seed(3)
    src, trg = torch.randn(4, 300, 3, generator=g), torch.randn(4, 101, 3, generator=g)
    trg[:, 57] = trg[:, 9]
    trg[:, 100] = trg[:, 9]
    src[:, :40] = trg[:, 9:10] + 1e-3 * torch.randn(4, 40, 3, generator=g)
    trg[0, 3] = float("nan")
    dist, idx = AE.get_NN(src.to(DEV), trg.to(DEV))
    rd, ri = AE.nn_reference(src, trg)
    assert (idx[:, :40] == 9).all() and torch.equal(idx.cpu(), ri) and not (idx[0] == 3).any()
    assert rel_err(dist.cpu().numpy(), rd.numpy()) < 1e-6


def test_nn_backward_against_fp64_and_bitwise():
    pairs = [(s.to(DEV), t.to(DEV)) for s, t in EI.nn_inputs(EI.NN_SEED + 1, 32, 4000, 778)]
    ws = [torch.randn(32, 4000, generator=torch.Generator().manual_seed(7 + i)).to(DEV) for i in range(2)]

    def run():
        leaves = [(s.clone().requires_grad_(True), t.clone().requires_grad_(True)) for s, t in pairs]
        outs = AE.nn_many(leaves)
        sum((d * w).sum() for (d, _), w in zip(outs, ws)).backward()
        return outs, [(a.grad, b.grad) for a, b in leaves]
    outs, g1 = run()
    _, g2 = run()
    for (s, t), (_, idx), w, (ga, gb), (ga2, gb2) in zip(pairs, outs, ws, g1, g2):
        assert torch.equal(ga, ga2) and torch.equal(gb, gb2)
        a64, b64 = s.double().requires_grad_(True), t.double().requires_grad_(True)
        comp = ((a64 - torch.gather(b64, 1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
        (comp * w.double()).sum().backward()
        ea, eb = rel_err(ga.cpu().numpy(), a64.grad.cpu().numpy()), rel_err(gb.cpu().numpy(), b64.grad.cpu().numpy())
        print("nn backward rel err: src %.3g trg %.3g" % (ea, eb))
        assert ea < 1e-5 and eb < 1e-5
    only_src = pairs[0][0].clone().requires_grad_(True)
    AE.get_NN(only_src, pairs[0][1])[0].sum().backward()
    assert only_src.grad is not None


@pytest.mark.parametrize("case", list(EI.CASES))
def test_metric_kernel_on_the_fixture_cases(case, z, cpu_data, bounds):
    data = cpu_data[case]
    vals = AE.arctic_metrics(data.to(DEV))
    assert vals.shape == (6, SI.FIXTURE_B) and vals.dtype == torch.float32 and vals.is_cuda
    _check_rows(vals, AE.arctic_metrics_reference(data, torch.float64), bounds, case, data["targets.object.v_len"])
    for i, k in enumerate(AE.METRIC_KEYS):                         # and the reference's own NaN pattern / success rate
        ref = z["%s/metric/%s" % (case, k)]
        assert np.array_equal(np.isnan(vals[i].cpu().numpy()), np.isnan(ref)), k
        if k.startswith("success_rate"):
            ok = ~np.isnan(ref)
            assert np.array_equal(vals[i].cpu().numpy()[ok], ref[ok].astype(np.float32))


def _big():
    m = models(DEV, EI.BIG_LENGTHS)
    outputs, targets, meta = EI.to_device(*EI.case_inputs(lengths=EI.BIG_LENGTHS, **EI.BIG), DEV)
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    meta = dict(meta, obj_idx=idx, max_len=max_len)
    return outputs, targets, meta, m


def test_realistic_size_against_fp64_and_bitwise(bounds):
    outputs, targets, meta, m = _big()
    data = AE.prepare_data(EI.args(DEV), outputs, targets, meta, EI.CFG, flag="device", models=m)
    assert data["pred.object.v.cam"].shape[1] > 3900 and len(set(data["targets.object.v_len"].tolist())) > 3
    vals = AE.arctic_metrics(data)
    again = AE.arctic_metrics(data)
    assert torch.equal(torch.nan_to_num(vals, nan=-1.0), torch.nan_to_num(again, nan=-1.0))
    # fp64, from the data the kernel saw: every vertex is clear of its threshold, so the counts must be equal
    margin, _ = EI.success_margin(data["targets.object.v.cam"].cpu(), data["pred.object.v.cam"].cpu(),
                                  data["targets.object.v_len"].cpu(), data["meta_info.part_ids"].cpu(), data["meta_info.diameter"].cpu())
    print("smallest relative distance of a vertex from its success threshold: %.3g" % float(margin.min()))
    assert float(margin.min()) > EI.BIG_MARGIN
    success = vals[AE.METRIC_KEYS.index("success_rate/0.05")]
    assert ((success > 0) & (success < 100)).any()                       # frames with mixed outcomes are among them
    _check_rows(vals, AE.arctic_metrics_reference(data, torch.float64), bounds, "realistic", data["targets.object.v_len"])


@pytest.mark.parametrize("case", ["partial", "all_valid"])
def test_prepare_data_on_the_device_against_the_fixture(case, z):
    m = models(DEV)
    outputs, targets, meta = EI.to_device(*EI.case_inputs(case), DEV)
    data = AE.prepare_data(EI.args(DEV), outputs, targets, meta, EI.CFG, flag="device", models=m)
    assert list(data.keys()) == list(z[case + "/keys"])
    for k in z:
        if not k.startswith(case + "/data/"):
            continue
        kk = k.split("/data/")[1]
        got, ref = data[kk], z[k]
        assert got.is_cuda and tuple(got.shape) == ref.shape, kk
        if ref.dtype.kind == "f":
            assert rel_err(got.cpu().numpy(), ref) < 2e-4, kk
        else:
            assert np.array_equal(got.cpu().numpy(), ref), kk
    for h in ("r", "l"):                        # not fixtures: fp64 brute force on the same clouds
        src, trg = data["pred.object.v.cam"].double(), data["pred.mano.v3d.cam." + h].double()
        i64, _, gap = EI.nn_yardstick(src, trg)
        idx, dist = data["pred.nn_idx_" + h], data["pred.nn_dist_" + h]
        assert idx.dtype == torch.int64 and idx.shape == src.shape[:2]
        assert torch.equal(idx[gap >= 2.0 ** -20], i64[gap >= 2.0 ** -20])
        at = ((src - torch.gather(trg, 1, idx[..., None].expand(-1, -1, 3))) ** 2).sum(-1)
        assert ((dist.double() - at).abs() <= 8 * 2.0 ** -24 * at).all()
    cpu = AE.prepare_data(EI.args(DEV), outputs, targets, meta, EI.CFG, flag="eval", models=m)
    assert all(not v.is_cuda for v in cpu.values() if torch.is_tensor(v))


def test_sync_counts_and_launches():
    from torch.profiler import ProfilerActivity, profile

    outputs, targets, meta, m = _big()
    args = EI.args(DEV)
    ev = AE.ArcticEvaluator()

    def step():
        data = AE.prepare_data(args, outputs, targets, meta, EI.CFG, flag="device", models=m)
        ev.update(data)
        return data
    data = step()                                    # warm-up: conversions, library load, the evaluator's totals
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            stats = AE.measure_error(data, list(AE.DEFAULT_METRICS))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len([w for w in caught if "synchroniz" in str(w.message)]) == 1
    assert list(stats) == list(AE.METRIC_KEYS)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert count("nn_fwd_kernel") == 1 and count("arctic_metrics_kernel") == 1 and count("arctic_metrics_accumulate_kernel") == 1
    assert count("mano_fwd_kernel") == 1 and count("obj_fwd_kernel") == 1


def test_update_captures_in_a_graph(cpu_data):
    data = cpu_data["partial"].to(DEV)
    eager, graphed = AE.ArcticEvaluator(), AE.ArcticEvaluator()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graphed.update(data)                         # warm-up allocates the totals
    torch.cuda.current_stream().wait_stream(s)
    graphed.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.update(data)
    graphed.reset()
    for _ in range(3):
        graph.replay()
        eager.update(data)
    torch.cuda.synchronize()
    assert torch.equal(graphed.total, eager.total) and torch.equal(graphed.count, eager.count)
    assert float(eager.count[0]) == 3 and graphed.compute() == eager.compute()


def test_evaluator_against_the_engine_style_means(z, cpu_data, bounds):
    ev = AE.ArcticEvaluator()
    for case in EI.SEQUENCE:
        ev.update(cpu_data[case].to(DEV))
    out = ev.compute()
    assert list(out) == list(AE.METRIC_KEYS)
    for k in AE.METRIC_KEYS:
        ref = float(z["avg/" + k])
        print("avg %-18s %.6f reference %.6f" % (k, out[k], ref))
        assert abs(out[k] - ref) <= bounds[k] * abs(ref), k
    assert float(ev.count[AE.METRIC_KEYS.index("cdev/ho")]) == 4


@pytest.mark.parametrize("trigger", ["env", "fp64"])
def test_fallbacks_give_the_restatements(trigger, monkeypatch, cpu_data):
    data = cpu_data["partial"].to(DEV)
    (s, t), = EI.nn_inputs(9, 2, 100, 30, pairs=1)
    s, t = s.to(DEV), t.to(DEV)
    if trigger == "env":
        monkeypatch.setenv("MSDA_ARCTIC_EVAL_FUSED", "0")
    else:
        s, t = s.double(), t.double()
        data = AE.XDict({k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in data.items()})
    AE._WARNED.clear()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        d, i = AE.get_NN(s, t)
        a = AE.arctic_metrics(data)
        AE.arctic_metrics(data)
    # a missed kernel is named once per cause; the A/B knob is the user's own choice and stays silent
    told = [str(w.message) for w in caught if "torch restatement" in str(w.message)]
    assert len(told) == (0 if trigger == "env" else 2) and all("float64" in m for m in told), told
    rd, ri = AE.nn_reference(s, t)
    assert torch.equal(d, rd) and torch.equal(i, ri) and d.dtype == s.dtype
    r = AE.arctic_metrics_reference(data).float()
    assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(r, nan=-1.0))


def test_pairs_of_different_shapes_keep_the_kernels():
    from torch.profiler import ProfilerActivity, profile

    (a, b), (c, d) = EI.nn_inputs(11, 4, 500, 200)
    (_, e), = EI.nn_inputs(12, 4, 500, 90, pairs=1)
    pairs = [(a.to(DEV), b.to(DEV)), (c.to(DEV), e.to(DEV)), (c.to(DEV), d.to(DEV))]
    AE.nn_many(pairs)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            outs = AE.nn_many(pairs)
            torch.cuda.synchronize()
    assert not [w for w in caught if "torch restatement" in str(w.message)]
    names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    assert sum("nn_fwd_kernel" in n for n in names) == 2          # the two N2 = 200 pairs share one launch
    for (s, t), (dist, idx) in zip(pairs, outs):
        i64, _, gap = EI.nn_yardstick(s.double(), t.double())
        assert idx.shape == (4, 500) and torch.equal(idx[gap >= 2.0 ** -20], i64[gap >= 2.0 ** -20])
