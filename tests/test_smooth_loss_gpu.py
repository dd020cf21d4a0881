"""The SmoothNet criterion's losses on the MI355X (csrc/msda_smooth_loss.hip) against ``smooth_loss_reference(dtype=float64)``
on the same fp32 inputs.

Shapes.  The fixture cases of tests/golden/smooth_loss_inputs.py: N = 6 (five validity patterns), 8 (coherent), 1, 2, 3 and the
pattern without a valid centre frame, objects padded to a few hundred rows (no multiple of the 256- or 512-thread workgroups, nor are the 778
hand vertices: the input fixture asserts it); two variants of ``all_valid``: an object with exactly one bottom row, and a contact index hit by 70 hand
vertices of both hands while most object rows are hit by none.  One realistic case: arctic_eval_inputs.BIG (N = 32, objects
of about 4000 rows), with its own validity pattern (no hand counts) and with all frames valid.

Tolerances, measured at test time on the CPU and printed.  Values, per key: max(4 x the deviation of the reference-run fp32
fixture from the fp64 restatement, 16 x 2^-24), relative to the key's largest value (the scalar itself; the largest per-frame
entry for eval_acc_pose's arrays).  The factor 4 covers the same number of fp32 operations in another order, plus FMA.
Gradients, per tensor: max(4 x the deviation of the CPU fp32 restatement's autograd from the fp64 autograd on the same
inputs, 1e-5), relative to the tensor's largest entry.  The NaN pattern of the per-frame arrays and the zero pattern of the
losses are identical.

Values found on the MI355X when this was written, in units of 2^-24.  Fixture deviations from fp64: loss/cd 1.27, acc/h 1.76,
acc/o 94.71 (the reference rounds the object root, a mean of a few hundred coordinates near z = 12 m, to fp32, and the stencil
multiplies by 900), giving the bounds 16, 16 and 378.8.  The kernels, largest over all cases: loss/cd 2.70, acc/h 1.17,
acc/o 1.47 (the kernels keep the object root in fp64); at N = 32 with objects of 4000 rows 1.17, 0.69 and 0.28.
Gradients: the object vertices' with acc_grad are ill-conditioned in fp32 where a difference vector is small: the CPU fp32
autograd deviates by 9e-5 (N = 3) to 1.2e-2 (N = 32), so the bounds there are 3.7e-4 to 4.8e-2, and the kernels measured
at most 5.5e-5; every other gradient has the floor 1e-5 as its bound and measured 3e-8 to 5.3e-6.

Launches: three forward and one backward whatever the data holds; no host sync; a captured graph replays the eager result
bit for bit; two runs are bitwise equal."""
import sys
import types
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import arctic_eval_inputs as EI  # noqa: E402
import smooth_loss_inputs as MI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd import arctic_eval as AE  # noqa: E402
from uvhand_amd import smooth_loss as SL  # noqa: E402
from uvhand_amd.modules import ArcticSmoother, SmoothCriterion  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOOR = 16 * 2.0 ** -24
GRAD_FLOOR = 1e-5
W = {"loss/cd": 10.0, "acc/h": 1.3, "acc/o": 0.7}
VARIANTS = ("one_bottom", "shared_idx")


@pytest.fixture(scope="module")
def z():
    return load_golden("smooth_loss")


def _variant(name, pred, gt):
    gt = AE.XDict(gt)
    if name == "one_bottom":
        ids = gt["object.parts_ids"].clone()
        bottom = (ids[0] == 2).nonzero().view(-1)
        ids[0, bottom[1:]] = 1
        gt.overwrite("object.parts_ids", ids)
    elif name == "shared_idx":
        iro, ilo, dro, dlo = (gt[k].clone() for k in ("idx.ro", "idx.lo", "dist.ro", "dist.lo"))
        iro[:, :40], ilo[:, :30] = 7, 7
        dro[:, :40], dlo[:, :30] = 1e-3, 1e-3
        for k, v in (("idx.ro", iro), ("idx.lo", ilo), ("dist.ro", dro), ("dist.lo", dlo)):
            gt.overwrite(k, v)
    return pred, gt


@pytest.fixture(scope="module")
def cpu_inputs():
    m = MI.models()
    out = {case: MI.case_inputs(case, m) for case in MI.CASES}
    for v in VARIANTS:
        out[v] = _variant(v, *out["all_valid"])
    for pred, _ in out.values():                     # the tail of a strided loop: neither kernel block size divides the rows
        L, NV = pred["object.v.cam"].shape[1], pred["mano.v3d.cam.r"].shape[1]
        assert L % 256 != 0 and L % 512 != 0 and NV % 256 != 0 and (2 * NV) % 512 != 0
    assert sorted({gt["is_valid"].shape[0] for _, gt in out.values()}) == [1, 2, 3, 6, 8]
    return out


@pytest.fixture(scope="module")
def big():
    """arctic_eval_inputs.BIG with the gt hand vertices: (pred, gt) on the CPU, and the same with every frame valid."""
    pred, gt = MI.case_inputs(EI.BIG["case"], MI.models(lengths=EI.BIG_LENGTHS), B=EI.BIG["B"], lengths=EI.BIG_LENGTHS,
                              seed=EI.BIG["seed"])
    ones = torch.ones(EI.BIG["B"])
    valid = AE.XDict(gt)
    for k in ("is_valid", "left_valid", "right_valid"):
        valid.overwrite(k, ones.clone())
    return {"big": (pred, gt), "big_valid": (pred, valid)}


def _dev(d):
    return AE.XDict({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()})


@pytest.fixture(scope="module")
def bounds(z, cpu_inputs):
    """Per key: max(4 x the fixture's deviation from the fp64 restatement, 16 x 2^-24), measured here on the CPU."""
    dev = {k: 0.0 for k in SL.KEYS}
    for case in MI.CASES:
        pred, gt = cpu_inputs[case]
        r64 = SL.smooth_loss_reference(pred, gt, dtype=torch.float64)
        rows = SL._acc_rows(pred, gt, torch.float64)
        for k in SL.KEYS:
            name = "%s/loss/%s" % (case, k)
            if name in z and float(r64[k]) != 0.0:
                dev[k] = max(dev[k], abs(float(z[name]) - float(r64[k])) / abs(float(r64[k])))
        for k, row in zip(("acc/h", "acc/o"), rows or ()):
            name = "%s/eval/%s" % (case, k)
            ok = ~np.isnan(z[name]) if name in z else np.zeros(0, dtype=bool)
            if ok.any():
                dev[k] = max(dev[k], rel_err(z[name][ok], row.numpy()[ok]))
    print("fixture deviations from fp64 (x 2^-24):", {k: round(v * 2 ** 24, 2) for k, v in dev.items()})
    return {k: max(4 * v, FLOOR) for k, v in dev.items()}


def _total(out):
    return sum(W[k] * out[k] for k in SL.KEYS)


def _grads64(pred, gt, acc_grad, dtype=torch.float64):
    p, ls = MI.leaves(pred, dtype=dtype)
    _total(SL.smooth_loss_reference(p, gt, dtype=dtype, acc_grad=acc_grad)).backward()
    return [torch.zeros_like(t) if t.grad is None else t.grad for t in ls]


def _run(pred, gt, acc_grad):
    p, ls = MI.leaves(pred)
    out = SL.compute_smoothnet_loss(p, gt, None, None, 224, acc_grad=acc_grad)
    _total(out).backward()
    return out, [torch.zeros_like(t) if t.grad is None else t.grad for t in ls]


def _check_values(what, out, r64, bounds):
    for k in SL.KEYS:
        got, ref = float(out[k].detach()), float(r64[k])
        assert out[k].dtype == torch.float32 and out[k].dim() == 0 and out[k].device.type == "cuda"
        assert (got == 0.0) == (ref == 0.0) and np.isfinite(got), (what, k, got, ref)
        err = abs(got - ref) / abs(ref) if ref else 0.0
        print("%s %-8s rel err %.3g (x 2^-24: %.2f, bound %.2f)" % (what, k, err, err * 2 ** 24, bounds[k] * 2 ** 24))
        assert err <= bounds[k], (what, k, err)


def _check_grads(what, pred, gt, grads, acc_grad):
    g64 = _grads64(pred, gt, acc_grad)
    g32 = _grads64(pred, gt, acc_grad, dtype=torch.float32)
    for k, g, a, b in zip(MI.PRED_LEAVES, grads, g64, g32):
        top = float(a.abs().max())
        if top == 0.0:
            assert not g.any(), (what, k)
            continue
        dev32 = float((b.double() - a).abs().max()) / top
        bound = max(4 * dev32, GRAD_FLOOR)
        err = float((g.double().cpu() - a).abs().max()) / top
        print("%s grad %-16s acc_grad=%d rel err %.3g (cpu fp32 %.3g, bound %.3g)" % (what, k, acc_grad, err, dev32, bound))
        assert err <= bound, (what, k, err, bound)


@pytest.mark.parametrize("case", MI.CASES + list(VARIANTS))
def test_values_and_per_frame_rows_against_fp64(case, cpu_inputs, bounds):
    pred, gt = cpu_inputs[case]
    r64 = SL.smooth_loss_reference(pred, gt, dtype=torch.float64)
    dp, dg = _dev(pred), _dev(gt)
    before = _native.launch_count()
    out = SL.compute_smoothnet_loss(dp, dg, None, None, 224)
    assert _native.launch_count() - before == 3 and tuple(out.keys()) == SL.KEYS
    _check_values(case, out, r64, bounds)
    ev = SL.eval_acc_pose(dp, dg, None)
    N = gt["is_valid"].shape[0]
    assert ev["acc/h"].shape == (N,) and ev["acc/o"].shape == (max(N - 2, 0),) and ev["acc/h"].dtype == np.float32
    rows = SL._acc_rows(pred, gt, torch.float64)
    if rows is None:
        assert np.isnan(ev["acc/h"]).all()
        return
    for k, row in zip(("acc/h", "acc/o"), rows):
        ref = row.numpy()
        assert np.array_equal(np.isnan(ev[k]), np.isnan(ref)), (case, k)
        ok = ~np.isnan(ref)
        if ok.any():
            assert rel_err(ev[k][ok], ref[ok]) <= bounds[k], (case, k)


@pytest.mark.parametrize("acc_grad", [False, True])
@pytest.mark.parametrize("case", ["all_valid", "partial", "left_invalid", "coherent", "n1", "n2", "n3", "no_centre", "one_bottom", "shared_idx"])
def test_gradients_against_fp64_bitwise_and_launch_counts(case, acc_grad, cpu_inputs):
    pred, gt = cpu_inputs[case]
    dp, dg = _dev(pred), _dev(gt)
    _run(dp, dg, acc_grad)
    before = _native.launch_count()
    out, grads = _run(dp, dg, acc_grad)
    assert _native.launch_count() - before == 3 + 1
    out2, grads2 = _run(dp, dg, acc_grad)
    assert all(torch.equal(out[k], out2[k]) for k in SL.KEYS)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert out["acc/h"].requires_grad == acc_grad and out["acc/o"].requires_grad == acc_grad
    off = SL.compute_smoothnet_loss(dp, dg, None, None, 224, acc_grad=not acc_grad)
    assert all(torch.equal(out[k], off[k]) for k in SL.KEYS)
    _check_grads(case, pred, gt, grads, acc_grad)
    if not acc_grad:
        assert not grads[2].any() and not grads[3].any()


def test_realistic_size(big, bounds):
    for name, (pred, gt) in big.items():
        assert pred["object.v.cam"].shape[1] >= 3900 and gt["is_valid"].shape[0] == 32
        r64 = SL.smooth_loss_reference(pred, gt, dtype=torch.float64)
        dp, dg = _dev(pred), _dev(gt)
        for acc_grad in (False, True):
            out, grads = _run(dp, dg, acc_grad)
            out2, grads2 = _run(dp, dg, acc_grad)
            assert all(torch.equal(out[k], out2[k]) for k in SL.KEYS) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
            _check_values(name, out, r64, bounds)
            _check_grads(name, pred, gt, grads, acc_grad)
    assert float(SL.smooth_loss_reference(*big["big_valid"], dtype=torch.float64)["acc/h"]) > 0


def test_no_host_sync(big):
    pred, gt = big["big_valid"]
    dp, dg = _dev(pred), _dev(gt)
    _run(dp, dg, True)                               # warm-up: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run(dp, dg, True)
        _run(dp, dg, False)
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.parametrize("acc_grad", [False, True])
def test_graph_capture_equals_eager(acc_grad, cpu_inputs):
    pred, gt = cpu_inputs["coherent"]
    dp, dg = _dev(pred), _dev(gt)
    p, ls = MI.leaves(dp)

    def step():
        for t in ls:
            t.grad = None
        out = SL.compute_smoothnet_loss(p, dg, None, None, 224, acc_grad=acc_grad)
        _total(out).backward()
        return [out[k].detach() for k in SL.KEYS] + [t.grad for t in ls]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(s)
    eager = [None if t is None else t.clone() for t in eager]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def _same_as_restatement(pred, gt, **kw):
    before = _native.launch_count()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = SL.compute_smoothnet_loss(pred, gt, None, None, 224, **kw)
    assert _native.launch_count() == before, "a fallback trigger reached the kernels"
    want = SL.smooth_loss_reference(pred, gt, dtype=torch.float32, **kw)
    assert all(torch.equal(got[k], want[k]) and got[k].dtype == torch.float32 for k in SL.KEYS)
    return [str(w.message) for w in caught]


def test_every_fallback_trigger_gives_the_restatement(cpu_inputs, monkeypatch):
    pred, gt = cpu_inputs["all_valid"]
    dp, dg = _dev(pred), _dev(gt)
    assert _same_as_restatement(pred, gt) == []                                          # CPU tensors: silent
    monkeypatch.setenv("MSDA_SMOOTH_LOSS_FUSED", "0")
    assert _same_as_restatement(dp, dg) == []                                            # the knob: silent
    monkeypatch.delenv("MSDA_SMOOTH_LOSS_FUSED")
    SL._WARNED.clear()
    p64 = AE.XDict(dp)
    p64.overwrite("object.v.cam", dp["object.v.cam"].double())
    msgs = _same_as_restatement(p64, dg)
    assert len(msgs) == 1 and "'pred.object.v.cam'" in msgs[0] and "float64" in msgs[0]
    assert _same_as_restatement(p64, dg) == []                                           # warns once per cause
    g32 = AE.XDict(dg)
    g32.overwrite("idx.ro", dg["idx.ro"].int())
    msgs = _same_as_restatement(dp, g32)
    assert len(msgs) == 1 and "'targets.idx.ro'" in msgs[0] and "int64" in msgs[0]
    gh = AE.XDict(dg)
    gh.overwrite("is_valid", dg["is_valid"].half())                                      # mismatched dtypes
    assert any("'targets.is_valid'" in m for m in _same_as_restatement(dp, gh))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert any("autocast" in m for m in _same_as_restatement(dp, dg))
    # over a kernel limit: 1025 hand vertices
    n, nv = 3, 1025
    g = torch.Generator().manual_seed(3)
    wide_p, wide_g = AE.XDict(dp), AE.XDict(dg)
    for s in ("r", "l"):
        wide_p.overwrite("mano.v3d.cam." + s, torch.randn(n, nv, 3, generator=g).to(DEV))
        wide_g.overwrite("mano.v3d.cam." + s, torch.randn(n, nv, 3, generator=g).to(DEV))
    for k in ("ro", "lo"):
        wide_g.overwrite("dist." + k, (6e-3 * torch.rand(n, nv, generator=g)).to(DEV))
        wide_g.overwrite("idx." + k, torch.randint(0, 100, (n, nv), generator=g).to(DEV))
    for d in (wide_p, wide_g):
        for k in list(d):
            if torch.is_tensor(d[k]) and d[k].shape[:1] == (6,):
                d.overwrite(k, d[k][:n].contiguous())
    assert any("msda_smooth_loss_supported" in m for m in _same_as_restatement(wide_p, wide_g))
    # a prediction and a gt object of different padded length: the restatement, which raises as torch does
    short = AE.XDict(dp)
    short.overwrite("object.v.cam", dp["object.v.cam"][:, :-1].contiguous())
    before = _native.launch_count()
    with pytest.raises((IndexError, RuntimeError)), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        SL.compute_smoothnet_loss(short, dg, None, None, 224)
    assert _native.launch_count() == before


def test_smooth_criterion_on_a_training_step(z, bounds):
    """ArcticSmoother -> make_output -> prepare_data(flag='train') -> SmoothCriterion -> backward, as engine.py:357-403."""
    m = MI.models(DEV)
    outputs, gt, meta = EI.to_device(*MI.raw_inputs("all_valid"), DEV)
    args = EI.args(DEV)
    obj_idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    items = AE.get_arctic_item(outputs, EI.CFG, DEV)
    leaves = [[t.detach().clone().requires_grad_(True) for t in grp] for grp in items]
    torch.manual_seed(0)
    smoother = ArcticSmoother(2, 3).to(DEV).eval()
    weights = {"loss/cd": 10.0, "acc/h": 1, "acc/o": 1}
    crit = SmoothCriterion(2, 3, weights, m).to(DEV)

    def step():
        smoothed = smoother(leaves)
        pred = AE.make_output(args, *smoothed, meta["query_names"], meta["intrinsics"], models=m, obj_idx=obj_idx, max_len=max_len)
        data = AE.prepare_data(args, None, gt, meta, EI.CFG, pred=pred, flag="train", models=m)
        return data, crit(args, data, gt, meta)
    data, losses = step()
    assert list(losses.keys()) == list(z["all_valid/keys"]) == list(SL.KEYS)
    assert all(v.dim() == 0 and v.dtype == torch.float32 for v in losses.values())
    cpu = AE.XDict({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in data.items()})
    r64 = SL.smooth_loss_reference(cpu.search("pred.", ""), cpu.search("targets.", ""), dtype=torch.float64)
    for k in SL.KEYS:
        assert abs(float(losses[k]) - float(r64[k])) <= bounds[k] * abs(float(r64[k])), k
    sum(losses[k] * weights[k] for k in losses if k in weights).backward()
    for grp in leaves:
        for t in grp:
            assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0
    assert all(p.grad is not None for p in smoother.parameters())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, losses = step()
        sum(losses[k] * weights[k] for k in losses if k in weights).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
