"""The SmoothNet criterion's losses on the CPU (uvhand_amd/smooth_loss.py): the torch restatement against
tests/golden/smooth_loss.npz, which gen_smooth_loss.py made by running the reference's own compute_smoothnet_loss,
eval_acc_pose, compute_error_accel, compute_contact_devi_loss, contact_deviation and nanmean; the reference behaviours the
drop-in keeps and its stated deviations, one assertion each; ``acc_grad``.

Tolerances.  The inputs are rebuilt at test time by the package's CPU MANO / object chain, whose matrix products depend on
the BLAS thread count: a hand coordinate at z of 10 to 20 m is reproducible to one fp32 ulp there, u = 2^-19 m, not always
bitwise (measured: 9.5e-7 m between 1 and 2 threads; the object chain has no matrix product and is bitwise).  The fixture
therefore holds checksums of the ten vertex and joint tensors the reference run read, and the bounds are measured:
  ``acc/*`` on bitwise the generator's inputs (scalars and per-frame rows): the fp32 restatement runs the reference's torch
  operations in its order, so it is held to 16 x 2^-24 relative (measured 0); the fp64 restatement is held to
  max(4 x the fp32 restatement's own deviation from it, 16 x 2^-24): the reference's fp32 run may be as far from the exact
  value as this fp32 run, times the factor 4 that the GPU test grants another order of the same operations.
  Where the rebuilt inputs differ from the generator's (another thread count), an allowance for one ulp of every coordinate
  is added: the stencil [1, -2, 1] * 900 carries u to 4 * 900 u per component for the prediction and as much for the gt, so a
  norm, and every mean of norms, moves by at most sqrt(3) * 7200 * 2^-19 = 0.0238 m/s^2.
  ``loss/cd``: a contact distance moves by at most sqrt(3) * 2 u when both its end points move by u, and so does every mean of
  distances; two hands: 4 sqrt(3) u = 1.3e-5 m, plus 16 x 2^-24 relative for the rounding (measured on identical inputs: 0 in
  fp32, 1.3 x 2^-24 in fp64).
  Gradients of 10 * loss/cd: a unit vector d / |d| turns by at most 2 |delta d| / |d| <= 8 u / |d|; the bound is
  max(1e-5, 8 u / the case's smallest contact distance, taken in fp64 from the inputs), relative to the tensor's largest entry.
Finite differences (fp64, step 1e-6 m, central): 1e-6 relative to the largest gradient entry probed, the truncation error of a
norm of O(1) curvature being 1e-12."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import smooth_loss_inputs as MI  # noqa: E402
import uvhand_amd  # noqa: E402
from uvhand_amd import arctic_eval as AE  # noqa: E402
from uvhand_amd import smooth_loss as SL  # noqa: E402
from uvhand_amd.modules import SmoothCriterion  # noqa: E402

TOL = 16 * 2.0 ** -24
U = 2.0 ** -19
ACC_IN = 3 ** 0.5 * 7200 * U             # added only where the rebuilt inputs are not bitwise the generator's
CD_ABS = 4 * 3 ** 0.5 * U
NAN = float("nan")


@pytest.fixture(scope="module")
def z():
    return load_golden("smooth_loss")


@pytest.fixture(scope="module")
def inputs():
    m = MI.models()
    return {case: MI.case_inputs(case, m) for case in MI.CASES}


def _with(d, **kw):
    out = AE.XDict(d)
    for k, v in kw.items():
        out.overwrite(k.replace("__", "."), v)
    return out


def _input_allowance(z, case, pred, gt):
    """0 where the rebuilt vertex and joint tensors are bitwise the ones the reference run read, else ACC_IN."""
    same = all(np.array_equal(z["%s/insum/%s/%s" % (case, side, k)], MI.checksum(d[k]))
               for side, d in (("pred", pred), ("gt", gt)) for k in MI.PRED_LEAVES)
    return 0.0 if same else ACC_IN


def _ref_value(z, case, k):
    """The fixture's value of a key; 0 where the reference raises (N < 3) and the drop-in returns zero."""
    name = "%s/loss/%s" % (case, k)
    return float(z[name]) if name in z else 0.0


@pytest.mark.parametrize("case", MI.CASES)
def test_restatement_against_the_reference(case, inputs, z):
    pred, gt = inputs[case]
    r32 = SL.smooth_loss_reference(pred, gt)
    r64 = SL.smooth_loss_reference(pred, gt, dtype=torch.float64)
    assert tuple(r32.keys()) == SL.KEYS == ("loss/cd", "acc/h", "acc/o")
    if case + "/raises" not in z:
        assert list(z[case + "/keys"]) == list(SL.KEYS)
    extra = _input_allowance(z, case, pred, gt)
    for k in SL.KEYS:
        ref = _ref_value(z, case, k)
        assert r32[k].dtype == torch.float32 and r32[k].dim() == 0 and r64[k].dtype == torch.float64
        if k == "loss/cd":
            b32 = b64 = CD_ABS + TOL * abs(ref)
        else:
            b32 = TOL * abs(ref) + extra
            b64 = max(4 * abs(float(r32[k]) - float(r64[k])), TOL * abs(ref)) + extra
        print("%s %-8s fp32 %.3g fp64 %.3g (bounds %.3g, %.3g)" % (case, k, abs(float(r32[k]) - ref), abs(float(r64[k]) - ref), b32, b64))
        assert abs(float(r32[k]) - ref) <= b32, (k, float(r32[k]), ref)
        assert abs(float(r64[k]) - ref) <= b64, (k, float(r64[k]), ref)
        assert (float(r64[k]) == 0.0) == (ref == 0.0) == (float(r32[k]) == 0.0)


@pytest.mark.parametrize("case", MI.CASES)
def test_eval_acc_pose_against_the_reference(case, inputs, z):
    pred, gt = inputs[case]
    out = SL.eval_acc_pose(pred, gt, None)
    N = gt["is_valid"].shape[0]
    assert list(out.keys()) == ["acc/h", "acc/o"] and all(isinstance(v, np.ndarray) for v in out.values())
    assert out["acc/h"].shape == (N,) and out["acc/o"].shape == (max(N - 2, 0),)
    assert np.isnan(out["acc/h"][0]) and np.isnan(out["acc/h"][-1])
    if case + "/raises" in z:
        assert N < 3 and np.isnan(out["acc/h"]).all()
        return
    for k in ("acc/h", "acc/o"):
        ref = z["%s/eval/%s" % (case, k)]
        assert out[k].shape == ref.shape and out[k].dtype == ref.dtype == np.float32
        assert np.array_equal(np.isnan(out[k]), np.isnan(ref)), k
        ok = ~np.isnan(ref)
        if ok.any():
            bound = TOL * np.abs(ref[ok]).max() + _input_allowance(z, case, pred, gt)
            assert np.abs(out[k][ok].astype(np.float64) - ref[ok]).max() <= bound, k


def _smallest_contact(pred, gt):
    """fp64: the smallest distance of a counted contact (inf: none)."""
    best = float("inf")
    for s, k, v in (("r", "ro", "right_valid"), ("l", "lo", "left_valid")):
        vo, vh = pred["object.v.cam"].double(), pred["mano.v3d.cam." + s].double()
        d = (torch.gather(vo, 1, gt["idx." + k][:, :, None].repeat(1, 1, 3)) - vh).norm(dim=2)
        on = (gt["dist." + k] <= 3e-3) & ((gt[v] * gt["is_valid"]) == 1)[:, None]
        if on.any():
            best = min(best, float(d[on].min()))
    return best


@pytest.mark.parametrize("case", MI.CASES)
def test_contact_gradient_against_the_reference(case, inputs, z):
    pred, gt = inputs[case]
    p, ls = MI.leaves(pred)
    (10 * SL.smooth_loss_reference(p, gt)["loss/cd"]).backward()
    bound = max(1e-5, 8 * U / _smallest_contact(pred, gt))
    for k, t in zip(MI.PRED_LEAVES, ls):
        ref = z["%s/grad/%s" % (case, k)]
        grad = torch.zeros_like(t) if t.grad is None else t.grad
        got = grad[:, :MI.grad_rows(t.shape[0])].numpy()
        assert got.shape == ref.shape
        if np.abs(ref).max() > 0:
            assert rel_err(got, ref) <= bound, (k, bound)
        else:
            assert not got.any(), k
        total = float(z["%s/gradsum/%s" % (case, k)])
        assert abs(float(grad.double().abs().sum()) - total) <= bound * total


def test_compute_error_accel_is_the_stencil_times_fps_squared():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(5, 7, 3, generator=g, dtype=torch.float64), torch.randn(5, 7, 3, generator=g, dtype=torch.float64)
    d = b - a
    want = ((d[:-2] - 2 * d[1:-1] + d[2:]) * 900.0).norm(dim=2).mean(dim=1)
    assert torch.allclose(SL.compute_error_accel(a, b), want, rtol=1e-12, atol=0)
    assert torch.allclose(SL.compute_error_accel(a, b, fps=60.0), want * 4, rtol=1e-12, atol=0)


# ---- reference behaviours the drop-in keeps ---------------------------------------------------------------------------------------
def _acc64(pred, gt):
    """Manual fp64: (acc_r, acc_l, acc_o) [N - 2] without validity."""
    d = lambda t: t.double()  # noqa: E731
    bottom = gt["object.parts_ids"][0] == 2
    rows = []
    for k, rp, rg in (("mano.v3d.cam.r", d(pred["mano.j3d.cam.r"])[:, :1], d(gt["mano.j3d.cam.r"])[:, :1]),
                      ("mano.v3d.cam.l", d(pred["mano.j3d.cam.l"])[:, :1], d(gt["mano.j3d.cam.l"])[:, :1]),
                      ("object.v.cam", d(pred["object.v.cam"])[:, bottom].mean(1, keepdim=True), d(gt["object.v.cam"])[:, bottom].mean(1, keepdim=True))):
        e = (d(pred[k]) - rp) - (d(gt[k]) - rg)
        rows.append(((e[:-2] - 2 * e[1:-1] + e[2:]) * 900.0).norm(dim=2).sum(dim=1) / e.shape[1])
    return rows


def test_accelerations_cross_window_boundaries(inputs):
    """N = 6 is B = 2 windows of T = 3: the centre frames 2 and 3 straddle the boundary and count like any other."""
    pred, gt = inputs["all_valid"]
    out = SL.eval_acc_pose(pred, gt, None)
    assert not np.isnan(out["acc/o"]).any() and not np.isnan(out["acc/h"][1:-1]).any()
    assert rel_err(out["acc/o"], _acc64(pred, gt)[2].numpy()) < 1e-3


def test_the_error_is_the_mean_over_all_padded_columns(inputs):
    pred, gt = inputs["coherent"]
    r64 = SL.smooth_loss_reference(pred, gt, dtype=torch.float64)
    acc_r, acc_l, acc_o = _acc64(pred, gt)                           # divides by shape[1], padding included
    assert abs(float(r64["acc/o"]) - float(acc_o.mean())) <= 1e-12 * float(acc_o.mean())
    assert (gt["object.v_len"] < gt["object.v.cam"].shape[1]).any()


def test_acc_h_is_the_per_frame_nanmean_of_the_hands_then_over_frames(inputs):
    pred, gt = inputs["coherent"]
    lv = gt["left_valid"].clone()
    lv[3] = 0.0                                                      # the left hand drops out of centre frames 2, 3, 4
    r64 = SL.smooth_loss_reference(pred, _with(gt, left_valid=lv), dtype=torch.float64)
    acc_r, acc_l, _ = _acc64(pred, gt)
    per_frame = [(acc_r[i] + acc_l[i]) / 2 if i + 1 not in (2, 3, 4) else acc_r[i] for i in range(6)]
    want = float(sum(per_frame) / 6)
    assert abs(float(r64["acc/h"]) - want) <= 1e-12 * want


def test_a_half_flag_invalidates_a_centre_frame_and_truncation_keeps_one_above(inputs):
    pred, gt = inputs["coherent"]
    half = gt["is_valid"].clone()
    half[3] = 0.5
    out = SL.eval_acc_pose(pred, _with(gt, is_valid=half), None)
    assert np.isnan(out["acc/o"][1:4]).all() and not np.isnan(out["acc/o"][[0, 4, 5]]).any()
    above = gt["is_valid"].clone()
    above[3] = 1.25                                                  # 1 + 1.25 + 1 truncates to 3: valid for the accelerations
    out = SL.eval_acc_pose(pred, _with(gt, is_valid=above), None)
    assert not np.isnan(out["acc/o"]).any()
    # ... while the contact deviation keeps (1 - valid) != 0: frame 3 is out, exactly as with a flag of 0
    zero = gt["is_valid"].clone()
    zero[3] = 0.0
    cd = lambda v: SL.smooth_loss_reference(pred, _with(gt, is_valid=v))["loss/cd"]  # noqa: E731
    assert torch.equal(cd(above), cd(zero)) and not torch.equal(cd(above), cd(gt["is_valid"]))


def test_the_object_root_uses_frame_zeros_part_ids_over_the_padded_length(inputs):
    pred, gt = inputs["all_valid"]
    base = SL.smooth_loss_reference(pred, gt, dtype=torch.float64)["acc/o"]
    ids = gt["object.parts_ids"].clone()
    ids[1:] = 1                                                      # the other frames' ids are never read
    assert torch.equal(SL.smooth_loss_reference(pred, _with(gt, object__parts_ids=ids), dtype=torch.float64)["acc/o"], base)
    ids = gt["object.parts_ids"].clone()
    pad = int(gt["object.v_len"][0])
    assert pad < ids.shape[1]
    ids[0, -1] = 2                                                   # a padded column of frame 0 joins every frame's root
    assert not torch.equal(SL.smooth_loss_reference(pred, _with(gt, object__parts_ids=ids), dtype=torch.float64)["acc/o"], base)


def test_loss_cd_adds_the_two_hands_nan_to_num(inputs, z):
    pred, gt = inputs["no_contact"]
    assert float(SL.smooth_loss_reference(pred, gt)["loss/cd"]) == 0.0 == float(z["no_contact/loss/loss/cd"])
    pred, gt = inputs["all_valid"]
    f = lambda t: t.double()  # noqa: E731
    parts = [torch.nan_to_num(SL._nanmean(SL.contact_deviation(f(pred["object.v.cam"]), f(pred["mano.v3d.cam." + s]), f(gt["dist." + k]),
                                                                gt["idx." + k], f(gt["is_valid"]), f(gt[v]))))
             for s, k, v in (("r", "ro", "right_valid"), ("l", "lo", "left_valid"))]
    got = SL.smooth_loss_reference(pred, gt, dtype=torch.float64)["loss/cd"]
    assert float(got) == float(parts[0] + parts[1]) and float(parts[0]) > 0 and float(parts[1]) > 0


# ---- stated deviations --------------------------------------------------------------------------------------------------------------
def test_no_valid_centre_frame_gives_fp32_zeros_where_the_reference_gives_int64(inputs, z):
    pred, gt = inputs["no_centre"]
    assert str(z["no_centre/dtype/acc/h"]) == "torch.int64" and float(z["no_centre/loss/acc/h"]) == 0.0
    p, ls = MI.leaves(pred)
    out = SL.compute_smoothnet_loss(p, gt, None, None, 224, acc_grad=True)
    for k in ("acc/h", "acc/o"):
        assert out[k].dtype == torch.float32 and out[k].dim() == 0 and float(out[k]) == 0.0
    assert float(out["loss/cd"].detach()) > 0
    sum(out.values()).backward()
    assert ls[2].grad is None or not ls[2].grad.any()                # the roots: a zero gradient


@pytest.mark.parametrize("case", ["n1", "n2"])
def test_fewer_than_three_frames_give_zeros_where_the_reference_raises(case, inputs, z):
    pred, gt = inputs[case]
    assert str(z[case + "/raises"]) == "IndexError"
    out = SL.compute_smoothnet_loss(pred, gt, None, None, 224)
    assert float(out["acc/h"]) == 0.0 == float(out["acc/o"]) and out["acc/h"].dtype == torch.float32
    assert abs(float(out["loss/cd"]) - float(z[case + "/loss/loss/cd"])) <= CD_ABS + TOL * float(z[case + "/loss/loss/cd"])


def test_objects_of_different_padded_length_raise_as_torch_does(inputs):
    pred, gt = inputs["all_valid"]
    short = _with(pred, object__v__cam=pred["object.v.cam"][:, :-1].contiguous())
    with pytest.raises((IndexError, RuntimeError)):
        SL.compute_smoothnet_loss(short, gt, None, None, 224)


# ---- acc_grad -------------------------------------------------------------------------------------------------------------------------
def test_acc_grad_keeps_the_values_and_the_default_detaches(inputs):
    pred, gt = inputs["coherent"]
    p, _ = MI.leaves(pred)
    off = SL.compute_smoothnet_loss(p, gt, None, None, 224)
    on = SL.compute_smoothnet_loss(p, gt, None, None, 224, acc_grad=True)
    for k in SL.KEYS:
        assert torch.equal(off[k], on[k]), k
    assert off["loss/cd"].requires_grad and not off["acc/h"].requires_grad and not off["acc/o"].requires_grad
    assert on["acc/h"].requires_grad and on["acc/o"].requires_grad


def test_acc_grad_matches_finite_differences_in_fp64(inputs):
    pred, gt = inputs["coherent"]
    w = {"loss/cd": 10.0, "acc/h": 1.0, "acc/o": 1.0}
    p, ls = MI.leaves(pred, dtype=torch.float64)

    def total(pp):
        out = SL.smooth_loss_reference(pp, gt, dtype=torch.float64, acc_grad=True)
        return sum(w[k] * out[k] for k in SL.KEYS)
    total(p).backward()
    g = torch.Generator().manual_seed(11)
    bottom = (gt["object.parts_ids"][0] == 2).nonzero().view(-1)
    probed, worst = 0.0, 0.0
    with torch.no_grad():
        for k, t in zip(MI.PRED_LEAVES, ls):
            rows = torch.randint(0, t.shape[1], (6,), generator=g).tolist()
            if k.startswith("mano.j3d"):
                rows = [0, 0, 0, 1]                                  # the root row, and one row without gradient
            if k == "object.v.cam":
                rows += [int(bottom[0]), int(gt["idx.ro"][2, 0])]    # a bottom column and a contact row
            for i, r in enumerate(rows):
                f, c = 1 + i % (t.shape[0] - 2), i % 3
                old = float(t[f, r, c])
                t[f, r, c] = old + 1e-6
                up = float(total(p))
                t[f, r, c] = old - 1e-6
                dn = float(total(p))
                t[f, r, c] = old
                fd = (up - dn) / 2e-6
                probed = max(probed, abs(float(t.grad[f, r, c])))
                worst = max(worst, abs(fd - float(t.grad[f, r, c])))
    assert probed > 0 and ls[2].grad[:, 1:].abs().max() == 0 and ls[2].grad[:, 0].abs().max() > 0
    assert worst <= 1e-6 * probed, (worst, probed)


def test_cpu_drop_in_is_the_restatement_bit_for_bit(inputs):
    for case in ("all_valid", "partial", "coherent"):
        pred, gt = inputs[case]
        for acc_grad in (False, True):
            p1, l1 = MI.leaves(pred)
            p2, l2 = MI.leaves(pred)
            a = SL.compute_smoothnet_loss(p1, gt, None, None, 224, acc_grad=acc_grad)
            b = SL.smooth_loss_reference(p2, gt, acc_grad=acc_grad)
            assert all(torch.equal(a[k], b[k]) for k in SL.KEYS)
            (10 * a["loss/cd"] + a["acc/h"] + a["acc/o"]).backward()
            (10 * b["loss/cd"] + b["acc/h"] + b["acc/o"]).backward()
            for x, y in zip(l1, l2):
                assert (x.grad is None) == (y.grad is None) and (x.grad is None or torch.equal(x.grad, y.grad))


# ---- the criterion and the exports ------------------------------------------------------------------------------------------------------
def test_smooth_criterion_is_the_references_module(inputs):
    pred, gt = inputs["coherent"]
    weights = {"loss/cd": 10.0, "acc/h": 1, "acc/o": 1}
    crit = SmoothCriterion(2, 4, weights, {"mano_r": None})
    assert (crit.batch_size, crit.window_size, crit.weight_dict, crit.acc_grad) == (2, 4, weights, False)
    assert crit.pre_process_models == {"mano_r": None} and not list(crit.parameters())
    data = AE.XDict()
    data.merge(pred.prefix("pred."))
    data.merge(gt.prefix("targets."))
    import types
    losses = crit(types.SimpleNamespace(img_res=224), data, None, None)
    want = SL.smooth_loss_reference(pred, gt)
    assert list(losses.keys()) == list(SL.KEYS) and all(torch.equal(losses[k], want[k]) for k in SL.KEYS)
    assert SmoothCriterion(2, 4, weights, {}, acc_grad=True).acc_grad is True


def test_package_exports():
    for name in ("compute_smoothnet_loss", "smooth_loss_reference", "eval_acc_pose", "compute_error_accel"):
        assert getattr(uvhand_amd, name) is getattr(SL, name) and name in uvhand_amd.__all__
    assert uvhand_amd.SmoothCriterion is SmoothCriterion and "SmoothCriterion" in uvhand_amd.__all__
