"""The arctic_pre_process drop-in on the CPU (uvhand_amd/pre_process.py): the torch restatements against
tests/golden/pre_process.npz, which gen_pre_process.py made by running the reference's own arctic_pre_process / process_data
and what they call; the distance fields' rules on inputs whose answer is known by construction; the fit's status bits.

Tolerances.  Float keys: 2e-4 relative to the key's largest value, the bound tests/test_arctic_eval_gpu.py uses for the same
MANO / object chain.  `dist.*` / `idx.*` are not fixtures (the generator cannot run knn_points): fp64 brute force is their
yardstick, the index equal except where the two nearest squared distances lie within 2^-20 relative."""
import math
import sys

import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import arctic_eval_inputs as EI  # noqa: E402
import pre_process_inputs as PI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd import arctic_eval as AE  # noqa: E402
from uvhand_amd import pre_process as PP  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors  # noqa: E402


@pytest.fixture(scope="module")
def models():
    return dict(EI.mano_models(), arti_head=ObjectTensors.from_arrays(SI.obj_arrays()))


@pytest.fixture(scope="module")
def z():
    return load_golden("pre_process")


def check_fields(targets):
    return PI.assert_fields(targets, targets["mano.v3d.cam.r"], targets["mano.v3d.cam.l"], targets["object.v.cam"],
                            targets["object.v_len"])


@pytest.mark.parametrize("case", list(PI.CASES))
def test_restatement_against_the_reference(case, models, z):
    targets, meta = PI.case_inputs(case)
    given = dict(targets)
    out_t, out_m = PP.arctic_pre_process(EI.args(), targets, meta, models=models)
    assert out_t is targets and isinstance(out_m, AE.XDict) and "fit_status" not in meta
    seen = PI.assert_matches_fixture(z, case, out_t, out_m)
    assert seen >= (30 if case == "all_valid" else 20), seen
    assert all(out_t[k] is v for k, v in given.items())                # the inputs stay what they were
    assert out_m["fit_status"].dtype == torch.int32 and not out_m["fit_status"].any()
    assert out_m["object.v_len"] is out_t["object.v_len"] and out_m["mano.faces.r"] is models["mano_r"].faces
    check_fields(out_t)
    # the drop-in is pre_process plus the signature
    t2, m2 = PP.pre_process(*PI.case_inputs(case), models=models)
    assert all(torch.equal(t2[k], out_t[k]) for k in out_t if torch.is_tensor(out_t[k]))


def test_fp64_restatement_gives_the_fixture_deviation(models, z):
    dev = PI.fixture_deviation(z, models, PP.fit_targets_reference)
    print("fixture deviations from fp64 (x 2^-24):", {k: round(v * 2 ** 24, 2) for k, v in dev.items()})
    assert all(0 < v < 2e-4 for v in dev.values()), dev
    # and the fp32 restatement against the fp64 one, per output (R0, T0 and the vertex offsets are in no fixture)
    targets, meta = PI.case_inputs("partial")
    ins = PI.fit_call_inputs(targets, meta, models)
    (o32, s32), (o64, s64) = PP.fit_targets_reference(*ins), PP.fit_targets_reference(*[t.double() for t in ins])
    assert list(o32) == list(PP.FIT_OUTPUTS) and torch.equal(s32, s64) and s32.dtype == torch.int32
    for k in PP.FIT_OUTPUTS:
        assert o32[k].dtype == torch.float32 and o64[k].dtype == torch.float64 and o32[k].shape == o64[k].shape
        assert rel_err(o32[k].numpy(), o64[k].numpy()) < 2e-5, k
    R = o64["R0"]
    assert (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-14
    assert (torch.linalg.det(R) - 1).abs().max() < 1e-14


def test_input_asserts():
    for case in PI.CASES:
        r1, r2 = PI.check_case(*PI.case_inputs(case))
        assert r2 > PI.MIN_RATIO and r1 >= r2
    PI.check_case(*PI.case_inputs(EI.BIG["case"], B=EI.BIG["B"], lengths=EI.BIG_LENGTHS, seed=EI.BIG["seed"]), lengths=EI.BIG_LENGTHS)


def test_distance_field_inputs_have_few_near_ties():
    """What tests/test_pre_process_gpu.py relies on, from the fp64 data alone: at its seeded clouds the share of searching
    points whose two nearest squared distances lie within 2^-20 relative (fp32 cannot order those) is within 0.1 %."""
    near = total = 0
    for NV, L in PI.DF_SHAPES:
        hr, hl, obj = PI.df_inputs(PI.DF_SEED, 3, NV, L)
        for v_len in PI.df_lengths(L):
            for first, dist, gap, searches in PI.df_yardstick(hr, hl, obj, torch.tensor(v_len)).values():
                near += int(((gap < PI.NEAR_TIE) & searches).sum())
                total += int(searches.sum())
    print("near ties: %d of %d" % (near, total))
    assert near <= PI.NEAR_TIE_SHARE * total, (near, total)
    assert PI.df_lengths(4097) == [[1, 1023, 1024], [1025, 2047, 2048], [2049, 3071, 3072], [3073, 4095, 4096], [4097, 4097, 4097]]
    assert PI.df_lengths(37) == [[1, 37, 37]] and PI.df_lengths(1) == [[1, 1, 1]]


def test_distance_fields_by_construction():
    """The length rule, padded sources, v_len of 0, 1 and L, the tie rule on duplicated targets, a NaN target and the clamp."""
    g = torch.Generator().manual_seed(11)
    B, NV, L = 3, 7, 9
    obj = torch.randn(B, L, 3, generator=g)
    obj[:, 6] = obj[:, 2]                                   # a duplicated target: the lowest index wins
    hand_r = obj[:, [2, 0, 8, 5, 2, 1, 4]] + 1e-3 * torch.randn(B, NV, 3, generator=g)
    hand_l = hand_r.flip(1).contiguous()
    v_len = torch.tensor([0, 1, L])
    f = PP.distance_fields(hand_r, hand_l, obj, v_len)
    assert list(f) == list(PP.FIELD_KEYS)
    for k in PP.FIELD_KEYS:
        assert f[k].dtype == (torch.float32 if k.startswith("dist") else torch.int64)
        assert f[k].shape == (B, NV if k.endswith("o") else L)
    # v_len = 0: nothing to find, nothing searches
    assert all(not f[k][0].any() for k in PP.FIELD_KEYS)
    # v_len = 1: row 0 is the only candidate and the only searching row
    assert not f["idx.ro"][1].any() and not f["idx.or"][1, 1:].any() and not f["dist.or"][1, 1:].any()
    assert torch.allclose(f["dist.ro"][1], (hand_r[1] - obj[1, :1]).norm(dim=1)) and f["dist.or"][1, 0] > 0
    # v_len = L: by construction, and 6 never wins against 2
    assert f["idx.ro"][2].tolist() == [2, 0, 8, 5, 2, 1, 4] and f["idx.lo"][2].tolist() == [4, 1, 2, 5, 8, 0, 2]
    assert f["idx.or"][2, 2] in (0, 4) and f["idx.or"][2, 6] == f["idx.or"][2, 2] and (f["dist.ro"][2] < 1e-2).all()
    # a NaN target never wins; a NaN source finds nothing: +inf (dist_max), index 0
    obj2 = obj.clone()
    obj2[2, 2] = float("nan")
    f2 = PP.distance_fields(hand_r, hand_l, obj2, v_len)
    assert f2["idx.ro"][2].tolist() == [6, 0, 8, 5, 6, 1, 4]
    assert f2["idx.or"][2, 2] == 0 and math.isinf(float(f2["dist.or"][2, 2]))
    assert float(PP.distance_fields(hand_r, hand_l, obj2, v_len, 0.0, 0.5)["dist.or"][2, 2]) == 0.5
    # the clamp, and v_len beyond its range
    f3 = PP.distance_fields(hand_r, hand_l, obj, torch.tensor([-3, 1, L + 5]), 2e-4, 0.3)
    assert f3["dist.ro"].min() == pytest.approx(2e-4) and f3["dist.or"].max() <= 0.3 + 1e-7
    assert (f3["dist.or"][0] == pytest.approx(2e-4)) and torch.equal(f3["idx.ro"][2], f["idx.ro"][2])
    with pytest.raises(ValueError):
        PP.distance_fields(hand_r, hand_l, obj, v_len, 1.0, 0.5)
    with pytest.raises(ValueError):
        PP.distance_fields(hand_r, hand_l[:, :3], obj, v_len)
    d64 = PP.distance_fields(hand_r.double(), hand_l.double(), obj.double(), v_len)
    assert d64["dist.ro"].dtype == torch.float64 and torch.equal(d64["idx.ro"], f["idx.ro"])


def test_status_bits(models):
    targets, meta = PI.case_inputs("all_valid")
    ins = PI.fit_call_inputs(targets, meta, models)
    base, s0 = PP.fit_targets_reference(*ins)
    assert not s0.any()
    g = torch.Generator().manual_seed(5)
    kf = ins[0].clone()
    kf[1] = PI.mirrored(kf[1])
    cf, cc = PI.collinear(ins[1][3:4], g)
    kc = ins[1].clone()
    kf[3], kc[3] = cf[0], cc[0]
    jr = ins[4].clone()
    jr[4, 7, 1] = float("nan")
    k2 = ins[2].clone()
    k2[5] = 0.25                                              # every keypoint in one pixel: a singular normal matrix
    for dtype in (torch.float32, torch.float64):
        out, status = PP.fit_targets_reference(*[t.to(dtype) for t in (kf, kc, k2, ins[3], jr, *ins[5:])])
        assert status.tolist() == [0, 1, 0, 2, 4, 8]
        for k in PP.FIT_OUTPUTS:
            assert torch.isnan(out[k][4]).all(), k
            for b in (0, 2):                                  # no bit changes what other frames get
                assert rel_err(out[k][b].numpy(), base[k][b].numpy()) < 1e-5, (k, b)
        R = out["R0"][[0, 1, 2, 3, 5]].double()
        assert (torch.linalg.det(R) - 1).abs().max() < 1e-5 and torch.isfinite(out["T0"][5]).all()
        assert torch.isnan(out["transl"][5]).all() and torch.isnan(out["off_r"][5]).all()
    with pytest.raises(ValueError):
        PP.fit_targets(*ins[:4], ins[4][:, :5], *ins[5:])


def test_check_raises_as_the_reference(models):
    targets, meta = PI.case_inputs("all_valid")
    targets["object.kp3d.full.b"][2] = PI.mirrored(targets["object.kp3d.full.b"][2])
    t, m = PP.arctic_pre_process(EI.args(), dict(targets), meta, models=models)
    assert m["fit_status"].tolist() == [0, 0, 1, 0, 0, 0] and torch.isfinite(t["mano.v3d.cam.r"]).all()
    with pytest.raises(Exception, match="not orthogonal"):
        PP.arctic_pre_process(EI.args(), dict(targets), meta, models=models, check=True)


def test_models_are_required(models):
    targets, meta = PI.case_inputs("all_valid")
    AE.set_default_models(None)
    with pytest.raises(RuntimeError, match="models"):
        PP.arctic_pre_process(EI.args(), dict(targets), meta)
    AE.set_default_models(models)
    try:
        assert "idx.ol" in PP.arctic_pre_process(EI.args(), dict(targets), meta)[0]
    finally:
        AE.set_default_models(None)
    import uvhand_amd
    assert uvhand_amd.arctic_pre_process is PP.arctic_pre_process and uvhand_amd.fit_targets is PP.fit_targets
    with pytest.raises(ValueError, match="max_len"):
        PP.pre_process(dict(targets), meta, models=models, obj_idx=torch.zeros(SI.FIXTURE_B, dtype=torch.long))


def test_empty_batch():
    out, status = PP.fit_targets(*[torch.zeros(0, 4, 3)] * 2, torch.zeros(0, 4, 2), torch.zeros(0, 3, 3), *[torch.zeros(0, 2, 3)] * 4)
    assert status.shape == (0,) and out["R0"].shape == (0, 3, 3) and out["j3d_cam_l"].shape == (0, 2, 3)
    f = PP.distance_fields(torch.zeros(0, 5, 3), torch.zeros(0, 5, 3), torch.zeros(0, 7, 3), torch.zeros(0, dtype=torch.long))
    assert f["dist.ro"].shape == (0, 5) and f["idx.ol"].shape == (0, 7) and f["idx.ol"].dtype == torch.int64
