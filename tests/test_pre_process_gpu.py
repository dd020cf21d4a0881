"""arctic_pre_process on the MI355X (csrc/msda_pre_process.hip): the target fit, the distance fields, the composed step.

Tolerances.
  Target fit, against fit_targets_reference in fp64 on the same fp32 inputs: per output, relative to its largest value,
  max(4 x the deviation of the reference-run fp32 fixture from the same fp64 restatement, 16 x 2^-24), the rule and floor of
  tests/test_arctic_eval_gpu.py.  The deviations are measured at test time on the CPU (tests/test_pre_process.py prints them);
  when this was written they were, in units of 2^-24: transl 1.07, j3d_cam 2.56 / 3.06, cam_t 2.64 / 1.80, cam_t_wp 3.68 / 2.50
  / 1.73, so every bound is the floor.  R0, T0 and the two vertex offsets are in no fixture and get the floor: the kernel's
  algebra is fp64 and rounds once, half an ulp.  The bound is never measured against the kernel.
  Distance fields, against fp64 brute force on the same clouds (pre_process_inputs.assert_fields): the index equals the fp64
  argmin except where the two nearest squared distances lie within 2^-20 relative, at most 1e-3 of the searching rows
  (asserted from the fp64 data in tests/test_pre_process.py too); the distance is within 6 x 2^-24 relative of the fp64
  distance at the returned index; rows that do not search hold exactly 0 and 0.
  The step against the fixture: keys, order, dtypes and shapes exactly, float keys within 2e-4 relative."""
import sys
import warnings

import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import arctic_eval_inputs as EI  # noqa: E402
import pre_process_inputs as PI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd import pre_process as PP  # noqa: E402
from uvhand_amd.object_tensors import ObjectTensors  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOOR = 16 * 2.0 ** -24


def models(dev, lengths=None):
    return dict(EI.mano_models(dev), arti_head=ObjectTensors.from_arrays(SI.obj_arrays(lengths=lengths)).to(dev))


def to_dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.fixture(scope="module")
def z():
    return load_golden("pre_process")


@pytest.fixture(scope="module")
def bounds(z):
    dev = PI.fixture_deviation(z, models("cpu"), PP.fit_targets_reference)
    print("fixture deviations from fp64 (x 2^-24):", {k: round(v * 2 ** 24, 2) for k, v in dev.items()})
    return {k: max(4 * dev.get(k, 0.0), FLOOR) for k in PP.FIT_OUTPUTS}


def fit_batch(seed, B, NK, J):
    """Eight fp32 CPU tensors: frame 0 is exactly rigid (zero noise), frame 1 (if any) planar (z = x / 2, which fp32 holds
    exactly: a plane that rounding bends has an orientation again, and its sign is the rounding's), the rest noisy."""
    g = torch.Generator().manual_seed(seed)
    kp_cano = 0.1 * torch.randn(B, NK, 3, generator=g)
    if B > 1:
        kp_cano[1, :, 2] = 0.5 * kp_cano[1, :, 0]
    f = 900.0 + 200.0 * torch.rand(B, generator=g)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = f, f * (1.0 + 0.05 * torch.rand(B, generator=g))
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 110.0, 115.0, 1.0
    noise = torch.full((B, 1, 1), 1e-3, dtype=torch.float64)
    noise[0] = 0.0
    kp_full, kp2d, jr, jl, _ = PI.fit_inputs(kp_cano, K, g, noise=noise, J=J)
    return [kp_full, kp_cano, kp2d, K, jr, jl, 0.1 * torch.randn(B, J, 3, generator=g), 0.1 * torch.randn(B, J, 3, generator=g)]


def check_fit(ins, bounds, what):
    out, status = PP.fit_targets(*[t.to(DEV) for t in ins])
    ref, ref_status = PP.fit_targets_reference(*[t.double() for t in ins])
    assert status.dtype == torch.int32 and status.cpu().tolist() == ref_status.tolist(), what
    assert list(out) == list(PP.FIT_OUTPUTS)
    for k in PP.FIT_OUTPUTS:
        assert out[k].is_cuda and out[k].dtype == torch.float32 and out[k].shape == ref[k].shape, (what, k)
        err = rel_err(out[k].cpu().numpy(), ref[k].numpy())
        print("%s %-10s rel err %.3g (x 2^-24: %.2f)" % (what, k, err, err * 2 ** 24))
        assert err < bounds[k], (what, k, err)
    R = out["R0"].double().cpu()
    assert (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max() < FLOOR, what
    assert (torch.linalg.det(R) - 1).abs().max() < FLOOR, what
    return out, status


@pytest.mark.parametrize("NK", [3, 4, 16, 64])
def test_fit_against_fp64(NK, bounds):
    for B in (1, 3, 33):
        for J in (1, 21, 32):
            ins = fit_batch(100 * NK + 7 * B + J, B, NK, J)
            out, status = check_fit(ins, bounds, "NK %d B %d J %d" % (NK, B, J))
            # the status equals the restatement's (check_fit); the exactly rigid and the planar frame carry no bit, while
            # 1e-3 of noise can mirror a flat four-point set: the reference raises there
            assert not status[:2].any() and (NK == 4 or not status.any())
            again, _ = PP.fit_targets(*[t.to(DEV) for t in ins])
            assert all(torch.equal(out[k], again[k]) for k in out)


def test_fit_status_bits_and_isolation(bounds):
    targets, meta = PI.case_inputs("all_valid")
    ins = PI.fit_call_inputs(targets, meta, models("cpu"))
    base, s0 = PP.fit_targets(*[t.to(DEV) for t in ins])
    assert not s0.any()
    g = torch.Generator().manual_seed(5)
    kf, kc, k2, jr = ins[0].clone(), ins[1].clone(), ins[2].clone(), ins[4].clone()
    kf[1] = PI.mirrored(kf[1])
    cf, cc = PI.collinear(kc[3:4], g)
    kf[3], kc[3] = cf[0], cc[0]
    jr[4, 7, 1] = float("nan")
    k2[5] = 0.25
    bad = [kf, kc, k2, ins[3], jr] + ins[5:]
    out, status = PP.fit_targets(*[t.to(DEV) for t in bad])
    _, ref_status = PP.fit_targets_reference(*[t.double() for t in bad])
    assert status.cpu().tolist() == ref_status.tolist() == [0, 1, 0, 2, 4, 8]
    ref, _ = PP.fit_targets_reference(*[t.double() for t in bad])
    for k in PP.FIT_OUTPUTS:
        assert torch.isnan(out[k][4]).all(), k
        for b in (0, 2):                                          # no bit changes what other frames get
            assert torch.equal(out[k][b], base[k][b]), (k, b)
        assert rel_err(out[k][1].cpu().numpy(), ref[k][1].numpy()) < bounds[k], k        # the corrected rotation
    R = out["R0"][[0, 1, 2, 3, 5]].double().cpu()
    assert (torch.linalg.det(R) - 1).abs().max() < FLOOR and torch.isfinite(out["T0"][[3, 5]]).all()
    assert torch.isnan(out["transl"][5]).all() and torch.isnan(out["off_l"][5]).all()


@pytest.mark.parametrize("NV,L", PI.DF_SHAPES)
def test_distance_fields_against_fp64(NV, L):
    hr, hl, obj = [t.to(DEV) for t in PI.df_inputs(PI.DF_SEED, 3, NV, L)]
    for lens in PI.df_lengths(L):
        v_len = torch.tensor(lens, device=DEV)
        f = PP.distance_fields(hr, hl, obj, v_len)
        assert all(f[k].is_cuda and f[k].shape == (3, NV if k.endswith("o") else L) for k in PP.FIELD_KEYS)
        skipped, total = PI.assert_fields(f, hr, hl, obj, v_len)
        print("NV %d L %d v_len %s: near ties %d of %d" % (NV, L, lens, skipped, total))
        again = PP.distance_fields(hr, hl, obj, v_len)
        assert all(torch.equal(f[k], again[k]) for k in PP.FIELD_KEYS)
    # finite clamps: exactly the clamp of the unclamped field, rows that do not search included
    lo, hi = 0.02, 0.11
    c = PP.distance_fields(hr, hl, obj, v_len, lo, hi)
    for k in PP.FIELD_KEYS:
        assert torch.equal(c[k], f[k].clamp(lo, hi) if k.startswith("dist") else f[k]), k
    PI.assert_fields(c, hr, hl, obj, v_len, lo, hi)


def test_distance_fields_rules_as_on_the_cpu():
    """v_len of 0, 1 and L, duplicated and NaN targets, v_len out of range: the restatement's indices exactly."""
    g = torch.Generator().manual_seed(11)
    B, NV, L = 3, 7, 9
    obj = torch.randn(B, L, 3, generator=g)
    obj[:, 6] = obj[:, 2]
    hand_r = obj[:, [2, 0, 8, 5, 2, 1, 4]] + 1e-3 * torch.randn(B, NV, 3, generator=g)
    hand_l = hand_r.flip(1).contiguous()
    obj_nan = obj.clone()
    obj_nan[2, 2] = float("nan")
    for o, lens, lo, hi in ((obj, [0, 1, L], 0.0, float("inf")), (obj_nan, [0, 1, L], 0.0, float("inf")), (obj_nan, [L, L, L], 0.0, 0.5),
                            (obj, [-3, 1, L + 5], 2e-4, 0.3)):
        v_len = torch.tensor(lens)
        f = PP.distance_fields(hand_r.to(DEV), hand_l.to(DEV), o.to(DEV), v_len.to(DEV), lo, hi)
        r = PP.distance_fields_reference(hand_r, hand_l, o, v_len, lo, hi)
        for k in PP.FIELD_KEYS:
            if k.startswith("idx"):
                assert torch.equal(f[k].cpu(), r[k]), (k, lens)
            else:
                assert torch.equal(torch.isinf(f[k].cpu()), torch.isinf(r[k])), (k, lens)
                fin = torch.isfinite(r[k])
                assert torch.allclose(f[k].cpu()[fin], r[k][fin], rtol=1e-6, atol=0), (k, lens)
    assert f["idx.ro"][2].tolist() == [2, 0, 8, 5, 2, 1, 4] and not f["idx.ro"][0].any()


@pytest.mark.parametrize("case", list(PI.CASES))
def test_step_on_the_device_against_the_fixture(case, z):
    m = models(DEV)
    targets, meta = PI.case_inputs(case)
    targets, meta = PP.arctic_pre_process(EI.args(DEV), to_dev(targets), to_dev(meta), models=m)
    seen = PI.assert_matches_fixture(z, case, targets, meta, device_type="cuda")
    assert seen >= (30 if case == "all_valid" else 20), seen
    assert meta["fit_status"].is_cuda and not meta["fit_status"].any()
    PI.assert_fields(targets, targets["mano.v3d.cam.r"], targets["mano.v3d.cam.l"], targets["object.v.cam"], targets["object.v_len"])


def _big():
    m = models(DEV, EI.BIG_LENGTHS)
    targets, meta = PI.case_inputs(EI.BIG["case"], B=EI.BIG["B"], lengths=EI.BIG_LENGTHS, seed=EI.BIG["seed"])
    cpu = (dict(targets), dict(meta))
    targets, meta = to_dev(targets), to_dev(meta)
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    return targets, meta, idx, max_len, m, cpu


def test_realistic_size_syncs_and_launches(z, bounds):
    from torch.profiler import ProfilerActivity, profile

    targets, meta, idx, max_len, m, (cpu_t, cpu_m) = _big()
    step = lambda: PP.pre_process(dict(targets), meta, models=m, obj_idx=idx, max_len=max_len)  # noqa: E731
    out_t, out_m = step()                                  # warm-up: conversions, library load
    assert out_t["object.v.cam"].shape[1] > 3900 and len(set(out_t["object.v_len"].tolist())) > 3
    assert list(out_t.keys()) == list(z["partial/targets_keys"]) and list(out_m.keys())[-1] == "fit_status"
    assert not out_m["fit_status"].any()
    # the fit's outputs against the fp64 restatement on the same fp32 inputs (canonical keypoints and joints from the CPU chain)
    ins = PI.fit_call_inputs(cpu_t, cpu_m, models("cpu", EI.BIG_LENGTHS), lengths=EI.BIG_LENGTHS)
    ref, _ = PP.fit_targets_reference(*[t.double() for t in ins])
    for k, fk in PI.FIT_FIXTURE_KEYS.items():
        err = rel_err(out_t[fk].cpu().numpy(), ref[k].numpy())
        print("realistic %-10s rel err %.3g" % (k, err))
        assert err < 2e-4, (k, err)                        # the step's bound: kp_cano / joints come from the fp32 device chain
    skipped, total = PI.assert_fields(out_t, out_t["mano.v3d.cam.r"], out_t["mano.v3d.cam.l"], out_t["object.v.cam"], out_t["object.v_len"])
    print("realistic: near ties %d of %d" % (skipped, total))
    again, _ = step()
    assert all(torch.equal(again[k], out_t[k]) for k in out_t if torch.is_tensor(out_t[k]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
        PP.arctic_pre_process(EI.args(DEV), dict(targets), meta, models=m)        # names resolved with a pinned non-blocking copy
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert count("mano_fwd_kernel") == 1 and count("obj_fwd_kernel") == 1 and count("arctic_place_fwd_kernel") == 1, names
    assert count("pre_fit_kernel") == 1 and count("dist_fields_kernel") == 1, names


def test_step_captures_in_a_graph():
    m = models(DEV)
    targets, meta = PI.case_inputs("partial")
    targets, meta = to_dev(targets), to_dev(meta)
    idx, max_len = m["arti_head"].obj_index(meta["query_names"])
    run = lambda: PP.pre_process(dict(targets), meta, models=m, obj_idx=idx, max_len=max_len)  # noqa: E731
    eager_t, eager_m = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                              # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_t, g_m = run()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for k, v in eager_t.items():
            if torch.is_tensor(v):
                assert torch.equal(g_t[k], v), k
        assert torch.equal(g_m["fit_status"], eager_m["fit_status"]) and torch.equal(g_m["part_ids"], eager_m["part_ids"])


def test_check_raises_on_the_mirrored_frame_and_costs_one_sync():
    m = models(DEV)
    targets, meta = PI.case_inputs("all_valid")
    targets["object.kp3d.full.b"][2] = PI.mirrored(targets["object.kp3d.full.b"][2])
    targets, meta = to_dev(targets), to_dev(meta)
    t, mi = PP.arctic_pre_process(EI.args(DEV), dict(targets), meta, models=m)            # warm-up; without check: no raise
    assert mi["fit_status"].tolist() == [0, 0, 1, 0, 0, 0] and torch.isfinite(t["mano.v3d.cam.r"]).all()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            with pytest.raises(Exception, match="not orthogonal"):
                PP.arctic_pre_process(EI.args(DEV), dict(targets), meta, models=m, check=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len([w for w in caught if "synchroniz" in str(w.message)]) == 1


@pytest.mark.parametrize("trigger", ["env", "fp64", "cpu"])
def test_fallbacks_give_the_restatements(trigger, monkeypatch):
    targets, meta = PI.case_inputs("partial")
    ins = PI.fit_call_inputs(targets, meta, models("cpu"))
    hr, hl, obj = PI.df_inputs(PI.DF_SEED + 3, 2, 50, 70)
    v_len = torch.tensor([70, 33])
    if trigger != "cpu":
        ins, (hr, hl, obj, v_len) = [t.to(DEV) for t in ins], [t.to(DEV) for t in (hr, hl, obj, v_len)]
    if trigger == "env":
        monkeypatch.setenv("MSDA_PRE_PROCESS_FUSED", "0")
    elif trigger == "fp64":
        ins, (hr, hl, obj) = [t.double() for t in ins], [t.double() for t in (hr, hl, obj)]
    PP._WARNED.clear()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out, status = PP.fit_targets(*ins)
        f = PP.distance_fields(hr, hl, obj, v_len)
        PP.fit_targets(*ins)
        PP.distance_fields(hr, hl, obj, v_len)
    # a missed kernel is named once per cause; the A/B knob and CPU data are the user's own choice and stay silent
    told = [str(w.message) for w in caught if "torch restatement" in str(w.message)]
    assert len(told) == (2 if trigger == "fp64" else 0) and all("float64" in t for t in told), told
    ref, ref_status = PP.fit_targets_reference(*ins)
    assert torch.equal(status, ref_status) and all(torch.equal(out[k], ref[k]) and out[k].dtype == ins[0].dtype for k in out)
    rf = PP.distance_fields_reference(hr, hl, obj, v_len)
    assert all(torch.equal(f[k], rf[k]) for k in PP.FIELD_KEYS) and f["dist.ro"].dtype == hr.dtype


def test_empty_batch_on_the_device():
    z3 = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out, status = PP.fit_targets(z3(0, 4, 3), z3(0, 4, 3), z3(0, 4, 2), z3(0, 3, 3), *[z3(0, 2, 3)] * 4)
        f = PP.distance_fields(z3(0, 5, 3), z3(0, 5, 3), z3(0, 7, 3), torch.zeros(0, dtype=torch.long, device=DEV))
    assert not [w for w in caught if "torch restatement" in str(w.message)]
    assert status.shape == (0,) and status.is_cuda and out["R0"].shape == (0, 3, 3) and out["j3d_cam_l"].shape == (0, 2, 3)
    assert f["dist.ro"].shape == (0, 5) and f["idx.ol"].shape == (0, 7) and f["idx.ol"].dtype == torch.int64
