"""The DINO criterion on the GPU (csrc/msda_criterion_dino.hip via uvhand_amd.criterion): the fused drop-in against the
reference-run fixture (tests/golden/gen_dino_criterion.py), the kernels against an fp64 evaluation of the torch restatement
over the shapes at which the code takes another path, bitwise reproducibility, a set's independence of the other sets of its
call, every gradient element written, no host sync, the launch count, graph capture, the status bits and the fallbacks.

The fp64 rule (ENVELOPE below), per loss column and per gradient tensor of a case: the kernel's largest absolute error
against the restatement in fp64 on the kernel's own match indices is at most 4 times the error of the fp32 restatement on the
GPU, that yardstick floored at one fp32 ulp of the tensor's largest fp64 magnitude; cardinality_error and the counts in
`stats` are integer-derived and exact.  Each case prints `MEASURED-DINO <case> <tensor> fp32 <err> kernel <err> ulp <ulp>`.

Measured on one MI355X, the worst ratio (kernel error over the floored yardstick, bar 4) over the seven cases: loss_ce 0.50
(matched_only_q1), loss_hand_keypoint 0.74 (mixed_3_2), loss_obj_keypoint 0.73 (mixed_3_2), logit gradients 1.24
(matched_only_q1, set 1), keypoint gradients 0.65 (q257_g33, the denoising set's object head).  The module's 30 tests take 22 s
there on their own, the build's import included.
"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import dino_criterion_inputs as DI   # noqa: E402
from test_dino_criterion import check_values, inputs, make_criterion, rel   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE_CASES = list(DI.CASES)


@pytest.fixture(scope="module")
def C():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import criterion
    return criterion


# ---- the fixture through the fused drop-in -----------------------------------------------------------------------------------
def _launches():
    from uvhand_amd import _native
    return _native.launch_count()


@pytest.mark.parametrize("case", FIXTURE_CASES)
def test_fused_drop_in_matches_reference_values(C, case):
    outputs, targets, store = inputs(case, DEV)
    crit = make_criterion(case)
    n0 = _launches()
    got = crit(outputs, targets, DI.ARGS, {})
    assert _launches() - n0 == 3                                      # the fused route: 1 match + 2 forward launches
    assert all(v.is_cuda for v in got.values())
    check_values(got, store)


def test_fused_small_gradients_match_reference(C):
    outputs, targets, store = inputs("small", DEV, requires_grad=True)
    crit = make_criterion("small")
    n0 = _launches()
    DI.weighted_total(crit(outputs, targets, DI.ARGS, {}), crit.weight_dict).backward()
    assert _launches() - n0 == 4                                      # ... + 1 backward launch
    for name, g in DI.gradients(outputs).items():
        assert rel(g.cpu().numpy(), store[name]) <= 1e-5, name


def test_no_object_nan_placement(C):
    outputs, targets, store = inputs("no_object", DEV)
    got = make_criterion("no_object")(outputs, targets, DI.ARGS, {})
    want = [str(k) for k, v in zip(store["keys"], store["values"]) if np.isnan(v)]
    assert want and [k for k, v in got.items() if bool(torch.isnan(v))] == want


# ---- the kernels against fp64 over their envelope ----------------------------------------------------------------------------
# name: bs, K, D, matched Q, matched sets, (groups, single_pad), dn sets, every third frame invalid
ENVELOPE = {
    "mixed_3_2": (3, 14, 42, 40, 3, (2, 6), 2, False),               # the mixed call; n_f 3, 1, 0 in one call
    "dn_only_g1": (1, 2, 0, 0, 0, (1, 2), 1, False),                  # one row pair: groups 1, single_pad 2, labels only
    "dn_only_wide": (3, 14, 42, 0, 0, (3, 32), 2, False),             # denoising sets alone, n_f up to 16
    "matched_only_q1": (65, 14, 42, 1, 2, None, 0, False),            # matched sets alone, one query, bs past a wave
    "q257_g33": (3, 14, 42, 257, 2, (33, 6), 1, False),               # one row past a 256-row chunk; 198 denoising rows
    "k2_interleaved": (65, 2, 42, 40, 1, (3, 32), 1, True),           # K = 2, invalid frames, 65 chunks per set
    "many_chunks": (65, 14, 0, 257, 1, (2, 6), 1, True),              # 130 chunks in the matched set, labels only
}
TERMS = ("loss_ce", "loss_hand_keypoint", "loss_obj_keypoint", "cardinality_error")


def envelope_case(name, device, dtype, requires_grad=False):
    """(matched sets, dn sets, targets, groups, single_pad) with seeded values; every set has a paired object row."""
    bs, K, D, Q, n_m, dn, n_dn, interleaved = ENVELOPE[name]
    groups, single_pad = dn if dn else (0, 0)
    g = torch.Generator().manual_seed(sorted(ENVELOPE).index(name) + 7)

    def one(q):
        o = {"pred_logits": torch.randn(bs, q, K, generator=g) * 2.0}
        if D:
            o["pred_hand_key"] = torch.rand(bs, q, D, generator=g)
            o["pred_obj_key"] = torch.rand(bs, q, D, generator=g)
        return {k: v.to(device=device, dtype=dtype).requires_grad_(requires_grad) for k, v in o.items()}

    matched = [one(Q) for _ in range(n_m)]
    dns = [one(groups * single_pad) for _ in range(n_dn)]
    half = single_pad // 2 if dn else 3
    labels, keypoints = [], []
    for f in range(bs):
        T = (half, 1, 0, 1 + (f % half))[f % 4] if bs > 1 else half
        objects_only = K < 14 or Q == 1
        lab = [int(torch.randint(0 if K < 14 else 1, min(K, 12), (1,), generator=g))]      # the frame's first: an object
        for _ in range(T - 1):
            r = int(torch.randint(0, 10, (1,), generator=g))
            lab.append(12 + (r & 1) if r < 5 and not objects_only else int(torch.randint(0, min(K, 12), (1,), generator=g)))
        labels.append(lab[:T])
        keypoints.append(torch.rand(T, D, generator=g).to(device=device, dtype=dtype))
    is_valid = torch.ones(bs, dtype=torch.float32)
    if interleaved:
        is_valid[2::3] = 0
    targets = {"labels": labels, "is_valid": is_valid.to(device)}
    if D:
        targets["keypoints"] = keypoints
    return matched, dns, targets, groups, single_pad


def _weights(sets, device, dtype):
    return (1.0 + 0.25 * torch.arange(sets * 4, dtype=dtype, device=device)).view(sets, 4)


def _heads(D):
    return DI.HEADS if D else DI.HEADS[:1]


def run_fused_envelope(C, name, only=None):
    """match + dino_set_losses + backward of an envelope case (only: indices into matched + dn sets to keep)."""
    from uvhand_amd import matcher as M
    D = ENVELOPE[name][2]
    matched, dns, targets, groups, single_pad = envelope_case(name, DEV, torch.float32, requires_grad=True)
    if only is not None:
        every = matched + dns
        matched = [every[i] for i in only if i < len(matched)]
        dns = [every[i] for i in only if i >= len(every) - len(dns)]
    packed = M.pack_targets(targets, DEV)
    nb = float(max(sum(packed.sizes), 1))
    res = None
    if matched:
        with torch.no_grad():
            res = M.match(matched, packed, DI.COST_CLASS, DI.COST_BBOX)
    out = C.dino_set_losses(matched, packed, res, nb, dns, single_pad, groups, DI.FOCAL_ALPHA)
    sets = matched + dns
    (out.losses.nan_to_num() * _weights(len(sets), DEV, torch.float32)).sum().backward()
    torch.cuda.synchronize()
    got = {"losses": out.losses.detach().cpu(), "stats": out.stats.cpu(), "nb": nb}
    if res is not None:
        got.update(qi=res.query_idx.cpu(), ti=res.target_idx.cpu(), count=res.count.cpu(), num_valid=int(res.num_valid))
    for h in _heads(D):
        got["grad_" + h] = [o[h].grad.cpu() for o in sets]
    return got


_RUNS = {}


def fused_envelope(C, name):
    if name not in _RUNS:
        _RUNS[name] = run_fused_envelope(C, name)
    return _RUNS[name]


def dn_pairs(targets, groups, single_pad):
    """dino.py:620-634: per valid frame (output rows, target indices)."""
    pairs = []
    for f, lab in enumerate(targets["labels"]):
        if targets["is_valid"][f] != 1:
            continue
        t = torch.arange(len(lab), dtype=torch.int64).unsqueeze(0).repeat(groups, 1)
        pairs.append((((torch.arange(groups, dtype=torch.int64) * single_pad).unsqueeze(1) + t).flatten(), t.flatten()))
    return pairs


def restatement(C, name, got, device, dtype):
    """(terms [sets, 4], {head: per-set gradient list}) of the package's torch restatement in `dtype` on `device`, the
    matched sets on the kernel's own indices."""
    bs, K, D, Q, n_m, dn, n_dn, _ = ENVELOPE[name]
    matched, dns, targets, groups, single_pad = envelope_case(name, device, dtype, requires_grad=True)
    losses = ["labels", "cardinality"] + (["boxes"] if D else [])
    rows = []
    for s, o in enumerate(matched + dns):
        if s < n_m:
            idx = [(got["qi"][s, k, :got["count"][s, k]], got["ti"][s, k, :got["count"][s, k]])
                   for k in range(got["num_valid"])]
            nb = got["nb"]
        else:
            idx, nb = dn_pairs(targets, groups, single_pad), got["nb"] * groups
        d = C.arctic_set_losses(o, targets, idx, nb, losses, K, DI.FOCAL_ALPHA, empty=K - 1)
        rows.append(torch.stack([d[n].to(dtype) if n in d else torch.zeros((), dtype=dtype, device=device) for n in TERMS]))
    full = torch.stack(rows)
    (full.nan_to_num() * _weights(len(rows), device, dtype)).sum().backward()
    grads = {h: [(o[h].grad if o[h].grad is not None else torch.zeros_like(o[h])).cpu() for o in matched + dns]
             for h in _heads(D)}
    return full.detach().cpu(), grads


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


def _worst(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


@pytest.mark.parametrize("name", list(ENVELOPE))
def test_kernels_within_four_times_the_fp32_restatement(C, name):
    bs, K, D, Q, n_m, dn, n_dn, interleaved = ENVELOPE[name]
    got = fused_envelope(C, name)
    ref_terms, ref_grads = restatement(C, name, got, "cpu", torch.float64)
    f32_terms, f32_grads = restatement(C, name, got, DEV, torch.float32)
    assert not torch.isnan(ref_terms).any(), (name, "a 0 / 0 row in the record the ratios are measured on")
    assert (got["stats"][:, 0] == 0).all() and (got["stats"][:, 3] == 0).all()

    checks = {}
    for c, term in enumerate(TERMS[:3]):
        checks[term] = (f32_terms[:, c], got["losses"][:, c], ref_terms[:, c])
    for h in _heads(D):
        for s in range(n_m + n_dn):
            checks["grad_%s[%d]" % (h, s)] = (f32_grads[h][s], got["grad_" + h][s], ref_grads[h][s])
    failures = []
    for what, (f32, kernel, ref) in checks.items():
        ulp = _ulp32(float(ref.abs().max()))
        e32, e = _worst(f32, ref), _worst(kernel, ref)
        print("MEASURED-DINO %s %-22s fp32 %.3g kernel %.3g ulp %.3g ratio %.2f" % (name, what, e32, e, ulp,
                                                                                  e / max(e32, ulp)))
        if e > 4 * max(e32, ulp):
            failures.append((what, e, e32, ulp))
    assert not failures, (name, failures)

    # integer-derived: cardinality and the counts in stats, exact
    assert torch.equal(got["losses"][:, 3].double(), ref_terms[:, 3]), name
    _, _, targets, groups, single_pad = envelope_case(name, "cpu", torch.float32)
    valid = [f for f in range(bs) if targets["is_valid"][f] == 1]
    for s in range(n_m + n_dn):
        if s < n_m:
            labs = [targets["labels"][valid[k]][t] for k in range(got["num_valid"])
                    for t in got["ti"][s, k, :got["count"][s, k]].tolist()]
        else:
            labs = [x for f in valid for x in targets["labels"][f]] * groups
        n_hand = sum(x in (12, 13) for x in labs)
        assert got["stats"][s].tolist() == [0, n_hand, len(labs) - n_hand, 0], (name, s)


def test_envelope_covers_the_stated_shapes():
    cases = list(ENVELOPE.values())
    assert {c[0] for c in cases} == {1, 3, 65} and {c[1] for c in cases} == {2, 14} and {c[2] for c in cases} == {0, 42}
    assert {c[3] for c in cases if c[4]} == {1, 40, 257}
    assert {c[5] for c in cases if c[6]} == {(1, 2), (2, 6), (33, 6), (3, 32)}
    assert any(c[4] == 0 for c in cases) and any(c[6] == 0 for c in cases) and any(c[4] == 3 and c[6] == 2 for c in cases)
    from uvhand_amd import _native
    chunks = [_native.criterion_dino_workspace_bytes(c[0], [c[3]] if c[4] else [c[5][0] * c[5][1]]) // 64 for c in cases]
    assert min(chunks) == 1 and max(chunks) >= 100
    _, _, targets, _, single_pad = envelope_case("mixed_3_2", "cpu", torch.float32)
    assert sorted(len(t) for t in targets["labels"]) == [0, 1, single_pad // 2]


# ---- reproducibility, independence, written gradients -------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    for key in a:
        va, vb = a[key], b[key]
        if isinstance(va, list):
            if not all(torch.equal(_bits(x), _bits(y)) for x, y in zip(va, vb)):
                return False
        elif torch.is_tensor(va):
            if not torch.equal(_bits(va) if va.is_floating_point() else va, _bits(vb) if vb.is_floating_point() else vb):
                return False
    return True


@pytest.mark.parametrize("deterministic", [False, True])
def test_bitwise_reproducible(C, deterministic):
    torch.use_deterministic_algorithms(deterministic)
    try:
        for name in ("mixed_3_2", "many_chunks"):
            assert _same(run_fused_envelope(C, name), run_fused_envelope(C, name)), name
    finally:
        torch.use_deterministic_algorithms(False)


def test_a_set_alone_gives_the_bits_of_its_row(C):
    mixed = fused_envelope(C, "mixed_3_2")
    for s in (1, 4):                                                   # a matched set, a denoising set
        alone = run_fused_envelope(C, "mixed_3_2", only=[s])
        assert torch.equal(_bits(alone["losses"][0]), _bits(mixed["losses"][s])), s
        assert torch.equal(alone["stats"][0], mixed["stats"][s]), s


def test_dn_gradients_zero_off_the_pairs_and_every_element_written(C):
    from uvhand_amd import _native
    from uvhand_amd import matcher as M
    name = "dn_only_wide"
    bs, K, D, _, _, (groups, single_pad), n_dn, _ = ENVELOPE[name]
    _, dns, targets, _, _ = envelope_case(name, DEV, torch.float32)
    packed = M.pack_targets(targets, DEV)
    nb = torch.full((1,), 5.0, device=DEV)
    logits, hand, obj = ([o[h] for o in dns] for h in DI.HEADS)
    args = ([-1] * n_dn, None, 0, packed.t_max, packed.labels, packed.keypoints, packed.offsets, packed.is_valid,
            (1 << 12) | (1 << 13), nb, DI.FOCAL_ALPHA, single_pad, groups)
    losses, stats = _native.criterion_dino_fwd(logits, hand, obj, *args)
    sentinel = float(np.float32(-12345.5))
    out = tuple([torch.full_like(t, sentinel) for t in ts] for ts in (logits, hand, obj))
    _native.criterion_dino_bwd(logits, hand, obj, *args, _weights(n_dn, DEV, torch.float32), stats, out=out)
    torch.cuda.synchronize()
    pair = torch.zeros(bs, groups * single_pad, dtype=torch.bool)
    for f, lab in enumerate(targets["labels"]):                        # every frame valid: slot f is frame f
        for g in range(groups):
            pair[f, g * single_pad:g * single_pad + len(lab)] = True
    assert pair.any() and not pair.all()
    for ts in out:
        for t in ts:
            assert not (t == sentinel).any()
    for t in out[1] + out[2]:
        assert (t.cpu()[~pair] == 0).all()
    hand_rows = torch.stack([g.cpu()[pair].abs().sum(-1) > 0 for g in out[1]])
    obj_rows = torch.stack([g.cpu()[pair].abs().sum(-1) > 0 for g in out[2]])
    assert (hand_rows ^ obj_rows).all()                                # a pair's row goes to exactly one head


# ---- no host sync, launch count, graph capture ------------------------------------------------------------------------------------
def _small_step_inputs():
    from uvhand_amd import matcher as M
    outputs, targets, _ = inputs("small", DEV, requires_grad=True)
    sets, dn = DI.sets_of(outputs), DI.dn_set(outputs)
    groups, single_pad = DI.shape("small")[2:4]
    return sets, dn, M.pack_targets(targets, DEV), groups, single_pad


def test_match_losses_backward_no_sync_four_launches(C):
    from uvhand_amd import matcher as M
    sets, dn, packed, groups, single_pad = _small_step_inputs()
    w = _weights(len(sets) + 1, DEV, torch.float32)
    nb = torch.full((1,), 7.0, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n0 = _launches()
        res = M.match(sets, packed, DI.COST_CLASS, DI.COST_BBOX)
        n1 = _launches()
        out = C.dino_set_losses(sets, packed, res, nb, [dn], single_pad, groups, DI.FOCAL_ALPHA)
        n2 = _launches()
        (out.losses * w).sum().backward()
        n3 = _launches()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert (n1 - n0, n2 - n1, n3 - n2) == (1, 2, 1)                    # 1 match + 2 forward + 1 backward
    assert out.losses.shape == (len(sets) + 1, 4) and int(out.status.abs().sum()) == 0


def test_drop_in_forward_with_small_loss_many_makes_no_sync(C):
    class Many:
        def many(self, sets, targets, meta_info, args, suffixes):
            return [{"loss_mano" + s: sets[i]["pred_hand_key"].mean()} for i, s in enumerate(suffixes)]

    outputs, targets, _ = inputs("small", DEV)
    crit = make_criterion("small", small_loss=Many())
    crit(outputs, targets, DI.ARGS, {})
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            got = crit(outputs, targets, DI.ARGS, {})
        finally:
            torch.cuda.set_sync_debug_mode(0)
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert not syncs, [str(w.message) for w in syncs]
    assert "loss_mano" in got and "loss_mano_1" in got and "class_error" in got


def test_graph_capture_replays_on_fresh_predictions(C):
    from uvhand_amd import matcher as M
    sets, dn, packed, groups, single_pad = _small_step_inputs()
    leaves = [o[h] for o in sets + [dn] for h in DI.HEADS]
    nb = torch.full((1,), 9.0, device=DEV)
    w = _weights(len(sets) + 1, DEV, torch.float32)

    def step():
        with torch.no_grad():
            res = M.match(sets, packed, DI.COST_CLASS, DI.COST_BBOX)
        out = C.dino_set_losses(sets, packed, res, nb, [dn], single_pad, groups, DI.FOCAL_ALPHA)
        return res.buffer, out.losses, torch.autograd.grad((out.losses.nan_to_num() * w).sum(), leaves)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = step()
    before = cap[1].clone()
    g = torch.Generator(device=DEV).manual_seed(5)
    with torch.no_grad():
        for o in sets + [dn]:
            o["pred_logits"].copy_(torch.randn(o["pred_logits"].shape, generator=g, device=DEV) * 2)
            o["pred_hand_key"].mul_(0.5).add_(0.25)
    graph.replay()
    eager = step()
    torch.cuda.synchronize()
    assert not torch.equal(before, cap[1])
    assert torch.equal(cap[0], eager[0]) and torch.equal(_bits(cap[1]), _bits(eager[1]))
    assert all(torch.equal(a, b) for a, b in zip(cap[2], eager[2]))


# ---- status and fallbacks ----------------------------------------------------------------------------------------------------
def test_bad_label_sets_the_bit_and_check_mode_raises(C, monkeypatch):
    from uvhand_amd import _native
    outputs, targets, _ = inputs("small", DEV)
    targets["labels"][1][0] = DI.K                                    # outside [0, K)
    crit = make_criterion("small")
    crit(outputs, targets, DI.ARGS, {})                               # no trap, no raise
    sets, dn = DI.sets_of(outputs), DI.dn_set(outputs)
    from uvhand_amd import matcher as M
    packed = M.pack_targets(targets, DEV)
    groups, single_pad = DI.shape("small")[2:4]
    out = C.dino_set_losses([], packed, None, 3.0, [dn], single_pad, groups)
    assert int(out.status[0]) & _native.CRIT_BAD_LABEL
    monkeypatch.setenv("MSDA_CRITERION_CHECK", "1")
    with pytest.raises(IndexError):
        crit(outputs, targets, DI.ARGS, {})


def test_too_many_targets_for_single_pad_takes_the_restatement(C, monkeypatch):
    outputs, targets, _ = inputs("small", DEV)
    g = torch.Generator().manual_seed(3)
    targets["labels"][2] = [1, 2, 3, 4]                               # n_f = 4 > single_pad // 2 = 3
    targets["keypoints"][2] = torch.rand(4, DI.D, generator=g).to(DEV)
    crit = make_criterion("small")
    n0 = _launches()
    got = crit(outputs, targets, DI.ARGS, {})
    assert _launches() - n0 == len(DI.sets_of(outputs))               # one matcher launch per set, no criterion launch
    monkeypatch.setenv("MSDA_CRITERION_FUSED", "0")
    want = crit(outputs, targets, DI.ARGS, {})
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) or (torch.isnan(got[k]) and torch.isnan(want[k]))
                                           for k in got)


def test_fused_knob_off_gives_the_same_dict(C, monkeypatch):
    outputs, targets, store = inputs("interleaved", DEV)
    monkeypatch.setenv("MSDA_CRITERION_FUSED", "0")
    n0 = _launches()
    got = make_criterion("interleaved")(outputs, targets, DI.ARGS, {})
    assert _launches() - n0 == len(DI.sets_of(outputs))
    check_values(got, store)


def test_enc_outputs_raise_before_any_launch(C):
    outputs, targets, _ = inputs("small", DEV)
    outputs["enc_outputs"] = [{"pred_logits": outputs["pred_logits"]}]
    n0 = _launches()
    with pytest.raises(AssertionError):
        make_criterion("small")(outputs, targets, DI.ARGS, {})
    assert _launches() == n0


def test_return_indices_copies_the_match_buffer(C):
    outputs, targets, _ = inputs("small", DEV)
    crit = make_criterion("small")
    _, indices = crit(outputs, targets, DI.ARGS, {}, return_indices=True)
    sets = DI.sets_of(outputs)
    assert len(indices) == len(sets)
    for got, o in zip(indices, sets[1:] + sets[:1]):                   # the reference's order: aux..., interm, final
        want = crit.matcher(o, targets)
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, want))
