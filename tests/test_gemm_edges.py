"""The edge cases of tests/golden/gemm_edge_inputs.py on the CPU, no GPU needed: each lies inside the support predicates,
its fp64 reference is consistent, and each would catch the kernel bugs it targets.  For every case, the result a kernel would
give if it dropped or double-counted the last chunk of a reduction, skipped the last K stage, lost the last row or column of
a tail tile, or misplaced a dgrad segment boundary by one is computed in fp64, and it must miss the reference by at least
MARGIN (10) times the tolerance tests/test_gemm_edges_gpu.py applies to it, in at least one region that test compares."""
import copy
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gemm_edge_inputs as EI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.heads_func import ARCTIC, detr_heads_reference  # noqa: E402
from uvhand_amd.functions.smoother_func import motion_smoothers_reference  # noqa: E402


def _margin(mutant, ref, regions_of, tol_of):
    """max over the mutated tensors and their regions of err / tol (how far the GPU test's check misses the mutant); None
    where the mutant equals the reference (zeroing a row that is 0 anyway, e.g. the weight row of a dead ReLU unit)."""
    if all(torch.equal(t, ref[s][k]) for s, ts in mutant.items() for k, t in ts.items()):
        return None
    best = 0.0
    for sname, tensors in mutant.items():
        for key, t in tensors.items():
            r = ref[sname][key]
            tol = tol_of(key)
            for mask in regions_of(key, tuple(r.shape)).values():
                best = max(best, EI.region_err(t, r, mask) / tol)
    return best


def _assert_margins(kind, name, margins):
    margins = {k: [x for x in v if x is not None] for k, v in margins.items()}
    assert all(margins.values()), [k for k, v in margins.items() if not v]
    for what, vals in sorted(margins.items()):
        print("MARGIN %s %s %-14s min %.3g over %d variants" % (kind, name, what, min(vals), len(vals)))
    low = {k: min(v) for k, v in margins.items() if min(v) < EI.MARGIN}
    assert not low, low


def _zero(t, index):
    t = t.clone()
    t[index] = 0
    return t


# ---- heads ----------------------------------------------------------------------------------------------------------------
def _heads_forward(kind, d_mods, hs, init, inter):
    cls, mlps, sh = d_mods
    with torch.no_grad():
        logits, keys, outs = detr_heads_reference(kind, hs.double(), init.double() if init is not None else None,
                                                  inter.double() if inter is not None else None, cls, mlps, sh)
    return logits


@pytest.fixture(scope="module", params=list(EI.HEADS_CASES))
def heads_case(request):
    name = request.param
    return name, EI.heads_reference(name)


def test_heads_case_supported(heads_case):
    name, ((kind, mods, hs, init, inter), _, weights, _, _, extra) = heads_case
    _, shared, L, B, Q, C, K, R, _ = EI.HEADS_CASES[name]
    assert _native.heads_supported(C)
    assert 1 <= L <= 8 and (R in ((42,) if kind == ARCTIC else (2, 42)) or (kind == ARCTIC and R == 0))
    cls, mlps, _ = mods
    assert all(m is cls[0] for m in cls) == shared or L == 1
    assert extra["kink"].float().mean().item() < 0.05           # the kink rows are few


def test_heads_reference_consistent(heads_case):
    """fp64 against an fp32 CPU evaluation of the same composition; the chunk sets partition the rows; the dgrad segments
    of grad_hs (class head, every MLP's first layer, the shared Linears) add up to it."""
    name, ((kind, mods, hs, init, inter), d_mods, weights, sets, ref, extra) = heads_case
    cls, mlps, sh = mods
    with torch.no_grad():
        logits32 = detr_heads_reference(kind, hs, init, inter, cls, mlps, sh)[0]
    assert EI.region_err(logits32, ref["full"]["out/logits"], torch.ones(logits32.shape, dtype=torch.bool)) < EI.ACT
    for fam in ("lvlchunk", "chunk"):
        names = [s for s in sets if s.startswith(fam)]
        if names:
            for key, full in ref["full"].items():
                if key.startswith("grad/"):
                    total = sum(ref[s][key] for s in names)
                    assert (total - full).abs().max() <= 1e-10 * full.abs().max(), (fam, key)
    seg = _heads_segments(name, d_mods, weights, extra)
    g = ref["full"]["grad/hs"]
    for lvl, segs in enumerate(seg):
        total = sum(dy @ w for dy, w in segs)
        assert (total - g[lvl]).abs().max() <= 1e-10 * g.abs().max()


def _heads_segments(name, d_mods, weights, extra):
    """Per level, the dgrad segments [(dy [B, Q, k], W [k, C])] in the kernel's order."""
    kind, _, L, B, Q, C, K, R, _ = EI.HEADS_CASES[name]
    cls, mlps, sh = d_mods
    n_mlp = len(mlps)
    out = []
    for lvl in range(L):
        segs = [(weights[0][lvl].double(), cls[lvl].weight.detach())]
        segs += [(extra["dz0"][lvl * n_mlp + h], mlps[h][lvl].layers[0].weight.detach()) for h in range(n_mlp)]
        if sh is not None:
            segs += [(weights[1 + n_mlp + g][lvl].double(), lin.weight.detach()) for g, lin in enumerate(sh)]
        out.append(segs)
    return out


def test_heads_mutations_caught(heads_case):
    name, ((kind, mods, hs, init, inter), d_mods, weights, sets, ref, extra) = heads_case
    _, shared, L, B, Q, C, K, R, _ = EI.HEADS_CASES[name]
    full = ref["full"]

    def margin(mutant):
        return _margin(mutant, ref, lambda k, s: EI.heads_regions(name, k, s), lambda k: EI.heads_tol(name, k))

    m = {}
    pkeys = [k for k in full if k.startswith("grad/") and k != "grad/hs"]
    # the last weight-gradient chunk of each problem dropped or counted twice
    for sign, what in ((-1, "chunk_drop"), (1, "chunk_double")):
        for key in pkeys:
            fam, rows = EI.heads_problem_rows(name, key[5:])
            n = (rows + EI.CHUNK - 1) // EI.CHUNK
            last = fam + str(n - 1)
            contrib = ref[last][key] if n > 1 else full[key]
            mutant = {"full": {key: full[key] + sign * contrib}}
            if n > 1:
                mutant[last] = {key: ref[last][key] * (1 + sign)}
            m.setdefault(what, []).append(margin(mutant))
    # the last K stage (partial where C % 32 != 0) of the class heads' forward skipped
    d2 = copy.deepcopy(d_mods)
    with torch.no_grad():
        for lin in {id(x): x for x in d2[0]}.values():
            lin.weight[:, EI.STAGE * ((C - 1) // EI.STAGE):] = 0
    m["kstage_fwd"] = [margin({"full": {"out/logits": _heads_forward(kind, d2, hs, init, inter)}})]
    # the last row / column of a tail tile lost (left 0)
    for key, t in full.items():
        if key.startswith("out/") or key == "grad/hs":
            tag = "out" if key.startswith("out/") else "dx"
            m.setdefault("tail_row_" + tag, []).append(margin({"full": {key: _zero(t, (L - 1, B - 1, Q - 1))}}))
            m.setdefault("tail_col_" + tag, []).append(margin({"full": {key: _zero(t, (Ellipsis, t.shape[-1] - 1))}}))
        else:
            m.setdefault("tail_row_dw", []).append(margin({"full": {key: _zero(t, t.shape[0] - 1)}}))
            if t.dim() == 2:
                m.setdefault("tail_col_dw", []).append(margin({"full": {key: _zero(t, (slice(None), t.shape[1] - 1))}}))
    # a dgrad segment boundary misplaced by one: the last column of the left or the first of the right segment lost
    g = full["grad/hs"]
    for lvl, segs in enumerate(_heads_segments(name, d_mods, weights, extra)):
        for (dy_l, w_l), (dy_r, w_r) in zip(segs[:-1], segs[1:]):
            for dy, w in ((dy_l[..., -1:], w_l[-1:]), (dy_r[..., :1], w_r[:1])):
                mut = g.clone()
                mut[lvl] -= dy @ w
                m.setdefault("segment", []).append(margin({"full": {"grad/hs": mut}}))
    _assert_margins("heads", name, m)


# ---- smoother -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(EI.SMOOTHER_CASES))
def smoother_case(request):
    name = request.param
    masks = EI.smoother_cpu_masks(name) if EI.SMOOTHER_CASES[name][6] is not None else None
    return name, masks, EI.smoother_reference(name, masks, extra_sets=True)


def _sm_forward(name, d_mods, xs, masks):
    p = EI.SMOOTHER_CASES[name][6]
    cm = EI.smoother_call_masks(name, masks) if masks is not None else None
    with torch.no_grad():
        return {"out/%d" % i: EI.smoother_composition(d_mods[mm], x.double(), cm[i] if cm else None, p or 0.0)
                for i, (mm, x) in enumerate(xs)}


def test_smoother_case_supported(smoother_case):
    name, _, ((mods, xs), _, weights, _) = smoother_case
    T, O, H, R, nb, calls, p, _ = EI.SMOOTHER_CASES[name]
    assert _native.smoother_supported(T, O, H, R, nb)
    _, rows = EI.smoother_module_rows(name)
    assert len(rows) <= _native.SMOOTHER_MAX_MODULES and len(calls) <= _native.SMOOTHER_MAX_CALLS
    assert all(sum(1 for m, _, _ in calls if m == u) <= _native.SMOOTHER_MAX_CALLS_PER_MODULE for u in rows)
    assert p is None or 0.0 <= p < 1.0
    kept = sum((w != 0).any(1).sum().item() for w in weights) / sum(B * C for _, B, C in calls)
    assert kept > 0.85                                             # the kink rows are few (2 of 19 in four_blocks)


def test_smoother_reference_consistent(smoother_case):
    """The composition (kink rows, train mode, the mutations' forwards) against motion_smoothers_reference in eval, fp64
    against fp32 on the CPU."""
    name, masks, ((mods, xs), d_mods, weights, ref) = smoother_case
    if masks is None:
        comp = _sm_forward(name, d_mods, xs, None)
        with torch.no_grad():
            ref32 = motion_smoothers_reference(xs, mods, False)
        for i, y in enumerate(ref32):
            r = ref["full"]["out/%d" % i]
            assert (comp["out/%d" % i] - r).abs().max() <= 1e-12 * r.abs().max()
            assert EI.region_err(y, r, torch.ones(r.shape, dtype=torch.bool)) < EI.smoother_tol(name, "out/0")


def test_smoother_mutations_caught(smoother_case):
    name, masks, ((mods, xs), d_mods, weights, ref) = smoother_case
    T, O, H, R, nb, calls, p, _ = EI.SMOOTHER_CASES[name]
    full = ref["full"]
    per_call, rows = EI.smoother_module_rows(name)

    def margin(mutant):
        return _margin(mutant, ref, lambda k, s: EI.smoother_regions(name, k, s), lambda k: EI.smoother_tol(name, k))

    m = {}
    for mod in rows:
        keys = [k for k in full if k.startswith("grad/m%d." % mod)]
        # the rows of a module's last call, or of its last 32-row stage of the weight-gradient reduction, dropped / doubled
        for sign, what in ((-1, "call_drop"), (1, "call_double")):
            m.setdefault(what, []).append(margin({"full": {k: full[k] + sign * ref["lastcall"][k] for k in keys}}))
        m.setdefault("wgrad_kstage", []).append(margin({"full": {k: full[k] - ref["laststage"][k] for k in keys}}))
    # the last K stage of the encoder (pos), the decoder (pos) and the fusion forward skipped; a boundary of the fusion's
    # [pos | vel | acc] reduction misplaced by one (the last column of the left or the first of the right part lost)
    variants = []
    for lin_of, k in ((lambda mm: mm.pos_smoother.encoder[0], T), (lambda mm: mm.pos_smoother.decoder, H),
                      (lambda mm: mm.fusion_layer, 3 * O)):
        variants.append(("kstage_fwd", lin_of, slice(EI.STAGE * ((k - 1) // EI.STAGE), k)))
    for s in (1, 2):
        variants += [("segment", lambda mm: mm.fusion_layer, slice(s * O - 1, s * O)),
                     ("segment", lambda mm: mm.fusion_layer, slice(s * O, s * O + 1))]
    for what, lin_of, cols in variants:
        d2 = copy.deepcopy(d_mods)
        with torch.no_grad():
            lin_of(d2[0]).weight[:, cols] = 0
        outs = _sm_forward(name, d2, xs, masks)
        m.setdefault(what, []).append(margin({"full": {k: v for k, v in outs.items() if xs[int(k[4:])][0] == 0}}))
    # the last row (module row rows - 1: the module's last call, b = B - 1, c = C - 1) / column of a tail tile lost
    for i, (mod, row0, r) in enumerate(per_call):
        out, gx = full["out/%d" % i], full["grad/x%d" % i]
        if row0 + r == rows[mod]:
            m.setdefault("tail_row_out", []).append(margin({"full": {"out/%d" % i: _zero(out, (-1, slice(None), -1))}}))
            m.setdefault("tail_row_dx", []).append(margin({"full": {"grad/x%d" % i: _zero(gx, (-1, slice(None), -1))}}))
        m.setdefault("tail_col_out", []).append(margin({"full": {"out/%d" % i: _zero(out, (slice(None), -1))}}))
        m.setdefault("tail_col_dx", []).append(margin({"full": {"grad/x%d" % i: _zero(gx, (slice(None), -1))}}))
    for key, t in full.items():
        if key.startswith("grad/m"):
            m.setdefault("tail_row_dw", []).append(margin({"full": {key: _zero(t, t.shape[0] - 1)}}))
            if t.dim() == 2:
                m.setdefault("tail_col_dw", []).append(margin({"full": {key: _zero(t, (slice(None), t.shape[1] - 1))}}))
    _assert_margins("smoother", name, m)
