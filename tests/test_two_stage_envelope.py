"""The two-stage proposal, selection and embedding kernels over their envelope, on the CPU: the conditions of the seeded
builder (tests/golden/two_stage_envelope_inputs.py) that keep tests/test_two_stage_envelope_gpu.py from passing vacuously.

Proposals: torch's fp32 composition and the fp64 restatement agree on every validity bit — for every case, and for every valid
extent from 1 to 599 — every learned column stays 1e-4 relative away from 0.01 and 0.99 at every level, and each case counts
the rows or levels of the edge it exists for: rows that die of the (0.01, 0.99) rule on the pixel centre alone, levels that
die of their constant columns, a second trip of the extent loops.  Selection: the oracle equals the reference's composition
where that is defined (no ties, no NaN), the selected rows read every source the class rule can reach, and every logit class
holds what it is named for.  The Python-side refusal (``topk > S``) and fallback (``S = 8193``).  Fused node: the case table
has the issue's tile counts, every compared tensor a positive scale, and the bound comes out of the fp32 composition."""
import math
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import two_stage_envelope_inputs as EI  # noqa: E402
from uvhand_amd.functions import assembly_func as AF  # noqa: E402
from uvhand_amd.functions import two_stage_func as TS  # noqa: E402


# ---- proposals ----------------------------------------------------------------------------------------------------------------
def test_case_tables_are_the_issues():
    assert [c[0] for c in EI.PROPOSAL_CASES.values()] == [
        [(300, 1), (1, 300), (51, 5), (2, 100), (7, 7)], [(50, 50)], [(49, 49)], [(1, 1)], [(3, 2)] * 16, [(257, 2), (2, 257)],
        [(4, 60)]]
    assert EI.PROPOSAL_CASES["4x60pad10"][1] == 10 and EI.ASSEMBLY_CASES["4x60pad10"][1] == 10
    assert [c[0] for c in EI.ASSEMBLY_CASES.values()] == [(300, 1), (1, 300), (50, 50), (49, 49), (4, 60)]
    assert EI.CHANNELS == (4, 8, 260) and EI.LEARNED == ("none", "in_range", "high_from_3", "low_at_0", "nan")
    assert EI.SELECT_SHAPES == [(1, 1, 1, 1), (2, 2, 2, 14), (3, 3, 1, 14), (2, 1024, 300, 14), (2, 1025, 1025, 3),
                                (2, 1023, 1023, 14), (1, 4097, 1, 16), (1, 8192, 8192, 2), (5, 257, 0, 14)]
    assert len(EI.LOGITS) == 8 and len(EI.SELECT_CASES) == 8 * 10
    assert {hc for _, _, hc in EI.SELECT_CASES} == {(12, 13), (1, 2), (14, 15)}
    assert EI.PE_ROWS == (1, 3, 257) and len(EI.SPECIALS) == 11
    assert EI.NODE_CASES == [(1, 4), (63, 128), (64, 124), (65, 132), (129, 260), (130, 640), (513, 128), (100, 1020)]
    assert [EI.node_tiles(*c) for c in EI.NODE_CASES] == EI.NODE_TILES == [1, 1, 1, 4, 9, 15, 9, 16]
    assert EI.FLOOR == 16 * 2.0 ** -24 and EI.PROPOSAL_BOUND == 2e-6 and EI.PE_BOUND == 2e-6


def _composition_bits(mask, levels, xy):
    S = mask.shape[1]
    _, props = TS.proposals_composition(torch.zeros(mask.shape[0], S, 4), mask, levels, xy)
    dead = torch.isinf(props).all(-1)
    assert torch.equal(torch.isinf(props).any(-1), dead) and not bool(torch.isnan(props).any())
    return props, dead


@pytest.mark.parametrize("learned", EI.LEARNED)
@pytest.mark.parametrize("name", EI.PROPOSAL_CASES)
def test_proposal_case_bits_and_counters(name, learned):
    levels, pad_cols, edges = EI.PROPOSAL_CASES[name]
    L = len(levels)
    xy = EI.learned_offsets(learned)
    if xy is not None:
        margin = EI.learned_margin(xy, L)
        print("MEASURED-CPU %s %s learned margin %.2e" % (name, learned, margin))
        assert margin >= EI.MARGIN and int(torch.isnan(xy).sum()) == (learned == "nan")
    for pattern in EI.PATTERNS:
        mask = EI.proposal_mask(levels, pattern, pad_cols)
        assert mask.shape == (4, sum(h * w for h, w in levels))
        parts = EI.proposal_parts(mask, levels, xy)
        props32, dead32 = _composition_bits(mask, levels, xy)
        assert torch.equal(dead32, parts["dead"])            # fp32 and fp64 agree on every validity bit
        fin = ~parts["dead"]
        dev = (props32.double() - parts["props"])[fin].abs().max().item() if bool(fin.any()) else 0.0
        cnt = EI.proposal_counters(parts, levels)
        print("MEASURED-CPU %s %s %s: composition - fp64 %.2e, rule-alone rows %s, dead levels %d, second-trip entries %d"
              % (name, learned, pattern, dev, cnt["rule"].tolist(), cnt["xy"], cnt["trip2"]))
        assert dev <= EI.PROPOSAL_BOUND
        assert bool(parts["dead"][2].all()) and bool(parts["dead"][3].all())     # fully padded; valid_W = 0
        assert bool((parts["vw"][3] == 0).all()) and bool((parts["vw"][2] == 0).all())
        ok = parts["level_ok"].tolist()
        if learned == "none":
            assert ok == [l < 5 for l in range(L)]           # 0.05 * 2^5 = 1.6
        elif learned == "in_range":
            assert ok == [l < 7 for l in range(L)]
        elif learned == "high_from_3":
            assert ok == [l < 3 for l in range(L)]
        elif learned == "low_at_0":
            assert ok == [1 <= l < 7 for l in range(L)]
        else:
            assert not any(ok)
        if pattern != "plain" or learned != "none":
            continue
        # the edge each case exists for, on the clean frame (and the rectangle) of the plain pattern
        if "rule" in edges:
            assert int(cnt["rule"][0]) > 0
        if "no_rule" in edges:
            assert int(cnt["rule"][0]) == 0 and int(cnt["rule"][1]) == 0 and bool(fin[0, parts["level_ok"][parts["level"]]].all())
        assert (cnt["trip2"] > 0) == ("trip2" in edges)
        assert (cnt["xy"] > 0) == ("xy" in edges)
    if name == "50x50" and learned == "none":                # 0.5 / 50 is 0.01 and 49.5 / 50 is 0.99: the border ring dies
        parts = EI.proposal_parts(EI.proposal_mask(levels), levels, None)
        alive = (~parts["dead"][0]).view(50, 50)
        assert bool(alive[1:49, 1:49].all()) and int(alive.sum()) == 48 * 48
    if name == "4x60pad10" and learned == "none":
        parts = EI.proposal_parts(EI.proposal_mask(levels, "plain", 10), levels, None)
        assert parts["vw"][0].tolist() == [50.0] and parts["vh"][0].tolist() == [4.0]
        alive = (~parts["dead"][0]).view(4, 60)
        assert bool(alive[:, 1:49].all()) and int(alive.sum()) == 4 * 48
    if name == "3x2x16" and learned == "none":
        assert parts["level_ok"].tolist() == [True] * 5 + [False] * 11


@pytest.mark.parametrize("name", EI.ASSEMBLY_CASES)
def test_assembly_case_bits_and_counters(name):
    hw, pad_cols, edges = EI.ASSEMBLY_CASES[name]
    for pattern in EI.PATTERNS:
        mask = EI.proposal_mask([hw], pattern, pad_cols)
        parts = EI.proposal_parts(mask, [hw], None)
        _, props32 = AF.proposals_composition(torch.zeros(4, hw[0] * hw[1], 4), mask, [hw])
        assert torch.equal(torch.isinf(props32).all(-1), parts["dead"]) and torch.equal(torch.isinf(props32).any(-1), parts["dead"])
        cnt = EI.proposal_counters(parts, [hw])
        if pattern == "plain":
            assert (int(cnt["rule"][0]) > 0) == ("rule" in edges) and (cnt["trip2"] > 0) == ("trip2" in edges)
            assert int(cnt["rule"][0]) == 0 or "no_rule" not in edges


def test_every_extent_to_599_agrees_in_fp32_and_fp64():
    E = 599
    mask = torch.arange(E)[None, :] >= torch.arange(1, E + 1)[:, None]          # frame e - 1 has valid extent e
    for levels in ([(1, E)], [(E, 1)]):
        parts = EI.proposal_parts(mask, levels, None)
        extent = parts["vw" if levels[0][0] == 1 else "vh"][:, 0]
        assert extent.tolist() == list(range(1, E + 1))
        _, dead32 = _composition_bits(mask, levels, None)
        assert torch.equal(dead32, parts["dead"])
        killed = (~mask & parts["dead"]).sum(1)
        assert not bool(killed[:49].any()) and bool((killed[49:] > 0).all())    # the rule fires from an extent of 50


# ---- selection ----------------------------------------------------------------------------------------------------------------
def _ids(cases):
    return ["%dx%dx%dx%d-%s-h%d" % (s + (l, hc[0])) for s, l, hc in cases]


@pytest.mark.parametrize("shape,logits,hc", EI.SELECT_CASES, ids=_ids(EI.SELECT_CASES))
def test_select_case_holds_its_edges(shape, logits, hc):
    N, S, Q, K = shape
    c = EI.select_case(shape, logits, hc)
    cls = c["cls"]
    assert cls.shape == shape[:2] + (K,) and c["Q"] == Q
    idx, ref, counts = EI.select_oracle(cls, c["hand"], c["obj"], c["prop"], Q, hc)
    assert idx.shape == (N, Q) and ref.shape == (N, Q, 42)
    why = EI.impossible_branches(shape, hc)
    print("MEASURED-CPU %s %s %s: selected rows per source %s, impossible %s" % (shape, logits, hc, counts, why))
    assert all(counts[b] == 0 for b in why)
    assert sum(v > 0 for v in counts.values()) == EI.branches_selected(shape, hc)
    if hc[0] >= K and K >= 14:
        assert set(why) == {"hand"}
    if K == 3:
        assert set(why) == {"obj"}                           # classes 1 and 2 are the hands, class 0 the proposal
    if Q >= 300:
        assert bool(torch.isinf(ref).any())                  # a masked proposal (+inf) among the selected rows
    mx, arg = cls.max(-1)
    nan = torch.isnan(mx)
    if logits in EI.TIE_FREE:
        assert not bool(nan.any()) and all(mx[n].unique().numel() == S for n in range(N))
        c_ref, _ = TS.select_composition(cls, c["hand"], c["obj"], c["prop"], Q, hc)
        assert torch.equal(idx, torch.topk(mx, Q, dim=1)[1]) and torch.equal(ref, c_ref)
    if (logits in ("equal", "zeros") and S > 2) or (logits == "half" and S > 40):
        assert all(mx[n].unique().numel() < (S / 2 if S > 40 else S) for n in range(N))   # heavy ties
    if logits in ("equal", "descending"):
        assert torch.equal(idx, torch.arange(Q)[None, :].expand(N, Q))
    if logits == "ascending":
        assert torch.equal(idx, (S - 1 - torch.arange(Q))[None, :].expand(N, Q))
    if logits == "zeros":
        zero = mx == 0
        assert bool((zero & torch.signbit(mx)).any()) or S < 3
        assert bool((zero & ~torch.signbit(mx)).any()) or S < 3
        if S > 2 and K > 1:                                  # a row holding both zeros: the first is the class
            both = ((cls == 0) & torch.signbit(cls)).any(-1) & ((cls == 0) & ~torch.signbit(cls)).any(-1) & zero
            assert bool(both.any())
    if logits == "inf" and S > 1:
        assert bool((mx == float("inf")).any()) and bool((mx == float("-inf")).any())
        assert bool(((cls == float("inf")).sum(-1) > 1).any()) or K == 1 or S < 4
    if logits == "nan":
        assert bool(nan.any())
        if S > 2:
            assert bool(torch.isnan(cls).all(-1).any()) and 0.03 < nan.float().mean().item() < 0.09 or S < 40
            if "hand" not in why:
                assert bool(nan[:, S - 2].all()) and bool((arg[:, S - 2] == hc[1]).all())
            assert bool((arg[:, S - 1] == 0).all())
            first = torch.isnan(cls).float().argmax(-1)
            assert torch.equal(arg[nan], first[nan])         # the first NaN is the class
            if Q >= S:
                n_nan = int(nan[0].sum())
                assert torch.equal(idx[0, :n_nan], torch.nonzero(nan[0]).flatten())   # NaN rows first, by row index


def test_select_oracle_is_a_stable_descending_sort_with_nan_first():
    cls = torch.tensor([[[1.0, 0.0], [float("nan"), 5.0], [-0.0, -1.0], [0.0, -2.0], [3.0, 3.0], [2.0, float("nan")],
                         [3.0, 1.0], [float("inf"), 0.0], [float("-inf"), float("-inf")]]])
    src = [torch.full((1, 9, 42), float(v)) for v in (1, 2, 3)]
    idx, ref, counts = EI.select_oracle(cls, *src, 9, (1, 7))
    assert idx.tolist() == [[1, 5, 7, 4, 6, 0, 2, 3, 8]]
    assert ref[0, :, 0].tolist() == [3, 1, 3, 3, 3, 3, 3, 3, 3] and counts == dict(hand=1, obj=0, prop=8)


def test_python_side_refusal_and_fallback():
    c = EI.select_case((2, 300, 300, 14), "random", (12, 13))
    args = (c["cls"], c["hand"], c["obj"], c["prop"])
    with pytest.raises(RuntimeError):
        TS.select_queries(*args, 301)
    g = torch.Generator().manual_seed(1)
    big = [torch.randn(1, 8193, k, generator=g) for k in (14, 42, 42, 42)]
    ref, refp, idx = TS.select_queries(*big, 300, return_indices=True)
    c_ref, c_refp = TS.select_composition(*big, 300)
    o_idx, o_ref, _ = EI.select_oracle(*big, 300, TS.HAND_CLASSES)
    assert torch.equal(ref, c_ref) and torch.equal(refp, c_refp) and torch.equal(idx, o_idx) and torch.equal(ref, o_ref)


# ---- embedding and fused node -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", EI.PE_ROWS)
def test_pe_rows_hold_every_special_value(M):
    r = EI.pe_rows(M)
    bits = r.view(torch.int32)
    for v in EI.SPECIALS:
        want = torch.tensor(v, dtype=torch.float32).view(torch.int32)
        assert bool((bits == want).any()), v                 # bitwise: -0.0 and the denormals as themselves
    pe = EI.pe_f64(r)
    assert torch.equal(torch.isnan(pe).view(M, 42, 128).any(-1), torch.isnan(r))
    dev = (TS.pos_embed_composition(r).double() - pe)[~torch.isnan(pe)].abs().max().item()
    print("MEASURED-CPU pe M=%d: composition - fp64 %.2e" % (M, dev))
    assert dev <= EI.PE_BOUND
    assert torch.equal(EI.dim_t64().float(), TS.pe_dim_t("cpu"))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,Nc", EI.NODE_CASES)
def test_node_bound_comes_from_the_fp32_composition(M, Nc, bias):
    c = EI.node_case(M, Nc)
    assert c["r"].shape == (M, 42) and c["w"].shape == (Nc, 5376) and c["gy"].shape == (M, Nc)
    assert not bool(torch.isnan(c["r"]).any())
    dev32, scale = EI.node_dev32(M, Nc, bias)
    assert set(dev32) == ({"y", "grad_w", "grad_b"} if bias else {"y", "grad_w"})
    for n, d in dev32.items():
        print("MEASURED-CPU node (%d, %d) bias=%s %s: dev32 %.2e scale %.2e bound %.2e" % (M, Nc, bias, n, d, scale[n],
                                                                                         EI.node_bound(d)))
        assert math.isfinite(d) and scale[n] > 0 and EI.node_bound(d) == max(4 * d, EI.FLOOR)
