"""The envelope cases of tests/golden/matcher_envelope_inputs.py on the CPU, no GPU needed: the fixture regenerates from its
seeds, every case lies inside the envelope `_fused_ok` / `_fusable` route to the kernels, the exclusion cap holds, and the
cases bite.  For the last, what a plausibly wrong kernel would return is computed in fp64 (a greedy row-by-row assignment,
"first minimum wins" instead of scipy's tie rule, an equal path cost taking over a column, slot k paired with frame k instead of the k-th valid frame, a valid-frame
prefix that forgets the carry between rounds, the wide block read untransposed, T clipped to 15, D clipped to 63) and must
differ from the stored answer on at least one frame whose indices tests/test_matcher_envelope_gpu.py compares exactly, in
every case that targets it.  The solver used for that is a numpy restatement of scipy's algorithm (Crouse 2016) with the tie
rule as a parameter; with scipy's rule it reproduces every stored answer."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import matcher_envelope_inputs as EI  # noqa: E402
from uvhand_amd import criterion as CR  # noqa: E402
from uvhand_amd import matcher as M  # noqa: E402

STORE = dict(np.load(os.path.join(GOLDEN, "matcher_envelope.npz")))


def solve(cost, rule="scipy"):
    """scipy's rectangular LSAP step by step in numpy (fp64): (rows, cols) as linear_sum_assignment returns them.  rule:
    "scipy" (among equal minima an unassigned column wins, the last one in the `remaining` order, else the first),
    "first" (the first minimum in the `remaining` order wins), "lowest" (the lowest column index wins) or "path_le" (scipy's
    argmin, but an equal path cost replaces a column's predecessor)."""
    C = np.asarray(cost, np.float64)
    transpose = C.shape[1] < C.shape[0]
    if transpose:
        C = np.ascontiguousarray(C.T)
    nr, nc = C.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col, path = np.full(nr, -1), np.full(nc, -1), np.full(nc, -1)
    for cur in range(nr):
        spc = np.full(nc, np.inf)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        remaining, num, min_val, i, sink = np.arange(nc - 1, -1, -1), nc, 0.0, cur, -1
        while sink == -1:
            SR[i] = True
            js = remaining[:num]
            r = min_val + C[i, js] - u[i] - v[js]
            upd = r <= spc[js] if rule == "path_le" else r < spc[js]
            path[js[upd]] = i
            spc[js[upd]] = r[upd]
            vals = spc[js]
            lowest = vals.min()
            if lowest == np.inf:
                raise ValueError("cost matrix is infeasible")
            ties = np.flatnonzero(vals == lowest)
            if rule in ("scipy", "path_le"):
                free = ties[row4col[js[ties]] == -1]
                index = free[-1] if len(free) else ties[0]
            elif rule == "first":
                index = ties[0]
            else:
                index = ties[np.argmin(js[ties])]
            min_val = lowest
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num -= 1
            remaining[index] = remaining[num]
        u[cur] += min_val
        for i in np.flatnonzero(SR):
            if i != cur:
                u[i] += min_val - spc[col4row[i]]
        v[SC] -= min_val - spc[SC]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transpose:
        order = np.argsort(col4row)
        return col4row[order], order
    return np.arange(nr), col4row


def greedy(cost):
    """Each row of the solved problem (the targets of a tall block, else the queries) takes its cheapest free column."""
    C = np.asarray(cost, np.float64)
    transpose = C.shape[1] < C.shape[0]
    if transpose:
        C = C.T
    used, cols = np.zeros(C.shape[1], bool), []
    for row in C:
        j = int(np.argmin(np.where(used, np.inf, row)))
        used[j] = True
        cols.append(j)
    cols = np.array(cols)
    if transpose:
        order = np.argsort(cols)
        return cols[order], order
    return np.arange(len(cols)), cols


_BLOCKS = {}


def blocks_of(name, frames=None, dims=None):
    """Per set the list of cost blocks the generator solved: the fp64 restatement rounded to fp32, as fp64 numpy."""
    key = (name, None if frames is None else tuple(frames), dims)
    if key not in _BLOCKS:
        sets, targets = EI.convert(*EI.match_case(name), dtype=torch.float64)
        with torch.no_grad():
            _BLOCKS[key] = [[b.float().double().numpy() for b in EI.cost_blocks(M, o, targets, frames, dims)] for o in sets]
    return _BLOCKS[key]


def stored(name, s, k):
    qi, ti = STORE[name + "__qi"][s, k], STORE[name + "__ti"][s, k]
    return qi[qi >= 0].astype(np.int64), ti[ti >= 0].astype(np.int64)


def compared_exactly(name, s, k, T):
    return name in EI.TIE_CASES or STORE[name + "__gap"][s, k] >= EI.bound(EI.MATCH_CASES[name]["Q"], T)


def caught(name, answer, frames=None, dims=None, only=lambda Q, T: True):
    """Whether answer(block) misses the stored indices on a frame the GPU test compares exactly.  `frames`: the frame whose
    targets the wrong kernel pairs with each slot (-1: none, it reports no chunk)."""
    _, targets = EI.match_case(name)
    sizes, valid, Q = EI.frame_sizes(targets), EI.valid_frames(targets), EI.MATCH_CASES[name]["Q"]
    use = valid if frames is None else [f if f >= 0 else 0 for f in frames[:len(valid)]]
    for s, blocks in enumerate(blocks_of(name, None if frames is None else use, dims)):
        for k, f in enumerate(valid):
            if not (compared_exactly(name, s, k, sizes[f]) and only(Q, sizes[f])):
                continue
            if frames is not None and frames[k] < 0:
                return True
            qi, ti = answer(blocks[k]) if blocks[k].shape[1] else (np.zeros(0, np.int64),) * 2
            ref = stored(name, s, k)
            if not (np.array_equal(qi, ref[0]) and np.array_equal(ti, ref[1])):
                return True
    return False


# ---- the fixture -----------------------------------------------------------------------------------------------------------
def test_fixture_regenerates_bit_identically():
    pytest.importorskip("scipy", reason="the generator solves with scipy")
    import gen_matcher_envelope as gen
    fresh = gen.generate()
    assert sorted(fresh) == sorted(STORE)
    for key, value in fresh.items():
        if key.endswith("_version"):
            continue
        assert value.dtype == STORE[key].dtype and value.shape == STORE[key].shape, key
        np.testing.assert_array_equal(value, STORE[key], err_msg=key)


def test_fixture_holds_answers_only():
    assert os.path.getsize(os.path.join(GOLDEN, "matcher_envelope.npz")) < 400 * 1024
    assert str(STORE["scipy_version"]) and all(v.dtype in (np.int16, np.float64) or k.endswith("_version")
                                               for k, v in STORE.items())


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the predicates' device checks pass, the envelope checks remain."""
    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("name", list(EI.MATCH_CASES))
def test_case_inside_the_fused_envelope(name, monkeypatch):
    monkeypatch.setattr(M, "FUSED", True)
    monkeypatch.delenv("MSDA_CRITERION_FUSED", raising=False)
    case = EI.MATCH_CASES[name]
    sets, targets = EI.match_case(name)
    sizes = EI.frame_sizes(targets)
    preds = [v.as_subclass(_OnDevice) for o in sets for v in o.values()]
    assert M._fused_ok(preds[:len(sets[0])], sizes, case["bs"])
    assert CR._fusable(preds, sizes, case["bs"], len(sets))
    assert not M._fused_ok(preds[:1], sizes + [0], case["bs"]) and not CR._fusable(preds, sizes, case["bs"], 17)
    assert max(sizes) == 16 and case["D"] <= 64 and case["bs"] <= 130
    assert sorted(set(sizes)) == list(EI.SIZES)                   # T = 0, 1, 4, 15 and 16 in every batch


def test_table_covers_the_envelope():
    cases = EI.MATCH_CASES
    assert len(cases) <= 40
    for kind in ("arctic", "assembly"):
        assert {c["Q"] for c in cases.values() if c["kind"] == kind} >= {1, 5, 16, 17, 63, 64, 65, 300, 1024}
        assert any(c["sets"] == 7 for c in cases.values() if c["kind"] == kind)
    assert any(c["D"] == 64 for c in cases.values())
    c = cases["arctic_bs130"]
    assert (c["bs"], c["Q"]) == (130, 16) and 0.3 <= len(c["invalid"]) / 130 <= 0.4
    runs = [set(range(lo, lo + n)) for lo, n in EI.BS130_INVALID]
    assert any({63, 64} <= r for r in runs) and any({127, 128} <= r for r in runs)
    _, targets = EI.match_case("arctic_ties_q300")
    assert "keypoints" not in targets and all(len(set(lab)) < len(lab) for lab in targets["labels"] if len(lab) > 5)
    for name, labels in (("arctic_label0", {0}), ("arctic_hands", {12, 13}), ("arctic_objects", set(range(1, 12)))):
        assert {x for lab in EI.match_case(name)[1]["labels"] for x in lab} <= labels
    assert set(sum(EI.MUTANT_TARGETS.values(), ())) <= set(cases)


@pytest.mark.parametrize("name", list(EI.MATCH_CASES))
def test_exclusion_cap_and_stored_answers(name):
    """The stored indices are optimal partial permutations, the numpy solver with scipy's rule gives exactly them, and the
    share of frames under the gap is what the fixture says and within the cap (none for the tie cases)."""
    case = EI.MATCH_CASES[name]
    _, targets = EI.match_case(name)
    sizes, valid = EI.frame_sizes(targets), EI.valid_frames(targets)
    gap = STORE[name + "__gap"]
    assert gap.shape == (case["sets"], len(valid))
    under = 0
    for s, blocks in enumerate(blocks_of(name)):
        for k, f in enumerate(valid):
            T = sizes[f]
            qi, ti = stored(name, s, k)
            assert len(qi) == len(ti) == min(case["Q"], T) and len(set(ti)) == len(ti) and (np.diff(qi) > 0).all()
            under += gap[s, k] < EI.bound(case["Q"], T)
            if T:
                mine = solve(blocks[k])
                assert np.array_equal(mine[0], qi) and np.array_equal(mine[1], ti), (name, s, k)
    share = under / gap.size
    print("EXCLUDED %s %.3f" % (name, share))
    assert share == float(STORE[name + "__excluded"])
    assert share <= (0.0 if name in EI.TIE_CASES else EI.MAX_EXCLUDED)


@pytest.mark.parametrize("kind", EI.LSAP_KINDS)
def test_lsap_matrices(kind):
    """Shapes, feasibility and (for a few shapes, the numpy solver being slow) the stored indices."""
    for Q, T in EI.lsap_shapes():
        cost = EI.lsap_matrix(kind, Q, T)
        rows, cols = (STORE["lsap_%s_%d_%d__%s" % (kind, Q, T, w)] for w in ("rows", "cols"))
        assert rows.shape == cols.shape == (EI.LSAP_B, min(Q, T)) and (np.diff(rows.astype(int), axis=1) > 0).all()
        picked = np.stack([c[r, k] for c, r, k in zip(cost, rows, cols)])
        assert np.isfinite(picked).all()
        if kind == "inf":
            share = np.isinf(cost).mean() if Q * T > 16 else None
            assert share is None or 0.05 <= share <= 0.5, (Q, T, share)
        if Q <= 64:
            for b in range(EI.LSAP_B):
                mine = solve(cost[b])
                assert np.array_equal(mine[0], rows[b]) and np.array_equal(mine[1], cols[b]), (kind, Q, T, b)
    if kind in ("ties", "dup_cols"):                              # the tie rule decides: the other rule gives other indices
        differ = 0
        for Q, T in EI.lsap_shapes():
            if Q <= 64:
                cost = EI.lsap_matrix(kind, Q, T)
                differ += sum(not np.array_equal(solve(cost[b], "first")[1], STORE["lsap_%s_%d_%d__cols" % (kind, Q, T)][b])
                              for b in range(EI.LSAP_B))
        assert differ > 0


# ---- the cases bite ----------------------------------------------------------------------------------------------------------
def _no_carry_frames(name):
    """The frame a slot gets when the prefix over is_valid restarts its count in every round of blockDim.x frames."""
    case = EI.MATCH_CASES[name]
    threads = (max(case["Q"], 16) + 63) // 64 * 64
    _, targets = EI.match_case(name)
    frames = [-1] * case["bs"]
    for f0 in range(0, case["bs"], threads):
        rank = 0
        for f in range(f0, min(f0 + threads, case["bs"])):
            if targets["is_valid"][f] == 1:
                frames[rank] = f
                rank += 1
    return frames


def _untransposed(block):
    """The wide branch (Q <= T) with sh.stage read as it was written: thread j's row i gets C[j, i] (0 past the Q rows
    the query threads wrote)."""
    Q, T = block.shape
    m = np.zeros((Q, T))
    m[:, :Q] = block[:, :Q].T
    return solve(m)


MUTANTS = [(m, name) for m, names in EI.MUTANT_TARGETS.items() for name in names]


@pytest.mark.parametrize("mutant,name", MUTANTS)
def test_mutant_is_caught(mutant, name):
    case = EI.MATCH_CASES[name]
    if mutant == "greedy":
        assert caught(name, greedy)
    elif mutant == "first_min":
        assert caught(name, lambda b: solve(b, "first"))
    elif mutant == "path_le":
        assert caught(name, lambda b: solve(b, "path_le"))
    elif mutant == "slot_is_frame":
        assert caught(name, solve, frames=list(range(case["bs"])))
    elif mutant == "prefix_no_carry":
        assert (max(case["Q"], 16) + 63) // 64 * 64 < case["bs"]
        assert caught(name, solve, frames=_no_carry_frames(name))
    elif mutant == "wide_untransposed":
        assert caught(name, _untransposed, only=lambda Q, T: T >= Q and T > 0)
    elif mutant == "t_clip15":
        assert caught(name, lambda b: solve(b[:, :15]), only=lambda Q, T: T == 16)
    elif mutant == "d_clip63":
        assert case["D"] == 64
        assert caught(name, solve, dims=63)
    else:
        raise AssertionError(mutant)
