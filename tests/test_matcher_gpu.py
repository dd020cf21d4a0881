"""The HIP matchers (csrc/msda_matcher.hip) on the GPU: cost blocks against the torch composition, the solver against scipy's
stored answers, the drop-ins against the reference-run fixtures (tests/golden/gen_golden_r08.py), errors, no-sync mode,
graph capture and the A/B knob.  No test here needs scipy."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import matcher_inputs as MI   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import matcher
    return matcher


def _flat(result):
    return MI.flatten_indices(result)


def _torch_cost(M, outputs, targets):
    """The composition's [bs, Q, sum T] cost matrix (valid frames' targets) and the valid frames' sizes."""
    if isinstance(targets, dict):
        valid = [f for f in range(MI.BS) if targets["is_valid"][f] == 1]
        ids = torch.tensor([x for f in valid for x in targets["labels"][f]], device=DEV)
        cost = M._class_cost(outputs["pred_logits"], ids)
        if "keypoints" in targets:
            tgt = torch.cat([targets["keypoints"][f] for f in valid])
            hand = (ids == 12) | (ids == 13)
            obj = (ids != 0) & ~hand
            kp = torch.zeros_like(cost)
            kp[:, hand] = torch.cdist(outputs["pred_hand_key"].flatten(0, 1), tgt[hand], p=1)
            kp[:, obj] = torch.cdist(outputs["pred_obj_key"].flatten(0, 1), tgt[obj], p=1)
            C = MI.COST_KEYPOINT * kp + MI.COST_CLASS * cost
        else:
            C = MI.COST_CLASS * cost
        return C.view(MI.BS, MI.Q, -1), [len(targets["labels"][f]) for f in valid]
    ids = torch.cat([v["labels"] for v in targets])
    tgt = torch.cat([v["keypoints"] for v in targets])
    cost = M._class_cost(outputs["pred_logits"], ids)
    kp = torch.zeros_like(cost)
    kp[:, ids != 0] = torch.cdist(outputs["pred_keypoints"].flatten(0, 1), tgt[ids != 0], p=1)
    return (MI.COST_KEYPOINT * kp + MI.COST_CLASS * cost).view(MI.BS, MI.Q, -1), [len(v["keypoints"]) for v in targets]


def _cases():
    arc = np.load(os.path.join(GOLDEN, "matcher_arctic.npz"))
    asm = np.load(os.path.join(GOLDEN, "matcher_assembly.npz"))
    for case in MI.ARCTIC_CASES:
        yield ("arctic_" + case, *MI.to_device(*MI.arctic_case(case, int(arc[case + "_seed"])), DEV),
               {k[len(case) + 1:]: arc[k] for k in arc.files if k.startswith(case + "_")})
    yield ("assembly", *MI.to_device(*MI.assembly_case(int(asm["seed"])), DEV), dict(asm))


def test_cost_blocks_match_torch_composition(M):
    """Debug cost blocks against the torch composition on the same device: max |diff| / max |C| per block below 1e-5
    (measured on one MI355X: 4.8e-7, from expf / logf ulps and the L1 summation order)."""
    worst = 0.0
    for name, outputs, targets, _ in _cases():
        if name == "arctic_no_labels":
            continue
        packed = M.pack_targets(targets, DEV)
        dbg = torch.full((1, MI.BS, MI.Q, packed.t_max), float("nan"), device=DEV)
        res = M.match([outputs], packed, MI.COST_CLASS, MI.COST_KEYPOINT, cost_debug=dbg)
        C, sizes = _torch_cost(M, outputs, targets)
        assert int(res.num_valid) == len(sizes)
        lo = 0
        for k, T in enumerate(sizes):
            if T:
                ref = C[k, :, lo:lo + T]
                got = dbg[0, k, :, :T]
                err = ((got - ref).abs().max() / ref.abs().max()).item()
                worst = max(worst, err)
                assert err < 1e-5, (name, k, err)
            lo += T
    print("cost block worst relative error %.3g" % worst)


def test_lsap_equals_stored_scipy_answers(M):
    from uvhand_amd import _native
    store = np.load(os.path.join(GOLDEN, "matcher_lsap.npz"))
    for Q, T in MI.lsap_shapes():
        qi, ti, count, status = _native.lsap(torch.from_numpy(MI.lsap_matrix(Q, T)).to(DEV))
        assert status.eq(0).all() and count.eq(min(Q, T)).all(), (Q, T)
        np.testing.assert_array_equal(qi.cpu().numpy(), store["rows_%d_%d" % (Q, T)], err_msg="rows %d x %d" % (Q, T))
        np.testing.assert_array_equal(ti.cpu().numpy(), store["cols_%d_%d" % (Q, T)], err_msg="cols %d x %d" % (Q, T))


def test_lsap_ties_reach_scipy_optimum(M):
    from uvhand_amd import _native
    store = np.load(os.path.join(GOLDEN, "matcher_lsap.npz"))
    for Q, T in MI.TIE_SHAPES:
        cost = MI.tie_matrix(Q, T)
        qi, ti, _, status = (t.cpu().numpy() for t in _native.lsap(torch.from_numpy(cost).to(DEV)))
        assert (status == 0).all()
        for b in range(cost.shape[0]):
            assert len(set(qi[b])) == len(set(ti[b])) == min(Q, T)
            total = cost[b].astype(np.float64)[qi[b], ti[b]].sum()
            assert total == store["tie_opt_%d_%d" % (Q, T)][b], (Q, T, b)


def test_lsap_statuses(M):
    from uvhand_amd import _native
    c = torch.rand(3, 5, 2, device=DEV)
    c[1, 2, 0] = float("nan")
    c[2, :, 1] = float("inf")                       # column 1 of block 2 has no finite entry
    _, _, count, status = _native.lsap(c)
    assert status.tolist() == [0, 1, 2] and count.tolist() == [2, 0, 0]
    qi, ti, count, status = _native.lsap(torch.rand(2, 5, 0, device=DEV))
    assert qi.shape == (2, 0) and count.tolist() == [0, 0] and status.tolist() == [0, 0]


def test_drop_ins_equal_reference_fixtures(M):
    for name, outputs, targets, store in _cases():
        cls = M.AssemblyMatcher if name == "assembly" else M.ArcticMatcher
        result = cls(MI.COST_CLASS, MI.COST_KEYPOINT)(outputs, targets)
        if name == "arctic_no_labels":
            assert result == 0
        lens, i, j = _flat(result)
        np.testing.assert_array_equal(lens, store["lens"], err_msg=name)
        np.testing.assert_array_equal(i, store["i"], err_msg=name)
        np.testing.assert_array_equal(j, store["j"], err_msg=name)


def test_nan_logits_raise_scipys_error(M):
    arc = np.load(os.path.join(GOLDEN, "matcher_arctic.npz"))
    outputs, targets = MI.to_device(*MI.arctic_case("all_valid", int(arc["all_valid_seed"])), DEV)
    outputs["pred_logits"][3, 17, :] = float("nan")
    with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
        M.ArcticMatcher(MI.COST_CLASS, MI.COST_KEYPOINT)(outputs, targets)


def _seven_sets(outputs):
    g = torch.Generator(device=DEV).manual_seed(5)
    sets = [outputs]
    for _ in range(6):
        sets.append({k: v + 0.05 * torch.randn(v.shape, generator=g, device=DEV) for k, v in outputs.items()})
    return sets


def test_match_seven_sets_one_launch_no_sync(M):
    from uvhand_amd import _native
    arc = np.load(os.path.join(GOLDEN, "matcher_arctic.npz"))
    outputs, targets = MI.to_device(*MI.arctic_case("interleaved", int(arc["interleaved_seed"])), DEV)
    sets = _seven_sets(outputs)
    packed = M.pack_targets(targets, DEV)
    torch.cuda.synchronize()
    n0 = _native.launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = M.match(sets, packed, MI.COST_CLASS, MI.COST_KEYPOINT)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert _native.launch_count() - n0 == 1
    assert res.query_idx.shape == (7, MI.BS, packed.t_max)
    got = M.indices_from_host(res.buffer.cpu(), 7, MI.BS, packed.t_max, zero_if_empty=True)
    matcher = M.ArcticMatcher(MI.COST_CLASS, MI.COST_KEYPOINT)
    for s in range(7):                               # each set equals its own drop-in call
        ref = matcher(sets[s], targets)
        assert [(a.tolist(), b.tolist()) for a, b in got[s]] == [(a.tolist(), b.tolist()) for a, b in ref]
    assert (res.count[:, int(res.num_valid):] == -1).all()


def test_drop_in_forward_makes_one_sync(M):
    arc = np.load(os.path.join(GOLDEN, "matcher_arctic.npz"))
    outputs, targets = MI.to_device(*MI.arctic_case("interleaved", int(arc["interleaved_seed"])), DEV)
    matcher = M.ArcticMatcher(MI.COST_CLASS, MI.COST_KEYPOINT)
    matcher(outputs, targets)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            matcher(outputs, targets)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in syncs]


def test_match_graph_capture_replays_after_input_changes(M):
    asm = np.load(os.path.join(GOLDEN, "matcher_assembly.npz"))
    outputs, targets = MI.to_device(*MI.assembly_case(int(asm["seed"])), DEV)
    sets = _seven_sets(outputs)
    packed = M.pack_targets(targets, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        M.match(sets, packed, MI.COST_CLASS, MI.COST_KEYPOINT)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = M.match(sets, packed, MI.COST_CLASS, MI.COST_KEYPOINT)
    g = torch.Generator(device=DEV).manual_seed(9)
    for o in sets:
        o["pred_logits"].copy_(torch.randn(o["pred_logits"].shape, generator=g, device=DEV) * 2)
        o["pred_keypoints"].mul_(0.5).add_(0.25)
    graph.replay()
    eager = M.match(sets, packed, MI.COST_CLASS, MI.COST_KEYPOINT)
    torch.cuda.synchronize()
    assert torch.equal(captured.buffer, eager.buffer)


def test_fused_off_runs_the_composition_in_a_child():
    pytest.importorskip("scipy", reason="MSDA_MATCHER_FUSED=0 solves with scipy")
    code = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import matcher_inputs as MI
from uvhand_amd import matcher as M, _native
assert not M.FUSED
store = np.load(os.path.join(%r, "matcher_arctic.npz"))
outputs, targets = MI.to_device(*MI.arctic_case("interleaved", int(store["interleaved_seed"])), torch.device("cuda:0"))
n0 = _native.launch_count()
lens, i, j = MI.flatten_indices(M.ArcticMatcher(MI.COST_CLASS, MI.COST_KEYPOINT)(outputs, targets))
assert _native.launch_count() == n0
assert (lens == store["interleaved_lens"]).all() and (i == store["interleaved_i"]).all() and (j == store["interleaved_j"]).all()
print("composition ok")
""" % (os.path.dirname(HERE), os.path.join(HERE, "golden"), GOLDEN)
    env = dict(os.environ, MSDA_MATCHER_FUSED="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "composition ok" in r.stdout, r.stdout + r.stderr
