"""The drop-in matchers (uvhand_amd/matcher.py) without a GPU: construction, the reference's composition on CPU tensors
against the fixtures made by running the reference's classes (tests/golden/gen_golden_r08.py), and pack_targets."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import matcher_inputs as MI   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def M():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import matcher
    return matcher


def _check(result, store, prefix):
    lens, i, j = MI.flatten_indices(result)
    np.testing.assert_array_equal(lens, store[prefix + "lens"])
    np.testing.assert_array_equal(i, store[prefix + "i"])
    np.testing.assert_array_equal(j, store[prefix + "j"])
    if not isinstance(result, int):
        for a, b in result:
            assert a.dtype == torch.int64 and b.dtype == torch.int64 and not a.is_cuda


def test_construction(M):
    m = M.ArcticMatcher(cost_class=1.5, cost_keypoint=4, cfg="c")
    assert (m.cost_class, m.cost_keypoint, m.cfg) == (1.5, 4, "c")
    a = M.AssemblyMatcher()
    assert (a.cost_class, a.cost_keypoint, a.cfg) == (1, 1, None)
    assert isinstance(m, torch.nn.Module) and list(m.parameters()) == []
    for cls in (M.ArcticMatcher, M.AssemblyMatcher):
        with pytest.raises(AssertionError, match="all costs cant be 0"):
            cls(cost_class=0, cost_keypoint=0)


@pytest.mark.parametrize("case", MI.ARCTIC_CASES)
def test_arctic_composition_matches_reference(M, case):
    pytest.importorskip("scipy", reason="the composition route solves with scipy")
    store = np.load(os.path.join(GOLDEN, "matcher_arctic.npz"))
    outputs, targets = MI.arctic_case(case, int(store[case + "_seed"]))
    result = M.ArcticMatcher(MI.COST_CLASS, MI.COST_KEYPOINT)(outputs, targets)
    if case == "no_labels":
        assert result == 0
    _check(result, store, case + "_")
    assert store[case + "_margins"].size == 0 or store[case + "_margins"].min() >= 1e-3


def test_interleaved_case_pairs_chunk_k_with_frame_k():
    """The quirk the fixture pins: with invalid frames in between, the k-th valid frame's targets are matched against output
    frame k, so the result has one entry per valid frame and its target indices index that chunk."""
    store = np.load(os.path.join(GOLDEN, "matcher_arctic.npz"))
    _, targets = MI.arctic_case("interleaved", int(store["interleaved_seed"]))
    valid = [f for f in range(MI.BS) if targets["is_valid"][f] == 1]
    assert len(store["interleaved_lens"]) == len(valid) < MI.BS
    assert list(store["interleaved_lens"]) == [min(MI.Q, len(targets["labels"][f])) for f in valid]


def test_assembly_composition_matches_reference(M):
    pytest.importorskip("scipy", reason="the composition route solves with scipy")
    store = np.load(os.path.join(GOLDEN, "matcher_assembly.npz"))
    outputs, targets = MI.assembly_case(int(store["seed"]))
    _check(M.AssemblyMatcher(MI.COST_CLASS, MI.COST_KEYPOINT)(outputs, targets), store, "")


def test_lsap_fixture_covers_the_shapes():
    store = np.load(os.path.join(GOLDEN, "matcher_lsap.npz"))
    for Q, T in MI.lsap_shapes():
        rows, cols = store["rows_%d_%d" % (Q, T)], store["cols_%d_%d" % (Q, T)]
        assert rows.shape == cols.shape == (MI.LSAP_B, min(Q, T))
        assert (np.diff(rows, axis=1) > 0).all()


class _NoRead(torch.Tensor):
    """A tensor that refuses every host read of its values (what a device tensor would pay a sync for)."""
    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        name = getattr(func, "__name__", "")
        if name in ("__bool__", "item", "tolist", "__int__", "__float__", "__index__", "__iter__", "numpy", "__array__",
                    "__getitem__"):
            raise AssertionError("pack_targets read a value on the host: %s" % name)
        return super().__torch_function__(func, types, args, kwargs or {})


def test_pack_targets_arctic(M):
    labels = [[12, 3], [], [0, 13, 5]]
    kps = [torch.rand(2, 42), torch.rand(0, 42), torch.rand(3, 42)]
    is_valid = torch.tensor([1.0, 0.0, 1.0]).as_subclass(_NoRead)
    p = M.pack_targets({"labels": labels, "keypoints": kps, "is_valid": is_valid}, "cpu")
    assert p.kind == "arctic" and p.sizes == (2, 0, 3) and p.t_max == 3
    assert p.labels.tolist() == [12, 3, 0, 13, 5] and p.offsets.tolist() == [0, 2, 2, 5]
    assert torch.equal(p.keypoints, torch.cat(kps))
    assert p.is_valid.dtype == torch.int32 and torch.Tensor.tolist(p.is_valid.as_subclass(torch.Tensor)) == [1, 0, 1]


def test_pack_targets_assembly(M):
    tg = [{"labels": torch.tensor([1, 2]), "keypoints": torch.rand(2, 21, 3)},
          {"labels": torch.tensor([0]), "keypoints": torch.rand(1, 21, 3)}]
    p = M.pack_targets(tg, "cpu")
    assert p.kind == "assembly" and p.sizes == (2, 1) and p.is_valid is None
    assert p.labels.tolist() == [1, 2, 0] and p.offsets.tolist() == [0, 2, 3] and p.keypoints.shape == (3, 63)
    with pytest.raises(ValueError):
        M.pack_targets([{"labels": torch.tensor([1]), "keypoints": torch.rand(2, 63)}], "cpu")
