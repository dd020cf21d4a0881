"""The D = 32 launch plan over the sweep of tests/golden/plan_sweep_inputs.py, on the CPU: msda_describe_plan and the two
workspace sizes must be exactly what tests/golden/plan_sweep.npz recorded — every geometry, storage type and flag
combination.  The GPU tests prove which branch they ran from these strings, and the forward and the backward of one
autograd node agree on a buffer's layout through these sizes, so none of them may move unannounced."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import plan_sweep_inputs as PS  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    return PS.record(_native.load()), load_golden("plan_sweep")


def test_sweep_is_the_recorded_one(recorded):
    got, want = recorded
    assert np.array_equal(got["geometry"], want["geometry"]) and np.array_equal(got["calls"], want["calls"])
    assert len(want["geometry"]) >= 300 and want["plan"].size >= 7680


def test_every_plan_string_is_unchanged(recorded):
    got, want = recorded
    g_text, w_text = got["plans"][got["plan"]], want["plans"][want["plan"]]
    diff = np.argwhere(g_text != w_text)
    assert len(diff) == 0, ["%s %s: %s != %s" % (tuple(want["geometry"][g]), tuple(want["calls"][c]), g_text[g, c], w_text[g, c])
                            for g, c in diff[:5]]


@pytest.mark.parametrize("which", ["fwd_ws", "bwd_ws"])
def test_every_workspace_size_is_unchanged(recorded, which):
    got, want = recorded
    diff = np.argwhere(got[which] != want[which])
    assert len(diff) == 0, ["%s flags %d: %d != %d" % (tuple(want["geometry"][g]), f, got[which][g, f], want[which][g, f])
                            for g, f in diff[:5]]


def test_sweep_reaches_every_branch(recorded):
    """(the sweep would prove little if it sat on one side of the thresholds)"""
    _, want = recorded
    text = "\n".join(want["plans"])
    for sub in ("fwd=tiled(split=4", "fwd=tiled(split=2", "fwd=tiled(split=1", "fwd=lds(", "bwd=fused(", "bwd=fused_lds(",
                "bwd=two_launches(", "acc=single", "acc=wide", "acc=tile", "fixed", "prefix", ",det", ",heads_reduce", ",masks",
                "dense_px=0", "dense_px=32", "dense_px=64", "roleA=lds", "roleA=tiled", "prologue unsupported"):
        assert sub in text, sub
    assert (want["fwd_ws"] > 0).any() and (want["bwd_ws"] > want["fwd_ws"]).any()
