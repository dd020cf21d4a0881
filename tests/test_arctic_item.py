"""get_arctic_item / perturb_arctic_item on the CPU against the reference's fixtures (gen_golden_r11.py)."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import smoother_inputs as SI  # noqa: E402
from uvhand_amd.arctic_item import DEFAULT_SCALE, get_arctic_item, perturb_arctic_item  # noqa: E402


@pytest.mark.parametrize("case", SI.ITEM_CASES)
def test_selection_matches_fixture(case):
    z = load_golden("arctic_item")
    o = SI.item_outputs(case)
    assert np.array_equal(o["pred_logits"].numpy(), z[case + "/in/pred_logits"], equal_nan=True)
    res = SI.flatten(get_arctic_item(o, SI.Cfg()))
    assert len(res) == 9
    for i, t in enumerate(res):
        assert t.dtype == torch.float32
        assert np.array_equal(t.numpy(), z["%s/out%d" % (case, i)]), i


def test_results_are_fresh_tensors():
    o = SI.item_outputs("ties")
    before = [t.clone() for t in o["pred_cams"]]
    res = get_arctic_item(o, SI.Cfg())
    for group in res:
        for t in group:
            t.add_(1.0)
    assert all(torch.equal(a, b) for a, b in zip(before, o["pred_cams"]))


def test_perturb_keep_rate_and_scales():
    torch.manual_seed(5)
    n = 200000
    items = [[torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 3)], [torch.zeros(n, 48)] * 1 + [torch.zeros(n, 48)],
             [torch.zeros(n, 10), torch.zeros(n, 10)], [torch.zeros(n, 3), torch.zeros(n, 1)]]
    out = perturb_arctic_item(items, p_mask=0.05)
    assert out is items
    for g, group in enumerate(items):
        for p, t in enumerate(group):
            s = DEFAULT_SCALE[g][p] if isinstance(DEFAULT_SCALE[g], list) else DEFAULT_SCALE[g]
            changed = t != 0
            rate = changed.float().mean().item()
            sigma = (0.05 * 0.95 / t.numel()) ** 0.5
            assert abs(rate - 0.05) < 5 * sigma, (g, p, rate)
            std = t[changed].std().item()
            assert abs(std / s - 1) < 0.05, (g, p, std)


def test_perturb_leaves_unmasked_values():
    torch.manual_seed(6)
    x = torch.randn(1000, 48)
    items = [[x.clone()]]
    perturb_arctic_item(items, p_mask=0.0, scale=[[1.0]])
    assert torch.equal(items[0][0], x)
