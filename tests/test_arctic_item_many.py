"""get_arctic_item_many on the CPU: the per-set calls it falls back to, against get_arctic_item and the reference's fixtures."""
import sys

import numpy as np
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import smoother_inputs as SI  # noqa: E402
from uvhand_amd.arctic_item import get_arctic_item, get_arctic_item_many  # noqa: E402


def test_many_equals_per_set_calls():
    sets = [SI.item_outputs(c) for c in SI.ITEM_CASES]
    many = get_arctic_item_many(sets, SI.Cfg())
    assert isinstance(many, list) and len(many) == len(sets)
    for o, res in zip(sets, many):
        one = get_arctic_item(o, SI.Cfg())
        assert [len(g) for g in res] == [3, 2, 2, 2]
        for a, b in zip(SI.flatten(res), SI.flatten(one)):
            assert a.dtype == torch.float32 and torch.equal(a, b)


def test_many_matches_fixture():
    z = load_golden("arctic_item")
    many = get_arctic_item_many([SI.item_outputs(c) for c in SI.ITEM_CASES], SI.Cfg())
    for case, res in zip(SI.ITEM_CASES, many):
        for i, t in enumerate(SI.flatten(res)):
            assert np.array_equal(t.numpy(), z["%s/out%d" % (case, i)]), (case, i)


def test_many_takes_one_set_and_bf16_sources():
    o = SI.item_outputs("ties")
    for k in ("pred_cams", "pred_mano_params", "pred_obj_params"):
        o[k] = [t.to(torch.bfloat16) for t in o[k]]
    (res,) = get_arctic_item_many([o], SI.Cfg())
    one = get_arctic_item(o, SI.Cfg())
    for a, b in zip(SI.flatten(res), SI.flatten(one)):
        assert a.dtype == torch.float32 and torch.equal(a, b)
