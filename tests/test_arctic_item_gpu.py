"""get_arctic_item on the HIP kernels (csrc/msda_arctic_item.hip) against the reference's fixtures and the restatement."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import smoother_inputs as SI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.arctic_item import get_arctic_item, get_arctic_item_reference  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _to(o, requires_grad=False):
    return {"pred_logits": o["pred_logits"].to(DEV),
            **{k: [t.to(DEV).requires_grad_(requires_grad) for t in o[k]]
               for k in ("pred_cams", "pred_mano_params", "pred_obj_params")}}


@pytest.mark.parametrize("case", SI.ITEM_CASES)
def test_selection_matches_fixture(case):
    z = load_golden("arctic_item")
    o = _to(SI.item_outputs(case))
    n0 = _native.launch_count()
    res = SI.flatten(get_arctic_item(o, SI.Cfg()))
    assert _native.launch_count() - n0 == 1
    for i, t in enumerate(res):
        assert t.is_cuda and t.dtype == torch.float32
        assert np.array_equal(t.cpu().numpy(), z["%s/out%d" % (case, i)]), (case, i)


@pytest.mark.parametrize("case", ["same_query", "ties"])
def test_backward_matches_restatement(case):
    o_cpu = SI.item_outputs(case)
    o = _to(o_cpu, requires_grad=True)
    ref = {"pred_logits": o_cpu["pred_logits"],
           **{k: [t.clone().requires_grad_(True) for t in o_cpu[k]] for k in ("pred_cams", "pred_mano_params", "pred_obj_params")}}
    g = torch.Generator().manual_seed(1)
    res = SI.flatten(get_arctic_item(o, SI.Cfg()))
    weights = [torch.randn(t.shape, generator=g) for t in res]
    loss = sum((t * w.to(DEV)).sum() for t, w in zip(res, weights))
    n0 = _native.launch_count()
    loss.backward()
    assert _native.launch_count() - n0 == 1
    rres = SI.flatten(get_arctic_item_reference(ref, SI.Cfg()))
    sum((t * w).sum() for t, w in zip(rres, weights)).backward()
    for k in ("pred_cams", "pred_mano_params", "pred_obj_params"):
        for a, b in zip(o[k], ref[k]):
            np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=1e-6, atol=1e-6)
