"""The grouped fp32-MFMA GEMM kernels (csrc/msda_heads.hip, csrc/msda_smoother.hip) at edge shapes against fp64 on the CPU.

Each case of tests/golden/gemm_edge_inputs.py runs forward and backward through detr_heads / motion_smoothers; outputs, input
gradients and every parameter gradient are compared with detr_heads_reference / motion_smoothers_reference (train mode: the
masked composition with the kernels' own dropout masks) on .double() copies.  Every tensor is compared as a whole and per
region (the rows of the last 64-row tile, the last 64-column tile and, for the heads, each weight-gradient chunk's
contribution, from a backward whose loss weights keep only that chunk's rows), each region against its own maximum.  The
tolerances and their derivation live in the case table; tests/test_gemm_edges.py shows each case misses a wrong kernel by at
least 10 times them."""
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gemm_edge_inputs as EI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.heads_func import detr_heads  # noqa: E402
from uvhand_amd.functions.smoother_func import motion_smoothers  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 1234


def _check(kind, name, errs):
    """Print the worst error / tolerance per region (chunk regions pooled) and fail on any region above its tolerance."""
    worst = {}
    for (sname, key, region), (err, tol) in errs.items():
        r = region if sname == "full" else "chunks"
        if r not in worst or err / tol > worst[r][0] / worst[r][1]:
            worst[r] = (err, tol, sname + ":" + key)
    for r, (err, tol, where) in sorted(worst.items()):
        print("EDGE %s %s %-9s err %.3e tol %.3e (%s)" % (kind, name, r, err, tol, where))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, sorted(bad.items())[:10]


@pytest.mark.parametrize("name", list(EI.HEADS_CASES))
def test_heads_edges(name):
    kind, _, L, B, Q, C, K, R, _ = EI.HEADS_CASES[name]
    assert _native.heads_supported(C)
    (kind, mods, hs, init, inter), _, weights, sets, ref, _ = EI.heads_reference(name)
    cls, mlps, sh = mods
    g_mods = (cls.to(DEV), [m.to(DEV) for m in mlps], sh.to(DEV) if sh is not None else None)
    to = [t.to(DEV) if t is not None else None for t in (hs, init, inter)]
    got, _, launches = EI.heads_results(kind, g_mods, *to, weights, sets, detr_heads, count=_native.launch_count)
    # the fused route (test_detr_gpu.test_launch_counts); without keypoint MLPs depths 2 and 3 and their input gradients
    # have no tiles and launch nothing
    assert launches == ((3, 5) if mlps else (1, 3))
    errs = EI.compare(got, ref, lambda k, s: EI.heads_regions(name, k, s), lambda k: EI.heads_tol(name, k))
    _check("heads", name, errs)


def _masks(name, seed_t):
    p = EI.SMOOTHER_CASES[name][6]
    return {k: _native.smoother_dropout_mask(seed_t, k[0] * 3 + k[1], k[2], rows, n, p).cpu()
            for k, (rows, n) in EI.smoother_mask_shapes(name).items()}


@pytest.mark.parametrize("name", list(EI.SMOOTHER_CASES))
def test_smoother_edges(name):
    T, O, H, R, nb, calls, p, _ = EI.SMOOTHER_CASES[name]
    assert _native.smoother_supported(T, O, H, R, nb)
    train = p is not None
    masks = None
    if train:
        torch.cuda.manual_seed(SEED)                    # the seed motion_smoothers draws below
        masks = _masks(name, torch.empty((), dtype=torch.int64, device=DEV).random_().view(1))
        assert all(0 < m.mean().item() < 1 for m in masks.values())
    (mods, xs), _, weights, ref = EI.smoother_reference(name, masks)
    g_mods = [m.to(DEV) for m in mods]

    def fn(leaves, ms):
        torch.cuda.manual_seed(SEED)
        return motion_smoothers(leaves, ms, train)

    got, launches = EI.smoother_results(g_mods, [(m, x.to(DEV)) for m, x in xs], weights, {"full": None}, fn,
                                        count=_native.launch_count)
    assert launches == (2 * nb + 3, 2 * nb + 5)         # the fused route (test_smoother_gpu.test_launch_counts)
    errs = EI.compare(got, ref, lambda k, s: EI.smoother_regions(name, k, s), lambda k: EI.smoother_tol(name, k))
    _check("smoother", name, errs)
