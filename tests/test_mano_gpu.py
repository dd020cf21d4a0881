"""MANO on the HIP kernels (csrc/msda_mano.hip) against the manopth fixtures and the fp64 torch restatement.

Tolerances (max |error| over max |reference|): the forward is fp32 throughout, ~1e-7 per operation, so 1e-5 against fp64.
The gradients sum up to 2334 products per pose feature and run through the 15-step chain backward and the Rodrigues backward,
whose 1 / angle factors amplify the fp32 rounding of the pose (most at the smallest angles drawn here); 1e-4."""
import gc
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import mano_inputs as MI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.mano import MANO, MANO_MAX_GROUPS, mano_many, mano_reference  # noqa: E402

pytestmark = pytest.mark.gpu

FWD, GRAD = 1e-5, 1e-4
DEV = torch.device("cuda:0")
_LAYERS = {}


def _layer(side="right", flat=False, dev=DEV):
    key = (side, flat, str(dev))
    if key not in _LAYERS:
        _LAYERS[key] = MANO.from_arrays(**MI.model_arrays(side, flat, dtype=torch.float32)).to(dev)
    return _LAYERS[key]


def _err(a, b):
    return rel_err(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy())


@pytest.mark.parametrize("fixture,flat", [("mano_mean", False), ("mano_flat", True)])
@pytest.mark.parametrize("side", ["right", "left"])
def test_fixture_outputs_and_gradients(fixture, flat, side):
    z = load_golden(fixture)
    m = _layer(side, flat)
    leaves = [torch.from_numpy(z["%s/%s" % (side, k)]).float().to(DEV).requires_grad_(True)
              for k in ("betas", "global_orient", "hand_pose")]
    n0 = _native.launch_count()
    out = m(*leaves)
    assert _native.launch_count() - n0 == 1
    assert rel_err(out.vertices.detach().cpu().numpy(), z[side + "/vertices"]) < FWD
    assert rel_err(out.joints[:, :16].detach().cpu().numpy(), z[side + "/joints"]) < FWD
    seed = next(s for sd, f, s in MI.FIXTURE_CASES.values() if sd == side and f == flat)
    wv, wj = MI.upstream(seed + 100, MI.FIXTURE_B, torch.float32)
    ((out.vertices * wv.to(DEV)).sum() + (out.joints[:, :16] * wj.to(DEV)).sum()).backward()
    for leaf, key in zip(leaves, ("betas", "global_orient", "hand_pose")):
        assert rel_err(leaf.grad.cpu().numpy(), z["%s/grad_%s" % (side, key)]) < GRAD, key


def _random_case(B, seed, hi=np.pi):
    """fp64 inputs: angles in [0.05, hi], a zero-pose hand and a zero-pose joint where the batch allows."""
    mean = None
    betas, go, hp = MI.pose_inputs(seed, B, lo=0.05, hi=hi, mean=mean)
    if B > 1:
        go[1] = 0
        hp[1] = 0
    hp[0, 6:9] = 0
    g = torch.Generator().manual_seed(seed + 1)
    transl = 0.1 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    return betas, go, hp, transl


@pytest.mark.parametrize("mode", ["vertices", "joints", "both"])
@pytest.mark.parametrize("B", [1, 7, 32, 33, 256, 1000])
def test_matches_fp64_restatement(B, mode):
    flat = B % 2 == 1
    m = _layer("right" if B % 3 else "left", flat)
    m64 = MANO.from_arrays(**MI.model_arrays("right" if B % 3 else "left", flat, dtype=torch.float32)).double()
    ins = _random_case(B, 500 + B)
    g = torch.Generator().manual_seed(B)
    wv = torch.randn(B, MI.V, 3, generator=g, dtype=torch.float64) if mode != "joints" else None
    wj = torch.randn(B, 21, 3, generator=g, dtype=torch.float64) if mode != "vertices" else None

    def loss(o):
        return (0 if wv is None else (o.vertices * wv.to(o.vertices)).sum()) + (0 if wj is None else (o.joints * wj.to(o.joints)).sum())

    ref_leaves = [t.clone().requires_grad_(True) for t in ins]
    ref = m64(*ref_leaves)
    loss(ref).backward()
    leaves = [t.float().to(DEV).requires_grad_(True) for t in ins]
    out = m(*leaves)
    n0 = _native.launch_count()
    loss(out).backward()
    assert _native.launch_count() - n0 == 2
    assert _err(out.vertices, ref.vertices) < FWD
    assert _err(out.joints, ref.joints) < FWD
    for a, b, name in zip(leaves, ref_leaves, ("betas", "global_orient", "hand_pose", "transl")):
        assert _err(a.grad, b.grad) < GRAD, name


def _calls(specs):
    """specs: (side, flat, B, seed, betas batch 1?) -> mano_many calls with leaves on the GPU."""
    calls = []
    for side, flat, B, seed, b1 in specs:
        betas, go, hp, tr = _random_case(max(B, 1), seed, hi=2.0)
        ts = [betas[:1] if b1 else betas[:B], go[:B], hp[:B], tr[:B]]
        calls.append((_layer(side, flat),) + tuple(t.float().to(DEV).requires_grad_(True) for t in ts))
    return calls


SPECS = [("right", False, 32, 1, False), ("left", False, 7, 2, False), ("right", True, 0, 3, False),
         ("left", True, 33, 4, True), ("right", False, 1, 5, False)]


def _step(calls, first=0):
    """Outputs (detached: no eager autograd graph outlives the step) and input gradients of a weighted sum; call i of the list
    has weight 1 + first + i on its joints."""
    outs = mano_many(calls)
    loss = sum((o.vertices * 0.5).sum() + (o.joints * (1.0 + first + i)).sum() for i, o in enumerate(outs))
    leaves = [t for c in calls for t in c[1:]]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [t.detach() for o in outs for t in (o.vertices, o.joints)], grads


def test_grouped_matches_separate_calls():
    calls = _calls(SPECS)
    n0 = _native.launch_count()
    outs = mano_many(calls)
    assert _native.launch_count() - n0 == 1
    assert outs[2].vertices.shape == (0, MI.V, 3) and outs[2].joints.shape == (0, 21, 3)
    for c, o in zip(calls, outs):
        s = mano_many([c])[0]
        assert torch.equal(o.vertices, s.vertices) and torch.equal(o.joints, s.joints)
    grouped = _step(calls)[1]
    separate = [g for k, c in enumerate(calls) for g in _step([c], k)[1]]
    for a, b in zip(grouped, separate):
        assert (a is None and b is None) or torch.equal(a, b)


def test_broadcast_betas_gradient_summed():
    m = _layer()
    _, go, hp, _ = _random_case(9, 77)
    b1 = torch.randn(1, 10, dtype=torch.float64)
    leaves = [t.float().to(DEV).requires_grad_(True) for t in (b1, go, hp)]
    out = m(*leaves)
    out.vertices.sum().backward()
    ref_b = b1.expand(9, -1).float().to(DEV).clone().requires_grad_(True)
    ref = m(ref_b, leaves[1].detach(), leaves[2].detach())
    ref.vertices.sum().backward()
    assert torch.equal(out.vertices, ref.vertices)
    assert torch.equal(leaves[0].grad, ref_b.grad.sum(0, keepdim=True))


def test_launch_counts_criterion_shape():
    calls = _calls([("right" if i % 2 else "left", False, 32, 40 + i, False) for i in range(12)])
    n0 = _native.launch_count()
    outs, grads = _step(calls)
    assert _native.launch_count() - n0 == 3
    assert all(g is not None for g in grads)


def test_no_host_sync():
    calls = _calls(SPECS)
    _step(calls)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _step(calls)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_bitwise_reproducible():
    calls = _calls(SPECS)
    r1, r2 = _step(calls), _step(calls)
    assert all(torch.equal(a, b) for a, b in zip(r1[0], r2[0]))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(r1[1], r2[1]))


def test_graph_capture():
    calls = _calls(SPECS)
    eager = _step(calls)
    gc.collect()                      # PyTorch-ROCm: no eager autograd graph may be alive when the capture ends
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(calls)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _step(calls)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager[0], static[0]))
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(eager[1], static[1]))


def _launches(fn):
    n0 = _native.launch_count()
    out = fn()
    return _native.launch_count() - n0, out


def test_fallbacks_take_the_restatement(monkeypatch):
    calls = _calls(SPECS[:2])
    fused = mano_many(calls)
    monkeypatch.setenv("MSDA_MANO_FUSED", "0")
    n, ref = _launches(lambda: mano_many(calls))
    assert n == 0
    for a, b in zip(fused, ref):
        assert _err(a.vertices, b.vertices) < FWD
    monkeypatch.delenv("MSDA_MANO_FUSED")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        n, _ = _launches(lambda: mano_many(calls))
    assert n == 0
    cpu = _layer("right", False, torch.device("cpu"))
    n, _ = _launches(lambda: cpu(*[t.detach().cpu() for t in calls[0][1:]]))
    assert n == 0
    n, _ = _launches(lambda: mano_many([calls[0]] * (MANO_MAX_GROUPS + 1)))
    assert n == 0
    m = MANO.from_arrays(**MI.model_arrays("right", dtype=torch.float32)).to(DEV)
    m.posedirs.requires_grad_(True)
    n, _ = _launches(lambda: m(*calls[0][1:]))
    assert n == 0
    n, _ = _launches(lambda: mano_many([(_layer("right"),) + tuple(t.double() for t in calls[0][1:])]))
    assert n == 0
