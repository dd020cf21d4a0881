"""The input-projection neck on the GPU (csrc/msda_neck.hip through functions/neck_func.py and modules/detr.py).

References are never the code under test: the fp64 composition (input_proj_levels_reference on the CPU, the inputs widened)
and the fp32 composition on the GPU, on the same inputs.  Bound per tensor: 4 x the largest deviation of the fp32 composition
from the fp64 one on that case, with a floor of 16 * 2^-24 relative to the tensor's largest magnitude (the project's margin for
fp32 kernels whose summation order differs from torch's).

Measured on an MI355X, largest |deviation| / largest |fp64 value| over the levels of a case, kernels : fp32 composition:
  mixed     out 2.15e-05 : 2.15e-05; grad_x 5.52e-06 : 4.98e-06; grad_weight 6.44e-06 : 4.79e-06
            grad_bias 6.42e-06 : 4.77e-06; grad_gamma 7.64e-06 : 4.08e-06; grad_beta 9.69e-08 : 1.84e-07
  hidden256 out 2.37e-07 : 2.22e-07; grad_x 7.07e-07 : 5.91e-07; grad_weight 2.89e-07 : 3.15e-07
            grad_bias 1.86e-07 : 1.30e-07; grad_gamma 1.80e-07 : 2.32e-07; grad_beta 9.31e-08 : 8.57e-08
  single    out 1.75e-07 : 1.73e-07; grad_x 2.63e-07 : 1.95e-07; grad_weight 1.34e-07 : 2.03e-07
            grad_bias 2.23e-07 : 1.96e-07; grad_gamma 2.45e-07 : 1.67e-07; grad_beta 1.09e-07 : 1.09e-07
  permuted  out 2.00e-07 : 2.00e-07; grad_x 2.14e-07 : 1.59e-07; grad_weight 1.78e-07 : 1.50e-07
            grad_bias 1.41e-07 : 1.77e-07; grad_gamma 1.38e-07 : 1.45e-07; grad_beta 6.92e-08 : 1.09e-07
  offset    out 1.37e-05 : 2.05e-05; grad_x 1.66e-06 : 5.43e-06; grad_weight 3.99e-06 : 1.08e-05
            grad_bias 8.68e-06 : 3.37e-05; grad_gamma 2.58e-05 : 1.77e-04; grad_beta 9.72e-08 : 6.95e-08
  constant  out 1.90e-07 : 2.85e-06; grad_x 2.48e-07 : 2.48e-07; grad_weight 1.84e-07 : 1.38e-07
            grad_bias 1.37e-07 : 1.16e-07; grad_gamma 1.58e-07 : 5.70e-06; grad_beta 7.64e-08 : 7.64e-08
  large     out 2.10e-07 : 1.53e-07; grad_x 3.60e-07 : 4.15e-07; grad_weight 8.71e-07 : 5.86e-07
            grad_bias 6.60e-07 : 9.21e-07; grad_gamma 3.18e-07 : 1.71e-07; grad_beta 1.67e-07 : 1.00e-07
('mixed' out: its 1x1 level has groups of two elements, where the variance itself is of rounding size in both.)
"""
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import neck_inputs as NI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.neck_func import input_proj_levels, input_proj_levels_reference  # noqa: E402
from uvhand_amd.modules import detr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = 16 * 2.0 ** -24
_cache = {}


def _case(name):
    """The case's three evaluations, computed once: kernels and fp32 composition on the GPU, fp64 composition on the CPU."""
    if name not in _cache:
        args = NI.build(name, device=DEV)
        wide = NI.build(name, dtype=torch.float64)
        n0 = _native.launch_count()
        got = NI.run(input_proj_levels, *args)
        assert _native.launch_count() - n0 == 3
        _cache[name] = (args, got, NI.run(input_proj_levels_reference, *args), NI.run(input_proj_levels_reference, *wide))
    return _cache[name]


@pytest.mark.parametrize("name", list(NI.CASES))
def test_values_and_gradients_against_fp64(name):
    args, got, f32, f64 = _case(name)
    failed = []
    for family in NI.NAMES:
        worst = (0.0, 0.0)
        for l, (a, b, r) in enumerate(zip(got[family], f32[family], f64[family])):
            assert a.shape == r.shape and a.dtype == torch.float32
            scale = float(r.abs().max())
            dev_kernel = float((a.double().cpu() - r).abs().max())
            dev_torch = float((b.double().cpu() - r).abs().max())
            bound = max(4 * dev_torch, FLOOR * scale)
            worst = max(worst, (dev_kernel / (scale + 1e-300), dev_torch / (scale + 1e-300)))
            if not dev_kernel <= bound:
                failed.append((family, l, dev_kernel, bound))
        print("neck %-9s %-11s kernels %.2e  fp32 composition %.2e" % (name, family, worst[0], worst[1]))
    assert not failed, failed


def test_constant_group_statistics():
    """Group 0 of the 'constant' case holds one value: variance 0, so the output is beta exactly (times the mask)."""
    (xs, convs, norms, uniforms, _), got, _, _ = _case("constant")
    cpg = norms[0][1].numel() // NI.GROUPS
    for out, n, u in zip(got["out"], norms, uniforms):
        want = n[2][:cpg].view(1, -1, 1, 1) * (u[:, :cpg] > 0.3)
        assert torch.equal(out[:, :cpg], want.expand_as(out[:, :cpg]))


@pytest.mark.parametrize("name", ["mixed", "large"])
def test_mask_is_the_comparison_exactly(name):
    """Uniforms that hold float32(0.3), its two neighbours, 0 and values next to 1: the output is zero exactly where
    (u > 0.3) is false, and grad_beta of sum(out) — the sum of the mask over frames and pixels — counts exactly the kept ones."""
    (xs, convs, norms, uniforms, _), got, _, _ = _case(name)
    thr = torch.tensor(0.3, dtype=torch.float32)
    for u in uniforms:
        flat = u.view(-1)
        assert flat[0] == thr and flat[1] < thr < flat[2] and flat[3] == 0 and flat[4] < 1       # the edge values are in place
    for out, u in zip(got["out"], uniforms):
        assert torch.equal(out != 0, u > 0.3)
    ones = [torch.ones_like(u) for u in uniforms]
    res = NI.run(input_proj_levels, xs, convs, norms, uniforms, ones)
    for g, u in zip(res["grad_beta"], uniforms):
        assert torch.equal(g, (u > 0.3).sum((0, 2, 3)).float())


def test_gradient_zero_pattern_through_an_elementwise_probe():
    """grad wrt a per-element offset added after the norm would be g * mask; the node exposes it as grad_beta's summands.  With
    one pixel and one frame per channel (H = W = N = 1) grad_beta IS that element: its zero pattern equals (u > 0.3)."""
    from uvhand_amd.functions.neck_func import _NeckFunction
    C = 64
    u = torch.rand(1, C, 1, 1, device=DEV)
    u.view(-1)[:4] = torch.tensor([0.3, 0.29999998, 0.30000004, 0.0])
    y = torch.randn(1, C, 1, 1, device=DEV)
    beta = torch.zeros(C, device=DEV, requires_grad=True)
    out, = _NeckFunction.apply(NI.GROUPS, NI.EPS, 1, True, y, None, torch.ones(C, device=DEV), beta, u)
    g, = torch.autograd.grad((out * torch.randn_like(out).abs().add(0.5)).sum(), beta)
    assert torch.equal(g != 0, (u > 0.3).view(-1))


class _Backbone(torch.nn.Module):
    """Three fixed feature maps with all-false masks; backbone[1] is a sine-free positional stub that reads shapes only."""
    strides, num_channels = [8, 16, 32], [24, 40, 40]

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.maps = [torch.randn(2, c, s, s, generator=g).to(DEV) for c, s in zip(self.num_channels, (12, 6, 3))]

    def __getitem__(self, i):
        return lambda nested: torch.zeros_like(nested.tensors)

    def forward(self, samples):
        feats = [detr.NestedTensor(m, torch.zeros(m.shape[0], m.shape[2], m.shape[3], dtype=torch.bool, device=DEV))
                 for m in self.maps]
        return feats, [torch.zeros(m.shape[0], 64, m.shape[2], m.shape[3], device=DEV) for m in self.maps]


class _Shell(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.backbone = _Backbone()
        self.num_feature_levels = 4
        self.input_proj = detr._input_proj(self.backbone, 64, 4).to(DEV)


def _shell_run(model, fused, monkeypatch, seed=123):
    monkeypatch.setenv("MSDA_NECK_FUSED", fused)
    samples = detr.NestedTensor(torch.zeros(2, 3, 96, 96, device=DEV), torch.zeros(2, 96, 96, dtype=torch.bool, device=DEV))
    torch.manual_seed(seed)
    n0 = _native.launch_count()
    srcs, masks, pos = detr._backbone_inputs(model, samples, random_mask=True)
    return srcs, masks, pos, torch.cuda.get_rng_state(DEV), _native.launch_count() - n0


def test_backbone_inputs_draws_the_compositions_masks(monkeypatch):
    model = _Shell().train()
    a, am, ap, a_state, a_n = _shell_run(model, "1", monkeypatch)
    b, bm, bp, b_state, b_n = _shell_run(model, "0", monkeypatch)
    assert (a_n, b_n) == (1, 0) and len(a) == len(b) == 4 and [t.shape for t in a] == [t.shape for t in b]
    assert a[3].shape[-2:] == (2, 2)
    for x, y in zip(a, b):
        assert torch.equal(x == 0, y == 0) and 0.2 < float((x == 0).float().mean()) < 0.4
        assert float((x - y).abs().max()) < 1e-4
    assert torch.equal(a_state, b_state)
    assert all(torch.equal(x, y) for x, y in zip(am + ap, bm + bp))
    # eval mode: no mask, nothing drawn
    model.eval()
    torch.manual_seed(7)
    before = torch.cuda.get_rng_state(DEV)
    monkeypatch.setenv("MSDA_NECK_FUSED", "1")
    srcs, _, _ = detr._backbone_inputs(model, detr.NestedTensor(torch.zeros(2, 3, 96, 96, device=DEV),
                                                               torch.zeros(2, 96, 96, dtype=torch.bool, device=DEV)), True)
    assert torch.equal(torch.cuda.get_rng_state(DEV), before)
    assert all(float((s == 0).float().mean()) < 0.01 for s in srcs)


def test_bitwise_reproducible():
    """Two forward + backward runs: everything the kernels write is bitwise equal — the outputs, the bias / gamma / beta
    gradients through the whole route, and the conv-output gradient of the node (what torch's conv backward then receives)."""
    from uvhand_amd.functions.neck_func import _NeckFunction
    args, got, _, _ = _case("mixed")
    again = NI.run(input_proj_levels, *args)
    for family in ("out", "grad_bias", "grad_gamma", "grad_beta"):
        assert all(torch.equal(a, b) for a, b in zip(got[family], again[family])), family
    uniforms, weights = args[3], args[4]
    L = len(uniforms)
    ys = [torch.randn(u.shape, device=DEV).requires_grad_(True) for u in uniforms]
    tensors = ys + [c[1] for c in args[1]] + [n[1] for n in args[2]] + [n[2] for n in args[2]] + uniforms
    runs = []
    for _ in range(2):
        outs = _NeckFunction.apply(NI.GROUPS, NI.EPS, L, True, *tensors)
        runs.append(torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, weights)), ys))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def _four_levels(masked=True):
    xs, convs, norms, uniforms, weights = NI.build("mixed", device=DEV)
    pick = lambda v: v[:4] if v is not None else None          # noqa: E731
    return pick(xs), pick(convs), pick(norms), pick(uniforms) if masked else None, pick(weights)


def test_launch_counts_and_no_host_sync():
    args = _four_levels()
    NI.run(input_proj_levels, *args)                               # warm up allocator, conv plans and code objects
    torch.cuda.synchronize()
    xs, convs, norms, uniforms, weights = args
    xs = [x.requires_grad_(True) for x in xs]
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n0 = _native.launch_count()
        outs = input_proj_levels(xs, convs, norms, uniforms)
        n1 = _native.launch_count()
        loss = sum((o * w).sum() for o, w in zip(outs, weights))
        torch.autograd.grad(loss, xs)
        n2 = _native.launch_count()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert (n1 - n0, n2 - n1) == (1, 2)


def _route(args, monkeypatch=None, autocast=False):
    n0 = _native.launch_count()
    if autocast:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got = NI.run(input_proj_levels, *args)
            ref = NI.run(input_proj_levels_reference, *args)
    else:
        got = NI.run(input_proj_levels, *args)
        ref = NI.run(input_proj_levels_reference, *args)
    assert _native.launch_count() == n0
    for family in NI.NAMES:
        assert all(g is not None and torch.equal(g, r) for g, r in zip(got[family], ref[family])), family
    return got


def test_composition_routes(monkeypatch):
    args = NI.build("single", device=DEV)
    _route(args, autocast=True)
    wide = NI.build("single", dtype=torch.float64, device=DEV)
    assert _route(wide)["out"][0].dtype == torch.float64
    monkeypatch.setenv("MSDA_NECK_FUSED", "0")
    _route(args)
    monkeypatch.setenv("MSDA_NECK_FUSED", "1")
    n0 = _native.launch_count()
    NI.run(input_proj_levels, *args)
    assert _native.launch_count() - n0 == 3


def test_eval_mode_makes_no_mask_and_draws_nothing():
    xs, convs, norms, _, weights = _four_levels(masked=False)
    before = torch.cuda.get_rng_state(DEV)
    free0 = _native.launch_count()
    outs = input_proj_levels(xs, convs, norms, None)
    assert _native.launch_count() - free0 == 1 and torch.equal(torch.cuda.get_rng_state(DEV), before)
    ref = input_proj_levels_reference(xs, convs, norms, None)
    for o, r in zip(outs, ref):
        assert float((o - r).abs().max()) < 1e-4 and float((o == 0).float().mean()) < 0.01


def test_graph_capture_matches_eager():
    xs, convs, norms, _, weights = _four_levels(masked=False)
    xs = [x.requires_grad_(True) for x in xs]
    leaves = xs + [c[1].requires_grad_(True) for c in convs] + [n[1].requires_grad_(True) for n in norms] \
        + [n[2].requires_grad_(True) for n in norms]

    def step():
        outs = input_proj_levels(xs, convs, norms, None)
        loss = sum((o * w).sum() for o, w in zip(outs, weights))
        return list(outs) + list(torch.autograd.grad(loss, leaves))

    eager = [t.detach().clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, static))
