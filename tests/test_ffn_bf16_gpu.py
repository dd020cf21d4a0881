"""The bf16-autocast form of the layers' FFN (csrc/msda_ffn_bf16.hip, reached with MSDA_FFN_BF16=1 under bf16 autocast): routes
and dtypes, accuracy against an fp64 evaluation of the same FFN, the rounding points bit for bit, the launch budget, bitwise
reproducibility, the dropout mask, graph capture, and one encoder and one decoder layer.

Accuracy rule (the package's rule for a fused form against torch's own route, tests/test_heads_bf16_gpu.py): for the output and
every gradient the node's maximum absolute error against fp64 is at most 4 times the composition's own error against fp64 on the
same inputs, where the composition's error counts as at least one bf16 ulp of the tensor's largest magnitude.  In evaluation
the composition is torch's autocast route (knob off); in training it is fused_ffn_bf16_reference on the GPU with
ffn_keep_mask's mask of the node's seed, since nn.Dropout draws another mask.  Each test prints the ratios it measured; on an
MI355X they were 0.42 to 0.99 for y and 0.00 to 1.00 for the gradients over the cases below, but for one evaluation case
(M = 63, C = F = 64, bf16 x) with 3.00 to 3.65 for gx, gW1 and gb1."""
import gc
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from uvhand_amd import _native
from uvhand_amd.functions.linear_func import (_FusedFFNAmpFn, bracket_linear, ffn_keep_mask, fused_ffn,
                                              fused_ffn_bf16_reference)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
FACTOR = 4.0
CASES = [(1, 64, 64), (63, 64, 64), (64, 64, 128), (65, 128, 192), (129, 256, 1024), (130, 256, 2048)]
NAMES = ("y", "gx", "gW1", "gb1", "gW2", "gb2")


def _id(case):
    return "M%d-C%d-F%d" % case


@pytest.fixture
def knob(monkeypatch):
    monkeypatch.setenv("MSDA_FFN_BF16", "1")
    return monkeypatch


def _amp(dtype=BF):
    return torch.autocast("cuda", dtype=dtype)


def _layers(C, Fh, p=0.0, seed=0, **kw):
    torch.manual_seed(seed)
    return nn.Linear(C, Fh, **kw).to(DEV), nn.Dropout(p).to(DEV), nn.Linear(Fh, C, **kw).to(DEV)


def _data(M, C, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, C, generator=g).to(DEV).to(dtype), torch.randn(M, C, generator=g).to(DEV).to(BF)


def _params(l1, l2):
    return [l1.weight, l1.bias, l2.weight, l2.bias]


def _run(fn, x, go, l1, l2, saved_a=False):
    """fn(x) -> y under bf16 autocast; returns (y, gx, gW1, gb1, gW2, gb2) and y's grad_fn (saved_a: and the node's saved a,
    read before the backward frees it)."""
    x = x.detach().clone().requires_grad_(True)
    for p in _params(l1, l2):
        p.grad = None
    with _amp():
        y = fn(x)
    a = y.grad_fn.saved_tensors[1].clone() if saved_a else None
    y.backward(go.to(y.dtype))
    out = [y.detach(), x.grad] + [p.grad for p in _params(l1, l2)]
    return (out, y.grad_fn, a) if saved_a else (out, y.grad_fn)


def _fp64(x, go, l1, l2, p=0.0, keep=None):
    x = x.detach().double().requires_grad_(True)
    w1, b1, w2, b2 = (t.detach().double().requires_grad_(True) for t in _params(l1, l2))
    a = torch.relu(x @ w1.t() + b1)
    if keep is not None:
        a = a * keep.double() / (1.0 - p)
    y = a @ w2.t() + b2
    y.backward(go.double())
    return [y.detach(), x.grad, w1.grad, b1.grad, w2.grad, b2.grad]


def _bf16_ulp(x):
    m = float(x.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 7) if m > 0 else 2.0 ** -133


def _check_against_fp64(node, comp, ref, what):
    ratios = []
    for name, a, b, r in zip(NAMES, node, comp, ref):
        assert a.shape == r.shape and a.dtype == b.dtype, name
        assert torch.isfinite(a.float()).all(), name
        e_node = float((a.double() - r).abs().max())
        e_comp = max(float((b.double() - r).abs().max()), _bf16_ulp(r))
        ratios.append((name, e_node / e_comp))
    print("%s: node error / composition error against fp64: %s" % (what, ", ".join("%s %.3f" % x for x in ratios)))
    worst = max(ratios, key=lambda x: x[1])
    assert worst[1] <= FACTOR, "%s: %.3f times the composition's error" % worst
    return ratios


@pytest.mark.parametrize("xdtype", [torch.float32, BF], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_accuracy_in_evaluation(case, xdtype, knob):
    M, C, Fh = case
    l1, drop, l2 = _layers(C, Fh, 0.1)
    for m in (l1, drop, l2):
        m.eval()
    x, go = _data(M, C, xdtype)
    fn = lambda t: fused_ffn(t, l1, F.relu, drop, l2)
    node, grad_fn = _run(fn, x, go, l1, l2)
    assert "FusedFFNAmpFn" in type(grad_fn).__name__
    knob.delenv("MSDA_FFN_BF16")
    comp, grad_fn = _run(fn, x, go, l1, l2)
    assert "FusedFFNAmpFn" not in type(grad_fn).__name__
    assert node[0].dtype == BF and node[1].dtype == xdtype and all(g.dtype == torch.float32 for g in node[2:])
    _check_against_fp64(node, comp, _fp64(x, go, l1, l2), "eval %s %s" % (_id(case), xdtype))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("xdtype", [torch.float32, BF], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_accuracy_in_training(case, xdtype, p, knob):
    M, C, Fh = case
    l1, drop, l2 = _layers(C, Fh, p)
    x, go = _data(M, C, xdtype)
    torch.manual_seed(11)
    node, grad_fn = _run(lambda t: fused_ffn(t, l1, F.relu, drop, l2), x, go, l1, l2)
    assert "FusedFFNAmpFn" in type(grad_fn).__name__
    torch.manual_seed(11)
    seed = torch.empty((), dtype=torch.int64, device=DEV).random_().view(1)
    assert torch.equal(seed, grad_fn.seed)                                  # drawn with one random_() on a device scalar
    keep = ffn_keep_mask(seed, M, Fh, p)
    comp, _ = _run(lambda t: fused_ffn_bf16_reference(t, *_params(l1, l2), p, keep), x, go, l1, l2)
    _check_against_fp64(node, comp, _fp64(x, go, l1, l2, p, keep), "train p=%.1f %s %s" % (p, _id(case), xdtype))


def _exact_inputs(M, C, Fh, xdtype):
    """Small integers and powers of two: every product and every sum below is exact in fp32 in any order (asserted by the
    caller), while h = integers + sixty-fourths needs its bf16 rounding."""
    g = torch.Generator().manual_seed(3)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    l1, drop, l2 = _layers(C, Fh, 0.5)
    with torch.no_grad():
        l1.weight.copy_(ri(-1, 1, Fh, C))
        l1.bias.copy_(ri(-32, 32, Fh) / 64)
        l2.weight.copy_(ri(-1, 1, C, Fh) / 8)
        l2.bias.copy_(ri(-8, 8, C) / 8)
    return l1, drop, l2, ri(-2, 2, M, C).to(DEV).to(xdtype), ri(-2, 2, M, C).to(DEV).to(BF)


@pytest.mark.parametrize("xdtype", [torch.float32, BF], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("case", [(65, 128, 192), (130, 256, 2048)], ids=_id)
def test_rounding_points_bit_for_bit(case, xdtype, knob):
    """On inputs whose products and sums are exact in fp32 (p = 0.5: scale 2), y, a, gx and the four parameter gradients equal
    fused_ffn_bf16_reference and its autograd bit for bit: a rounding in another place, or one too many, shows."""
    M, C, Fh = case
    l1, drop, l2, x, go = _exact_inputs(M, C, Fh, xdtype)
    torch.manual_seed(5)
    node, grad_fn, a_node = _run(lambda t: fused_ffn(t, l1, F.relu, drop, l2), x, go, l1, l2, saved_a=True)
    assert "FusedFFNAmpFn" in type(grad_fn).__name__
    keep = ffn_keep_mask(grad_fn.seed, M, Fh, 0.5)
    ref, _ = _run(lambda t: fused_ffn_bf16_reference(t, *_params(l1, l2), 0.5, keep), x, go, l1, l2)
    # the restated a, and the conditions of exactness: every sum of absolute terms, in units of its terms' quantum, below 2^24
    w1, b1, w2, b2 = (t.detach().double() for t in _params(l1, l2))
    h64 = x.double() @ w1.t() + b1
    h = h64.to(torch.float32).to(BF)
    assert int((h.double() != h64).sum()) > 0                                # some h need the rounding
    a = (torch.relu(h).float() * 2.0 * keep.float()).to(BF)
    gh = ((go.double() @ w2) * 2.0 * (a > 0).double()).to(torch.float32).to(BF)
    for terms, quantum in (((x.double().abs() @ w1.abs().t() + b1.abs()), 2.0 ** -6),
                           ((a.double().abs() @ w2.abs().t() + b2.abs()), 2.0 ** -8),
                           ((go.double().abs() @ w2.abs()) * 2.0, 2.0 ** -3),
                           ((gh.double().abs() @ w1.abs()), 2.0 ** -2),
                           ((go.double().abs().t() @ a.double().abs()), 2.0 ** -5),
                           ((gh.double().abs().t() @ x.double().abs()), 2.0 ** -2)):
        assert float(terms.max()) / quantum < 2 ** 24
    assert torch.equal(a_node, a)
    for name, got, want in zip(NAMES, node, ref):
        assert got.dtype == want.dtype and torch.equal(got, want), name
    assert torch.equal(node[0].double(), (a.double() @ w2.t() + b2).to(torch.float32).to(BF).double())


def _count(fn):
    before = _native.launch_count()
    out = fn()
    torch.cuda.synchronize()
    return out, _native.launch_count() - before


def test_knob_off_is_the_composition_with_its_launches(monkeypatch):
    l1, drop, l2 = _layers(256, 1024, 0.0)
    x, go = _data(130, 256, torch.float32)
    comp = lambda t: bracket_linear(drop(F.relu(bracket_linear(t, l1))), l2)
    (want, _), n_want = _count(lambda: _run(comp, x, go, l1, l2))
    for value in (None, "", "0"):
        if value is None:
            monkeypatch.delenv("MSDA_FFN_BF16", raising=False)
        else:
            monkeypatch.setenv("MSDA_FFN_BF16", value)
        (got, grad_fn), n = _count(lambda: _run(lambda t: fused_ffn(t, l1, F.relu, drop, l2), x, go, l1, l2))
        assert "FusedFFNAmpFn" not in type(grad_fn).__name__ and n == n_want
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_routes_with_the_knob_on(knob):
    l1, drop, l2 = _layers(256, 1024, 0.1)
    x = torch.randn(2, 65, 256, device=DEV, requires_grad=True)

    def ffn(t, layers, act=F.relu, dtype=BF, grad=True):
        with _amp(dtype), torch.set_grad_enabled(grad):
            return fused_ffn(t, layers[0], act, layers[1], layers[2])

    mine = (l1, drop, l2)
    y = ffn(x, mine)
    assert type(y.grad_fn).__name__ == _FusedFFNAmpFn.__name__ + "Backward" and y.dtype == BF and y.shape == x.shape
    assert "FusedFFNAmpFn" in type(ffn(x.to(BF), mine).grad_fn).__name__
    # grad mode off: the node's launch all the same (one library launch, no grad_fn)
    y, n = _count(lambda: ffn(x, mine, grad=False))
    assert y.grad_fn is None and y.dtype == BF and n == 1
    # everything else keeps the composition
    x72 = torch.randn(5, 72, device=DEV, requires_grad=True)
    others = {
        "fp16 autocast": lambda: ffn(x, mine, dtype=torch.float16),
        "gelu": lambda: ffn(x, mine, act=F.gelu),
        "no bias": lambda: ffn(x, _layers(256, 1024, 0.1, bias=False)),
        "C = 72": lambda: ffn(x72, _layers(72, 128, 0.1)),
        "bf16 parameters": lambda: ffn(x, tuple(m.to(BF) for m in _layers(256, 1024, 0.1))),
    }
    for name, fn in others.items():
        y = fn()
        assert y.grad_fn is not None and "FusedFFNAmpFn" not in type(y.grad_fn).__name__, name
    y = fused_ffn(x, l1, F.relu, drop, l2)                                  # no autocast: today's fp32 node
    assert type(y.grad_fn).__name__ == "_FusedFFNFnBackward" and y.dtype == torch.float32


def test_views_of_x_give_the_bits_of_a_contiguous_x(knob):
    """A strided x and a bf16 x at an 8-byte offset (the kernels move 16 bytes) are copied first: the same y and gx."""
    M, C, Fh = 65, 128, 192
    l1, drop, l2 = _layers(C, Fh, 0.0)
    _, go = _data(M, C, BF)
    wide = torch.randn(M, C + 8, device=DEV)
    flat = torch.randn(M * C + 4, device=DEV).to(BF)
    for base, take in ((wide, lambda t: t[:, 4:4 + C]), (flat, lambda t: t[4:].view(M, C))):
        outs = []
        for copy_first in (False, True):
            leaf = base.clone().requires_grad_(True)
            view = take(leaf)
            assert not view.is_contiguous() or view.data_ptr() % 16
            with _amp():
                y = fused_ffn(view.clone() if copy_first else view, l1, F.relu, drop, l2)
            assert "FusedFFNAmpFn" in type(y.grad_fn).__name__
            y.backward(go)
            outs.append((y.detach(), leaf.grad))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert outs[0][1].shape == base.shape and outs[0][1].dtype == base.dtype


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_launch_budget(case, knob):
    """Forward: 1 library launch.  Backward: at most 5 (gh, gx, two weight-gradient first stages, their one second stage; the
    second stage exists once the rows split, which they do from 65 rows on); 2 with frozen weights (gh, gx); 4 or fewer with
    an x that needs no gradient; only gW2's with nothing but linear2 trained."""
    M, C, Fh = case
    l1, drop, l2 = _layers(C, Fh, 0.1)
    x, go = _data(M, C, torch.float32)

    def step(x_grad=True, w1_grad=True, w2_grad=True):
        for p, on in zip(_params(l1, l2), (w1_grad, w1_grad, w2_grad, w2_grad)):
            p.requires_grad_(on)
            p.grad = None
        xi = x.detach().clone().requires_grad_(x_grad)
        with _amp():
            y, nf = _count(lambda: fused_ffn(xi, l1, F.relu, drop, l2))
        if y.grad_fn is None:
            return nf, 0, xi
        _, nb = _count(lambda: y.backward(go))
        return nf, nb, xi

    nf, nb, xi = step()
    assert nf == 1 and nb <= 5 and (nb == 5 or M < 65), (nf, nb)
    assert xi.grad is not None and all(p.grad is not None for p in _params(l1, l2))
    nf, nb_frozen, xi = step(w1_grad=False, w2_grad=False)
    assert nf == 1 and nb_frozen == 2 and xi.grad is not None and all(p.grad is None for p in _params(l1, l2))
    nf, nb_nox, xi = step(x_grad=False)
    assert nf == 1 and nb_nox == nb - 1 and xi.grad is None
    nf, nb_w2, xi = step(x_grad=False, w1_grad=False)
    assert nf == 1 and nb_w2 <= 2 and l2.weight.grad is not None and l1.weight.grad is None
    nf, nb_none, _ = step(x_grad=False, w1_grad=False, w2_grad=False)
    assert nf == 1 and nb_none == 0


@pytest.mark.parametrize("xdtype", [torch.float32, BF], ids=["x-fp32", "x-bf16"])
def test_reproducible_and_seeded(xdtype, knob):
    """Two runs under one seed are bitwise equal; another seed changes y; a's zeros beyond ReLU's are ffn_keep_mask's."""
    M, C, Fh, p = 130, 256, 1024, 0.1
    l1, drop, l2 = _layers(C, Fh, p)
    x, go = _data(M, C, xdtype)
    fn = lambda t: fused_ffn(t, l1, F.relu, drop, l2)
    runs = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        out, grad_fn, a = _run(fn, x, go, l1, l2, saved_a=True)
        runs.append((out, a, grad_fn.seed.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert not torch.equal(runs[0][2], runs[2][2]) and not torch.equal(runs[0][0][0], runs[2][0][0])
    for _, a, seed in (runs[0], runs[2]):
        keep = ffn_keep_mask(seed, M, Fh, p)
        with _amp():
            h = F.linear(x, l1.weight, l1.bias)
        relu_pos = h > 0                                                    # (h itself may differ by an ulp from the kernel's)
        sure = (h.float().abs() > 1e-2)
        assert torch.equal((a > 0)[sure], (relu_pos & keep)[sure])
        dropped = int((~keep).sum())
        assert abs(dropped - M * Fh * p) <= 6 * math.sqrt(M * Fh * p * (1 - p))
        assert bool((a[~keep] == 0).all())


def test_graph_capture_replays_the_eager_bits(knob):
    """A training step captured in a HIP graph replays to the eager bits for the same seed (the generator's state registered
    with the graph advances as in eager mode), and makes no host sync."""
    M, C, Fh = 130, 256, 1024
    l1, drop, l2 = _layers(C, Fh, 0.1)
    x, go = _data(M, C, torch.float32)
    static_x = x.clone().requires_grad_(True)

    def step():
        for p in _params(l1, l2):
            p.grad = None
        static_x.grad = None
        with _amp():
            y = fused_ffn(static_x, l1, F.relu, drop, l2)
        y.backward(go)
        return y, y.grad_fn.seed

    torch.manual_seed(21)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                              # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()                                                              # no host sync in a whole eager step
    finally:
        torch.cuda.set_sync_debug_mode(0)
    gc.collect()                                                            # no eager autograd graph alive at the capture's end
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, seed = step()
        grads = [static_x.grad] + [p.grad for p in _params(l1, l2)]
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in [y] + grads]
    keep = ffn_keep_mask(seed.clone(), M, Fh, 0.1)
    want, _ = _run(lambda t: fused_ffn_bf16_reference(t, *_params(l1, l2), 0.1, keep), x, go, l1, l2)
    # the eager node with the same seed contents: the reference restates its mask, and the node's own kernels the bits
    xb, a, y2 = _native.ffn_forward_bf16(x, *_params(l1, l2), 0.1, seed)
    assert torch.equal(got[0], y2)
    eager = _native.ffn_backward_bf16(go, xb, a, l1.weight, l2.weight, 0.1, torch.float32, True, True, True, True, True)
    for name, g, e in zip(NAMES[1:], got[1:], eager):
        assert torch.equal(g, e), name
    _check_against_fp64(got, want, _fp64(x, go, l1, l2, 0.1, keep), "graph replay")


def _stack_layers():
    from conftest import load_golden
    from uvhand_amd.modules import DeformableTransformerDecoderLayer, DeformableTransformerEncoderLayer
    z = load_golden("stack_2d")
    enc = DeformableTransformerEncoderLayer(64, 128, 0.0, "relu", 4, 2, 4)
    dec = DeformableTransformerDecoderLayer(64, 128, 0.0, "relu", 4, 2, 4)
    for mod, prefix in ((enc, "enc_state.layers.0."), (dec, "dec_state.layers.0.")):
        state = {k[len(prefix):]: torch.from_numpy(v) for k, v in z.items() if k.startswith(prefix)}
        mod.load_state_dict(state, strict=True)
    return z, enc.to(DEV).eval(), dec.to(DEV).eval()


def test_encoder_and_decoder_layer_knob_on_against_knob_off(monkeypatch):
    """One encoder layer and one decoder layer at the fixture shapes of tests/test_stack_gpu.py under autocast in eval mode:
    knob on against knob off within that file's amp tolerances (3e-2 of max for activations, 8e-2 for input gradients)."""
    import numpy as np
    from conftest import rel_err
    from uvhand_amd.modules.deformable_layers import decoder_reference_points, encoder_reference_points
    z, enc, dec = _stack_layers()
    cu = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).to(DEV)
    shapes, lsi, valid, mask = cu("shapes"), cu("level_start"), cu("valid"), cu("mask")
    out, calls, forward = {}, [], _native.ffn_forward_bf16
    monkeypatch.setattr(_native, "ffn_forward_bf16", lambda *a: (calls.append(a[0].shape), forward(*a))[1])
    for on in ("0", "1"):
        monkeypatch.setenv("MSDA_FFN_BF16", on)
        src, pos, tgt, qpos = (cu(k).requires_grad_(True) for k in ("src", "pos", "tgt", "qpos"))
        before = len(calls)
        with _amp():
            memory = enc(src, pos, encoder_reference_points(shapes, valid, src.device), shapes, lsi, mask)
            hs = dec(tgt, qpos, decoder_reference_points(cu("refp"), valid), memory, shapes, lsi, mask)
        (hs.float() * cu("g_hs")[0]).sum().backward()
        torch.cuda.synchronize()
        out[on] = ([memory.detach().float(), hs.detach().float()], [src.grad, tgt.grad, pos.grad, qpos.grad],
                   len(calls) - before)
    assert out["0"][2] == 0 and out["1"][2] == 2                           # the node ran in both layers, and only with the knob
    for a, b in zip(out["1"][0], out["0"][0]):
        assert a.dtype == b.dtype and rel_err(a.cpu().numpy(), b.cpu().numpy()) < 3e-2
    for a, b in zip(out["1"][1], out["0"][1]):
        assert a.dtype == b.dtype and rel_err(a.cpu().numpy(), b.cpu().numpy()) < 8e-2
