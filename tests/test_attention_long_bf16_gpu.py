"""The bf16 form of the masked, long-sequence attention core (msda_attn32x_*_bf16, include/msda.h) against
the fp64 restatement of tests/test_attention_long_gpu.py on the (bf16-rounded, upcast) inputs, the numpy keep mask from the same
seed; and the wrapper, the decoder layer and a graph capture on top of it under torch.autocast(bfloat16) with
MSDA_ATTN_LONG_BF16=1.

Tolerance (the project's rule for bf16 nodes: README, prediction heads and FFN): per tensor the kernel's largest error against
fp64 may be at most 4 times the largest error of a torch restatement of the SAME rounding points (`attn32x_bf16_reference`
below: fp32 on the GPU, explicit backward formulas; P_drop rounded to bf16 before P . V, out rounded once, delta from the rounded
out, dS rounded before dQ and dK, the gradients rounded once); that yardstick counts as at least one bf16 ulp of the tensor's
largest fp64 value.  lse is an fp32 output and takes test_attention_long_gpu._rule against the fp32 formula.  Where the fp64 dq /
dk is identically zero (Lk = 1) the floor is one bf16 ulp of the sum's condition value (test_attention_long_gpu's docstring).
The wrapper and the layer take the same 4x rule with the stock autocast module's own error as the yardstick.

Measured on an MI355X (ratio = kernel error / yardstick, worst over all the cases below): see README, "bf16 autocast: the
masked, long core"."""
import copy
import gc
import math

import numpy as np
import pytest
import torch
from torch import nn

from test_attention_gpu import _keep_mask
from test_attention_long_gpu import SCALE, _formula, _hidden_chunk_mask, _mask, _random_mask, _rule, _seed_tensor

pytestmark = pytest.mark.gpu

B, C = 128, 128                  # the bf16 kernels' query (key) block per workgroup and key (query) chunk (csrc/msda_attn_long.hip)
BF16 = torch.bfloat16


def _ulp16(x):
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


RATIOS = {}


def _rule16(what, name, ours, yard_t, r64, zero_floor=0.0):
    """e(ours) <= 4 * max(e(yardstick tensor), one bf16 ulp of the largest fp64 value); keeps the worst ratio per tensor"""
    e_ours = float((ours.double() - r64).abs().max())
    e_yard = float((yard_t.double() - r64).abs().max())
    top = float(r64.abs().max())
    yard = max(e_yard, _ulp16(top) if top > 0 else _ulp16(zero_floor))
    ratio = e_ours / yard if yard else (float("inf") if e_ours else 0.0)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("%s %-12s ours %.3e yardstick tensor %.3e yardstick %.3e ratio %.2f worst so far %.2f"
          % (what, name, e_ours, e_yard, yard, ratio, RATIOS[name]))
    assert e_ours <= 4.0 * yard, (what, name, e_ours, e_yard, yard)
    return ratio


def attn32x_bf16_reference(q, k, v, go, heads, keep, p, mask):
    """The kernels' rounding points restated in torch, fp32 on the GPU, backward by its formulas (no autograd)."""
    Lq, N, E = q.shape
    Lk, hd = k.shape[0], E // heads
    rb = lambda t: t.to(BF16).float()
    split = lambda t, L: t.float().reshape(L, N * heads, hd).transpose(0, 1)
    join = lambda t, L: t.transpose(0, 1).reshape(L, N, E)
    Q, K, V, G = split(q, Lq), split(k, Lk), split(v, Lk), split(go, Lq)
    ks = 1.0 / (1.0 - float(np.float32(p)))
    s = torch.bmm(Q, K.transpose(1, 2)) * SCALE
    if mask is not None:
        s = s.masked_fill(mask[None], float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    total = e.sum(-1, keepdim=True)
    kf = keep.float() if p > 0 else torch.ones_like(e)
    out = rb(torch.bmm(rb(e * kf), V) * (ks / total))                       # un-normalised operand; normalised once; rounded once
    lse = (m + torch.log(total)).squeeze(-1)
    P = e / total
    delta = (G * out).sum(-1, keepdim=True)                                 # from the rounded out
    dP = torch.bmm(G, V.transpose(1, 2))
    dV = rb(torch.bmm(rb(P * kf * ks).transpose(1, 2), G))
    dS = rb(P * (dP * kf * ks - delta))
    dQ = rb(torch.bmm(dS, K) * SCALE)
    dK = rb(torch.bmm(dS.transpose(1, 2), Q) * SCALE)
    return {"out": join(out, Lq), "dq": join(dQ, Lq), "dk": join(dK, Lk), "dv": join(dV, Lk), "lse": lse}


def _inputs(Lq, Lk, N, heads, g):
    """bf16 q and k as column blocks of one packed tensor (what the wrapper passes), v and grad_out dense"""
    E = heads * 32
    qk = torch.randn(max(Lq, Lk), N, 2 * E, generator=g).to(BF16).cuda()
    return (qk[:Lq, :, :E], qk[:Lk, :, E:], torch.randn(Lk, N, E, generator=g).to(BF16).cuda(),
            torch.randn(Lq, N, E, generator=g).to(BF16).cuda())


def _run_core(q, k, v, go, heads, p, seed, mask, packed=True):
    from uvhand_amd import _native
    E = heads * 32
    out, lse = _native.attn32x_forward(q, k, v, heads, SCALE, p, seed if p > 0 else None, mask)
    if packed and q.shape[0] == k.shape[0]:              # gradients into the column blocks of one packed tensor
        g_qk = torch.full((q.shape[0], q.shape[1], 2 * E), float("nan"), device="cuda", dtype=q.dtype)
        gq, gk, gv = _native.attn32x_backward(q, k, v, out, lse, go, heads, SCALE, p, seed if p > 0 else None, mask,
                                              grad_q=g_qk[..., :E], grad_k=g_qk[..., E:])
    else:
        gq, gk, gv = _native.attn32x_backward(q, k, v, out, lse, go, heads, SCALE, p, seed if p > 0 else None, mask)
    return {"out": out, "dq": gq, "dk": gk, "dv": gv, "lse": lse}


def _check_core(what, Lq, Lk, N, heads, p, kind):
    from uvhand_amd import _native
    _native.load()
    g = torch.Generator().manual_seed(Lq * 7 + Lk + N + len(kind))
    q, k, v, go = _inputs(Lq, Lk, N, heads, g)
    mask = _mask(kind, Lq, Lk, g)
    seed_value = 0x1234567890ABCDEF ^ (Lq << 20) ^ Lk
    ours = _run_core(q, k, v, go, heads, p, _seed_tensor(seed_value), mask)
    for name in ("out", "dq", "dk", "dv"):
        assert ours[name].dtype == BF16
    assert ours["lse"].dtype == torch.float32
    keep = torch.from_numpy(_keep_mask(seed_value, N * heads, Lq, Lk, p)).cuda() if p > 0 else None
    r64 = _formula(q, k, v, go, heads, keep, p, mask, torch.float64)
    t32 = _formula(q, k, v, go, heads, keep, p, mask, torch.float32)
    rest = attn32x_bf16_reference(q, k, v, go, heads, keep, p, mask)
    for name in ("out", "dq", "dk", "dv"):
        _rule16(what, name, ours[name], rest[name], r64[name], r64.get(name + "_cond", 0.0))
    _rule(what, "lse", ours["lse"].view(N * heads, Lq), t32["lse"], r64["lse"])
    assert all(torch.isfinite(ours[n]).all() for n in ours)


GRID = [(Lq, Lk) for Lq in (1, B - 1, B, B + 1, 2 * B + 3) for Lk in (1, 17, 31, 32, 33, C - 1, C, C + 1, 2 * C + 5)]
# the query chunk of dK / dV and its key block at their own edges, the exact 32 x 32 denoising mask, the first size the resident
# core refuses
EXTRA = [(C - 1, B - 1), (C + 1, B + 1), (2 * C + 5, 2 * B + 3), (32, 32), (321, 321)]


@pytest.mark.parametrize("kind", ["none", "random", "cdn"])
@pytest.mark.parametrize("Lq,Lk", GRID + EXTRA)
def test_core_matches_fp64(Lq, Lk, kind):
    for p in (0.0, 0.1):
        _check_core("%dx%d %s p=%g" % (Lq, Lk, kind, p), Lq, Lk, 2, 2, p, kind)


@pytest.mark.parametrize("kind", ["none", "random", "cdn"])
def test_core_matches_fp64_at_2048(kind):
    for p in (0.0, 0.1):
        _check_core("2048x2048 %s p=%g" % (kind, p), 2048, 2048, 1, 1, p, kind)


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-1)).item()


@pytest.mark.parametrize("Lq,Lk,N,heads,p,masked", [(320, 3, 2, 4, 0.5, False), (64, 2, 1, 8, 0.5, False), (100, 5, 2, 2, 0.3, False),
                                                    (400, 400, 2, 2, 0.5, True), (400, 400, 2, 2, 0.3, True)])
def test_bf16_long_core_drops_what_the_fp32_long_core_drops(Lq, Lk, N, heads, p, masked):
    """The same seed tensor through the fp32 long core on the upcast inputs and through the bf16 long core: the same keep mask,
    so the two agree to the bf16 tolerance (one different bit in the few-key cases would move the output by O(max))."""
    from uvhand_amd.utils import cdn_attention_mask
    g = torch.Generator().manual_seed(Lq + Lk)
    q, k, v, go = _inputs(Lq, Lk, N, heads, g)
    mask = cdn_attention_mask(3, 5, Lq - 30, "cuda") if masked else None
    seed = _seed_tensor(0x0DDC0FFEE0DDF00D + Lq)
    b16 = _run_core(q, k, v, go, heads, p, seed, mask)
    f32 = _run_core(q.float(), k.float(), v.float(), go.float(), heads, p, seed, mask)
    assert _rel(b16["out"], f32["out"]) < 1e-2
    for name in ("dq", "dk", "dv"):
        assert _rel(b16[name], f32[name]) < 2e-2, name


def test_bf16_long_core_drops_what_the_resident_bf16_core_drops():
    from uvhand_amd import _native
    L, N, heads, p = 300, 2, 8, 0.1
    g = torch.Generator().manual_seed(300)
    q, k, v, go = _inputs(L, L, N, heads, g)
    seed = _seed_tensor(0x0DDC0FFEE0DDF00D + L)
    a = _run_core(q, k, v, go, heads, p, seed, None)
    out, lse = _native.attn32_forward(q, k, v, heads, SCALE, p, seed)
    gq, gk, gv = _native.attn32_backward(q, k, v, out, lse, go, heads, SCALE, p, seed)
    assert _rel(a["out"], out) < 1e-2
    for name, t in (("dq", gq), ("dk", gk), ("dv", gv)):
        assert _rel(a[name], t) < 2e-2, name


def _hidden_chunk_mask_128(L):
    """_hidden_chunk_mask for this form's 128-row chunks: the first query block cannot see the second key chunk [128, L), queries
    [128, L) cannot see the whole FIRST chunk; key 150 is hidden from every query."""
    m = torch.zeros(L, L, dtype=torch.bool)
    m[:B, C:] = True
    m[B:, :C] = True
    m[:, 150] = True
    return m.cuda()


@pytest.mark.parametrize("make_mask", [_hidden_chunk_mask, _hidden_chunk_mask_128])
def test_hidden_chunks_reproducible_and_hidden_keys_get_exact_zeros(make_mask):
    L, N, heads = 200, 2, 2
    g = torch.Generator().manual_seed(77)
    q, k, v, go = _inputs(L, L, N, heads, g)
    mask = make_mask(L)
    for p in (0.0, 0.1):
        seed_value = 0xABCDEF0123456789
        seed = _seed_tensor(seed_value)
        a = _run_core(q, k, v, go, heads, p, seed, mask)
        b = _run_core(q, k, v, go, heads, p, seed, mask, packed=False)
        c = _run_core(q, k, v, go, heads, p, seed, mask)
        for name in a:                                   # two runs, and packed / unpacked gradient targets: bit for bit
            assert torch.equal(a[name], b[name]) and torch.equal(a[name], c[name]), name
        keep = torch.from_numpy(_keep_mask(seed_value, N * heads, L, L, p)).cuda() if p > 0 else None
        r64 = _formula(q, k, v, go, heads, keep, p, mask, torch.float64)
        rest = attn32x_bf16_reference(q, k, v, go, heads, keep, p, mask)
        for name in ("out", "dq", "dk", "dv"):
            _rule16("hidden chunks p=%g" % p, name, a[name], rest[name], r64[name])
        # key 150 is visible to no query: exactly nothing arrives
        assert (a["dk"][150] == 0).all() and (a["dv"][150] == 0).all()
        assert a["dk"][149].float().abs().max() > 0 and a["dv"][151].float().abs().max() > 0


def test_fully_hidden_query_row_is_nan_and_alone():
    from uvhand_amd import _native
    L, N, heads = 200, 2, 2
    g = torch.Generator().manual_seed(78)
    q, k, v, go = _inputs(L, L, N, heads, g)
    base = _random_mask(L, L, g)
    hidden = base.clone()
    hidden[137] = True
    seed = _seed_tensor(99)
    for p in (0.0, 0.1):
        out0, lse0 = _native.attn32x_forward(q, k, v, heads, SCALE, p, seed if p > 0 else None, base)
        out1, lse1 = _native.attn32x_forward(q, k, v, heads, SCALE, p, seed if p > 0 else None, hidden)
        assert out1.dtype == BF16 and torch.isnan(out1[137]).all() and (lse1[:, 137] == float("-inf")).all()
        rows = torch.arange(L, device="cuda") != 137
        assert torch.equal(out1[rows], out0[rows]) and torch.isfinite(out0).all()
        assert torch.equal(lse1[:, rows], lse0[:, rows])


def test_mixed_dtypes_raise_before_any_launch():
    from uvhand_amd import _native
    q = torch.randn(40, 1, 32, device="cuda").to(BF16)
    n0 = _native.launch_count()
    with pytest.raises(RuntimeError, match="bfloat16"):
        _native.attn32x_forward(q, q, q.float(), 1, 1.0)
    with pytest.raises(RuntimeError, match="float32"):
        _native.attn32x_forward(q.float(), q, q, 1, 1.0)
    out, lse = _native.attn32x_forward(q, q, q, 1, 1.0)
    n1 = _native.launch_count()
    with pytest.raises(RuntimeError, match="bfloat16"):
        _native.attn32x_backward(q, q, q, out, lse, q.float(), 1, 1.0)
    with pytest.raises(RuntimeError, match="bfloat16"):
        _native.attn32x_backward(q, q, q, out, lse, q, 1, 1.0, grad_v=torch.empty(40, 1, 32, device="cuda"))
    assert n1 == n0 + 1 and _native.launch_count() == n1


def test_masked_bf16_node_captures_in_a_graph():
    from uvhand_amd.functions.attention_func import _AttnFn
    from uvhand_amd.utils import cdn_attention_mask
    L, N, heads = 200, 2, 2
    E = heads * 32
    g = torch.Generator().manual_seed(9)
    qk = torch.randn(L, N, 2 * E, generator=g).to(BF16).cuda().requires_grad_(True)
    v = torch.randn(L, N, E, generator=g).to(BF16).cuda().requires_grad_(True)
    go = torch.randn(L, N, E, generator=g).to(BF16).cuda()
    m = cdn_attention_mask(3, 4, L - 24, "cuda")

    def step():
        out = _AttnFn.apply("attn32x", qk, v, m, heads, 0.0)
        return (out,) + torch.autograd.grad(out, (qk, v), go)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [t.clone() for t in step()]                                 # warm-up off the capture; the eager bits
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert all(t.dtype == BF16 for t in eager)
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()                                                              # no host sync in a whole eager step
    finally:
        torch.cuda.set_sync_debug_mode(0)
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)


# ---- the wrapper ------------------------------------------------------------------------------------------------------------

NAMES = ("attn32x_forward", "attn32x_backward", "attn32_forward", "attn32_backward")


def _core_launches(monkeypatch):
    """Launches (msda_launch_count) made inside the core's calls, per entry and operand type of q"""
    from uvhand_amd import _native
    seen = {}
    for name in NAMES:
        orig = getattr(_native, name)

        def wrapped(q, *a, _o=orig, _n=name, **kw):
            n0 = _native.launch_count()
            res = _o(q, *a, **kw)
            key = (_n, q.dtype)
            seen[key] = seen.get(key, 0) + _native.launch_count() - n0
            return res
        monkeypatch.setattr(_native, name, wrapped)
    return seen


def _knobs(monkeypatch, long_bf16=None, long_=None):
    for name, value in (("MSDA_ATTN_LONG_BF16", long_bf16), ("MSDA_ATTN_LONG", long_)):
        monkeypatch.delenv(name, raising=False)
        if value is not None:
            monkeypatch.setenv(name, value)


def test_routing_under_autocast(monkeypatch):
    from uvhand_amd import _native
    from uvhand_amd.functions.attention_func import self_attention
    _knobs(monkeypatch)
    seen = _core_launches(monkeypatch)
    torch.manual_seed(4)
    mha = nn.MultiheadAttention(256, 8, dropout=0.1).cuda().eval()
    m = torch.rand(400, 400, device="cuda") < 0.5
    m.fill_diagonal_(False)

    def run(x, mask=None, dtype=BF16, module=mha, backward=False):
        x = x.clone().requires_grad_(backward)
        with torch.autocast("cuda", dtype=dtype):
            ours = self_attention(module, x, x, attn_mask=mask)
            if backward:
                ours.float().sum().backward()
            stock = module(x, x, x, attn_mask=mask, need_weights=False)[0]
        return ours.detach(), stock.detach()
    x = torch.randn(400, 2, 256, device="cuda")
    long16 = {("attn32x_forward", BF16): 1, ("attn32x_backward", BF16): 2}
    # masked, knob on: the long core with bf16 operands, 1 forward and 2 backward launches; the module's output type
    _knobs(monkeypatch, "1")
    ours, stock = run(x, m, backward=True)
    assert seen == long16 and ours.dtype == stock.dtype == BF16
    assert torch.allclose(ours.float(), stock.float(), atol=3e-2)
    # the same call with the knob unset (or "0"): no library launch in the core, the module's bits
    for value in (None, "0", ""):
        _knobs(monkeypatch, value)
        seen.clear()
        n0 = _native.launch_count()
        ours, stock = run(x, m)
        assert not seen and _native.launch_count() == n0 and torch.equal(ours, stock)
    # unmasked L = 400 needs both knobs
    for a, b in (("1", None), (None, "1")):
        _knobs(monkeypatch, a, b)
        ours, stock = run(x)
        assert not seen and torch.equal(ours, stock)
    _knobs(monkeypatch, "1", "1")
    run(x, backward=True)
    assert seen == long16
    # unmasked L = 300: the resident bf16 core either way
    y = torch.randn(300, 2, 256, device="cuda")
    for a, b in ((None, None), ("1", "1")):
        _knobs(monkeypatch, a, b)
        seen.clear()
        run(y, backward=True)
        assert seen == {("attn32_forward", BF16): 1, ("attn32_backward", BF16): 2}
    # fp16 autocast, a float mask, a 3-D mask, head_dim 64: the module, knobs on
    _knobs(monkeypatch, "1", "1")
    seen.clear()
    ours, stock = run(x, m, dtype=torch.float16)
    assert torch.equal(ours, stock)
    fm = torch.zeros(400, 400, device="cuda").masked_fill(m, float("-inf"))
    ours, stock = run(x, fm)
    assert torch.equal(ours, stock)
    ours, stock = run(x, m[None].expand(16, 400, 400))
    assert torch.equal(ours, stock)
    wide = nn.MultiheadAttention(256, 4).cuda().eval()
    ours, stock = run(x, m, module=wide)
    assert torch.equal(ours, stock)
    assert not seen


def _module_grads(mha, fn, x_qk, x_v, go, autocast):
    a, b = x_qk.clone().requires_grad_(True), x_v.clone().requires_grad_(True)
    mha.zero_grad()
    with torch.autocast("cuda", dtype=BF16, enabled=autocast):
        out = fn(a, b)
    out.backward(go.to(out.dtype))
    return [out.detach(), a.grad, b.grad] + [p.grad.clone() for p in mha.parameters()]


@pytest.mark.parametrize("L", [50, 400])
def test_wrapper_against_the_module_under_the_denoising_mask(monkeypatch, L):
    from uvhand_amd.functions.attention_func import self_attention
    from uvhand_amd.utils import cdn_attention_mask
    _knobs(monkeypatch, "1")
    seen = _core_launches(monkeypatch)
    N = 2
    torch.manual_seed(3)
    mha = nn.MultiheadAttention(256, 8, dropout=0.1).cuda().eval()
    m = cdn_attention_mask(3, 2, L - 12, "cuda")
    assert tuple(m.shape) == (L, L)
    x_qk, x_v, go = (torch.randn(L, N, 256, device="cuda") for _ in range(3))
    ours = _module_grads(mha, lambda a, b: self_attention(mha, a, b, attn_mask=m), x_qk, x_v, go, True)
    assert seen == {("attn32x_forward", BF16): 1, ("attn32x_backward", BF16): 2}
    stock = _module_grads(mha, lambda a, b: mha(a, a, b, attn_mask=m, need_weights=False)[0], x_qk, x_v, go, True)
    mha64 = copy.deepcopy(mha).double()
    ref = _module_grads(mha64, lambda a, b: mha64(a, a, b, attn_mask=m, need_weights=False)[0], x_qk.double(), x_v.double(),
                        go.to(BF16).double(), False)
    names = ["out", "grad_x_qk", "grad_x_v"] + ["grad_" + n for n, _ in mha.named_parameters()]
    for name, a, b, r in zip(names, ours, stock, ref):
        assert a.dtype == b.dtype, name
        _rule16("wrapper L=%d" % L, "w:" + name, a, b, r)


def test_training_draws_from_torchs_generator(monkeypatch):
    from uvhand_amd.functions.attention_func import self_attention
    from uvhand_amd.utils import cdn_attention_mask
    _knobs(monkeypatch, "1")
    seen = _core_launches(monkeypatch)
    torch.manual_seed(5)
    mha = nn.MultiheadAttention(256, 8, dropout=0.1).cuda().train()
    m = cdn_attention_mask(3, 5, 370, "cuda")
    x = torch.randn(400, 2, 256, device="cuda", requires_grad=True)

    def run(seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        with torch.autocast("cuda", dtype=BF16):
            return self_attention(mha, x, x, attn_mask=m)
    a, b, c = run(11), run(11), run()
    assert seen == {("attn32x_forward", BF16): 3}
    assert torch.equal(a, b) and not torch.equal(a, c)
    a.float().sum().backward()
    assert torch.isfinite(x.grad).all() and torch.isfinite(mha.in_proj_weight.grad).all()


def test_decoder_layer_with_a_self_attention_mask_under_autocast(monkeypatch):
    """The layer with self_attn_mask on the bf16 long core against the same layer with self_attn run by the stock module (a
    listener on attn_matrix asks for it), both under autocast, eval mode; reference: an fp64 copy of the layer, the module
    inside, outside autocast."""
    from conftest import load_golden
    from uvhand_amd.modules import DeformableTransformerDecoder, DeformableTransformerDecoderLayer
    from uvhand_amd.utils import cdn_attention_mask
    _knobs(monkeypatch, "1")
    seen = _core_launches(monkeypatch)
    z = load_golden("layer_decoder_2d")
    cu = lambda key, dt=None: (lambda t: t.to(dt) if dt is not None and t.is_floating_point() else t)(
        torch.from_numpy(np.ascontiguousarray(z[key])).cuda())
    layer = DeformableTransformerDecoderLayer(64, 128, 0.0, "relu", 4, 2, 4)
    layer.load_state_dict({k[len("state."):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state.")}, strict=True)
    layer = layer.cuda().eval()
    Q = z["tgt"].shape[1]
    m = cdn_attention_mask(1, 2, Q - 4, "cuda")
    assert tuple(m.shape) == (Q, Q)

    def run(mod, dt, listen):
        handle = mod.attn_matrix.register_forward_hook(lambda *a: None) if listen else None
        tgt = cu("tgt", dt).requires_grad_(True)
        with torch.autocast("cuda", dtype=BF16, enabled=dt == torch.float32):
            out = mod(tgt, cu("qpos", dt), cu("ref", dt), cu("memory", dt), cu("shapes"), cu("level_start"), cu("mask"),
                      self_attn_mask=m)
        out.backward(cu("gout", dt).to(out.dtype))
        if handle is not None:
            handle.remove()
        return out.detach(), tgt.grad
    ours = run(layer, torch.float32, False)
    assert seen == {("attn32x_forward", BF16): 1, ("attn32x_backward", BF16): 2}
    seen.clear()
    stock = run(layer, torch.float32, True)
    assert not seen
    ref = run(copy.deepcopy(layer).double(), torch.float64, True)
    for name, a, b, r in zip(("out", "grad_tgt"), ours, stock, ref):
        _rule16("decoder layer", "layer:" + name, a, b, r)
    # the decoder hands tgt_mask to every layer
    seen.clear()
    dec = DeformableTransformerDecoder(layer, 2).cuda().eval()
    valid = torch.ones(z["tgt"].shape[0], 4, 2, device="cuda")
    refp = torch.rand(z["tgt"].shape[0], Q, 2, device="cuda")
    with torch.autocast("cuda", dtype=BF16):
        with_mask, _ = dec(cu("tgt"), refp, cu("memory"), cu("shapes"), cu("level_start"), valid, cu("qpos"), cu("mask"), tgt_mask=m)
    assert seen == {("attn32x_forward", BF16): 2} and torch.isfinite(with_mask).all()
