"""The bf16-autocast forms of the decoder self-attention core and of the residual add + LayerNorm (ABI 116):
msda_attn32_*_bf16 against an fp64 restatement with the numpy keep-mask, against the fp32 core on the same (upcast) inputs and
seed, reproducibility and graph capture; the wrapper and the layers under torch.autocast(bfloat16) against stock modules and the
fixtures; msda_add_layernorm_*_f32_bf16res against fp64."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu


def _keep_mask(seed, pairs, Lq, Lk, p):
    """numpy restatement of at_hash / thresh (uvhand_amd/csrc/msda_attn.hip), shared by the fp32 and bf16 cores."""
    if p == 0:
        return np.ones((pairs, Lq, Lk), bool)
    seed &= 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    q = np.arange(Lq, dtype=np.uint32)[None, :, None]
    key = np.arange(Lk, dtype=np.uint32)[None, None, :]
    pair = np.arange(pairs, dtype=np.uint32)[:, None, None]
    with np.errstate(over="ignore"):
        x = (q << np.uint32(16)) + key + (lo + pair * np.uint32(0x9E3779B1) + hi * np.uint32(0x85EBCA6B))
        x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x85EBCA6B)
        x = x ^ (x >> np.uint32(13)); x = x * np.uint32(0xC2B2AE35)
    thresh = np.uint32(min(4294967295.0, float(np.float32(p)) * 4294967296.0))
    return x >= thresh


def _reference(q, k, v, go, heads, scale, keep, p):
    Lq, N, E = q.shape
    Lk, hd = k.shape[0], E // heads
    qd, kd, vd = (t.double().detach().requires_grad_(True) for t in (q, k, v))
    split = lambda t, L: t.reshape(L, N * heads, hd).transpose(0, 1)
    s = torch.bmm(split(qd, Lq), split(kd, Lk).transpose(1, 2)) * scale
    pr = torch.softmax(s, -1) * torch.from_numpy(keep).to(s) / (1.0 - float(np.float32(p)))
    out = torch.bmm(pr, split(vd, Lk)).transpose(0, 1).reshape(Lq, N, E)
    out.backward(go.double())
    return out.detach(), qd.grad, kd.grad, vd.grad


# test_attention_gpu.CASES, then few-key cases: every probability is large there, so one wrong mask bit moves the output by O(max)
CASES = [(300, 300, 4, 8, 0.0), (300, 300, 3, 8, 0.1), (37, 37, 2, 3, 0.0), (16, 320, 2, 1, 0.25), (320, 17, 1, 4, 0.5),
         (1, 1, 1, 1, 0.0), (129, 200, 2, 8, 0.1)]
FEW_KEYS = [(320, 3, 2, 4, 0.5), (64, 2, 1, 8, 0.5), (100, 5, 2, 2, 0.3)]


def _seed(value):
    return torch.tensor([value - (1 << 64) if value >= (1 << 63) else value], dtype=torch.int64).cuda()


def _inputs(Lq, Lk, N, heads, dtype=torch.bfloat16):
    """bf16 q / k as column blocks of one packed tensor (what the wrapper passes), v and grad_out dense."""
    g = torch.Generator().manual_seed(Lq * 7 + Lk + N)
    E = heads * 32
    qk = torch.randn(max(Lq, Lk), N, 2 * E, generator=g).to(dtype).cuda()
    v = torch.randn(Lk, N, E, generator=g).to(dtype).cuda()
    go = torch.randn(Lq, N, E, generator=g).to(dtype).cuda()
    return qk[:Lq, :, :E], qk[:Lk, :, E:], v, go


def _run(q, k, v, go, heads, p, seed):
    from uvhand_amd import _native
    scale = 1.0 / math.sqrt(32)
    out, lse = _native.attn32_forward(q, k, v, heads, scale, p, seed if p > 0 else None)
    gq, gk, gv = _native.attn32_backward(q, k, v, out, lse, go, heads, scale, p, seed if p > 0 else None)
    return out, lse, gq, gk, gv


def _rel(a, b):
    return ((a.cpu().double() - b.cpu().double()).abs().max() / (b.cpu().double().abs().max() + 1e-1)).item()


@pytest.mark.parametrize("Lq,Lk,N,heads,p", CASES + FEW_KEYS)
def test_bf16_core_matches_fp64(Lq, Lk, N, heads, p):
    """bf16-rounded inputs, fp64 arithmetic and the numpy mask for the same seed.  Tolerances: out 1e-2, dq / dk / dv 2e-2 of
    max (P, dS and the results are rounded to bf16: 2^-9 relative each)."""
    from uvhand_amd import _native
    _native.load()
    q, k, v, go = _inputs(Lq, Lk, N, heads)
    seed_value = 0x1234567890ABCDEF ^ (Lq << 20)
    out, lse, gq, gk, gv = _run(q, k, v, go, heads, p, _seed(seed_value))
    torch.cuda.synchronize()
    assert out.dtype == gq.dtype == gk.dtype == gv.dtype == torch.bfloat16 and lse.dtype == torch.float32
    keep = _keep_mask(seed_value, N * heads, Lq, Lk, p)
    r_out, r_gq, r_gk, r_gv = _reference(q.cpu(), k.cpu(), v.cpu(), go.cpu(), heads, 1.0 / math.sqrt(32), keep, p)
    assert _rel(out, r_out) < 1e-2
    assert _rel(gq, r_gq) < 2e-2 and _rel(gk, r_gk) < 2e-2 and _rel(gv, r_gv) < 2e-2
    s = torch.einsum("qbhd,kbhd->bhqk", q.cpu().double().view(Lq, N, heads, 32), k.cpu().double().view(Lk, N, heads, 32)) / math.sqrt(32)
    assert (lse.cpu().double().view(N, heads, Lq) - torch.logsumexp(s, -1)).abs().max().item() < 1e-4


@pytest.mark.parametrize("Lq,Lk,N,heads,p", FEW_KEYS + [(300, 300, 2, 8, 0.1)])
def test_bf16_core_drops_what_the_fp32_core_drops(Lq, Lk, N, heads, p):
    """The same seed tensor through the fp32 core on the upcast inputs and through the bf16 core: the same mask, so the two
    agree to the bf16 tolerance (a single different bit in the few-key cases would move the output by O(max))."""
    from uvhand_amd import _native
    _native.load()
    q, k, v, go = _inputs(Lq, Lk, N, heads)
    seed = _seed(0x0DDC0FFEE0DDF00D + Lq)
    b16 = _run(q, k, v, go, heads, p, seed)
    f32 = _run(q.float(), k.float(), v.float(), go.float(), heads, p, seed)
    assert _rel(b16[0], f32[0]) < 1e-2
    for a, b in zip(b16[2:], f32[2:]):
        assert _rel(a, b) < 2e-2


def test_bf16_core_is_reproducible_and_capturable():
    from uvhand_amd import _native
    _native.load()
    Lq = Lk = 300
    N, heads, p = 4, 8, 0.1
    q, k, v, go = _inputs(Lq, Lk, N, heads)
    seed = _seed(77)
    first = _run(q, k, v, go, heads, p, seed)
    second = _run(q, k, v, go, heads, p, seed)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # one capture of forward + backward, replayed with the same seed contents
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(q, k, v, go, heads, p, seed)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _run(q, k, v, go, heads, p, seed)
    seed.fill_(12345)
    graph.replay()
    torch.cuda.synchronize()
    other = _run(q, k, v, go, heads, p, seed)
    for a, b in zip(captured, other):
        assert torch.equal(a, b)
    seed.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, first):
        assert torch.equal(a, b)


def _count(monkeypatch, module, names):
    calls = {n: 0 for n in names}
    for name in names:
        orig = getattr(module, name)

        def wrapped(*a, _o=orig, _n=name, **kw):
            calls[_n] += 1
            return _o(*a, **kw)
        monkeypatch.setattr(module, name, wrapped)
    return calls


def _bf16_core_counter(monkeypatch):
    """Counts the core calls that take bf16 operands (attn32_forward / attn32_backward dispatch on q's dtype)."""
    from uvhand_amd import _native
    calls = {"fwd": 0, "bwd": 0}
    for name, key in (("attn32_forward", "fwd"), ("attn32_backward", "bwd")):
        orig = getattr(_native, name)

        def wrapped(q, *a, _o=orig, _k=key, **kw):
            if q.dtype == torch.bfloat16:
                calls[_k] += 1
            return _o(q, *a, **kw)
        monkeypatch.setattr(_native, name, wrapped)
    return calls


def _mha_pair(L, N, E=256, heads=8, train=False, dropout=0.1):
    torch.manual_seed(3)
    mha = nn.MultiheadAttention(E, heads, dropout=dropout).cuda().train(train)
    x_qk, x_v = torch.randn(L, N, E, device="cuda"), torch.randn(L, N, E, device="cuda")
    return mha, x_qk, x_v


def _grads(mha, fn, x_qk, x_v, go):
    a, b = x_qk.clone().requires_grad_(True), x_v.clone().requires_grad_(True)
    mha.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = fn(a, b)
    out.backward(go.to(out.dtype))
    return out, [a.grad, b.grad, mha.in_proj_weight.grad.clone(), mha.in_proj_bias.grad.clone(), mha.out_proj.weight.grad.clone(),
                 mha.out_proj.bias.grad.clone()]


@pytest.mark.parametrize("L,N", [(300, 4), (50, 2)])
def test_wrapper_under_autocast_matches_the_module(monkeypatch, L, N):
    from uvhand_amd.functions.attention_func import self_attention
    calls = _bf16_core_counter(monkeypatch)
    mha, x_qk, x_v = _mha_pair(L, N)
    go = torch.randn(L, N, 256, device="cuda")
    ours, g_ours = _grads(mha, lambda a, b: self_attention(mha, a, b), x_qk, x_v, go)
    assert calls == {"fwd": 1, "bwd": 1}
    stock, g_stock = _grads(mha, lambda a, b: mha(a, a, b, need_weights=False)[0], x_qk, x_v, go)
    assert ours.dtype == stock.dtype
    assert rel_err(ours.detach().float().cpu().numpy(), stock.detach().float().cpu().numpy()) < 3e-2
    for x, y in zip(g_ours, g_stock):
        assert rel_err(x.float().cpu().numpy(), y.float().cpu().numpy()) < 3e-2


def test_wrapper_under_autocast_trains_with_dropout(monkeypatch):
    from uvhand_amd.functions.attention_func import self_attention
    calls = _bf16_core_counter(monkeypatch)
    mha, x_qk, x_v = _mha_pair(300, 2, train=True, dropout=0.1)

    def run(seed):
        torch.manual_seed(seed)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return self_attention(mha, x_qk, x_v)
    a, b, c = run(11), run(11), run(12)
    assert calls["fwd"] == 3
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_wrapper_routes_everything_else_to_the_module(monkeypatch):
    """fp16 autocast, head_dim 64, L = 400: the bf16 core is not called and the result is the module's."""
    from uvhand_amd.functions.attention_func import self_attention
    calls = _bf16_core_counter(monkeypatch)
    cases = [(torch.float16, 256, 8, 50), (torch.bfloat16, 256, 4, 50), (torch.bfloat16, 256, 8, 400)]
    for dtype, E, heads, L in cases:
        torch.manual_seed(3)
        mha = nn.MultiheadAttention(E, heads, dropout=0.1).cuda().eval()
        x_qk, x_v = torch.randn(L, 2, E, device="cuda"), torch.randn(L, 2, E, device="cuda")
        with torch.autocast("cuda", dtype=dtype):
            ours = self_attention(mha, x_qk, x_v)
            stock = mha(x_qk, x_qk, x_v, need_weights=False)[0]
        assert ours.dtype == stock.dtype and torch.equal(ours, stock), (dtype, E, heads, L)
    assert calls == {"fwd": 0, "bwd": 0}


def _cuda(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.requires_grad_(True) if grad else t


def _load(layer, z):
    state = {k[len("state."):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state.")}
    missing, unexpected = layer.load_state_dict(state, strict=True)
    assert not missing and not unexpected
    return layer.cuda()


def _ln_counter(monkeypatch):
    from uvhand_amd import _native
    return _count(monkeypatch, _native, ("add_layernorm_forward_bf16res", "add_layernorm_backward_bf16res", "add_layernorm_forward",
                                         "add_layernorm_backward"))


def _ln_kernel_calls(ln, which):
    """(calls of the mixed kernel, calls of either kernel) in direction `which` ("forward" / "backward")."""
    mixed = ln["add_layernorm_%s_bf16res" % which]
    return mixed, mixed + ln["add_layernorm_%s" % which]


@pytest.mark.parametrize("width", [2, 42])
def test_decoder_layer_under_autocast(monkeypatch, width):
    """The fixture's fp32 reference against the layer under autocast(bf16): the bf16 core and the mixed add + LayerNorm run;
    3e-2 of max for the output, 8e-2 for input and parameter gradients (the amp stack test's tolerances).  Except linear1's:
    measured 0.26 of max for linear1.weight at width 42 on an MI355X.  The FFN stays the stock bf16 composition under autocast,
    and with 9 queries x 2 frames a hidden unit whose pre-activation sits near zero can switch its ReLU between the bf16 run
    and the fp32 fixture; that changes the unit's whole gradient row by one query's term.  Those two are checked to be
    finite only; everything downstream of them is checked at 8e-2."""
    from uvhand_amd.modules import DeformableTransformerDecoderLayer
    core = _bf16_core_counter(monkeypatch)
    ln = _ln_counter(monkeypatch)
    z = load_golden("layer_decoder_%dd" % width)
    layer = _load(DeformableTransformerDecoderLayer(64, 128, 0.0, "relu", 4, 2, 4), z)
    tgt, qpos, memory = _cuda(z["tgt"], True), _cuda(z["qpos"], True), _cuda(z["memory"], True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(tgt, qpos, _cuda(z["ref"]), memory, _cuda(z["shapes"]), _cuda(z["level_start"]), _cuda(z["mask"]))
    out.backward(_cuda(z["gout"]).to(out.dtype))
    torch.cuda.synchronize()
    assert core == {"fwd": 1, "bwd": 1}
    # all three add + LayerNorms on a kernel; the self-attention's and the FFN's residuals are bf16 projection outputs
    for which in ("forward", "backward"):
        mixed, total = _ln_kernel_calls(ln, which)
        assert total == 3 and mixed >= 2, (which, mixed, total)
    assert out.dtype == torch.float32
    assert rel_err(out.detach().cpu().numpy(), z["out"]) < 3e-2
    for t, key in ((tgt, "grad_tgt"), (qpos, "grad_qpos"), (memory, "grad_memory")):
        assert rel_err(t.grad.float().cpu().numpy(), z[key]) < 8e-2, key
    for name, p in layer.named_parameters():
        if name.startswith("linear1."):
            assert torch.isfinite(p.grad).all(), name
            continue
        assert rel_err(p.grad.float().cpu().numpy(), z["pgrad." + name]) < 8e-2, name


def test_decoder_layer_with_a_listener_keeps_the_module_under_autocast(monkeypatch):
    """A hook on attn_matrix asks for the attention matrix: the module runs, the bf16 core does not, the output is unchanged."""
    from uvhand_amd.modules import DeformableTransformerDecoderLayer
    core = _bf16_core_counter(monkeypatch)
    z = load_golden("layer_decoder_2d")
    layer = _load(DeformableTransformerDecoderLayer(64, 128, 0.0, "relu", 4, 2, 4), z)
    seen = []
    layer.attn_matrix.register_forward_hook(lambda m, i, o: seen.append(o.shape))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(_cuda(z["tgt"]), _cuda(z["qpos"]), _cuda(z["ref"]), _cuda(z["memory"]), _cuda(z["shapes"]),
                    _cuda(z["level_start"]), _cuda(z["mask"]))
    assert seen and core == {"fwd": 0, "bwd": 0}
    assert rel_err(out.detach().float().cpu().numpy(), z["out"]) < 3e-2


def test_encoder_layer_under_autocast(monkeypatch):
    """The encoder layer fixture under autocast(bf16): the mixed add + LayerNorm runs; output 3e-2 of max, the gradient of src
    and of the two LayerNorms' parameters 8e-2.  The gradient of pos is checked to be finite only: measured 0.36 of max on an
    MI355X.  It reaches pos only through MSDeformAttn's sampling offsets and attention weights, which this layer runs as the
    module's bf16 composition under autocast (bf16_storage off); bilinear sampling-location gradients in bf16 are that coarse,
    and no kernel of this change is on that path.  For the same reason the other parameters are checked to be finite only."""
    from uvhand_amd.modules import DeformableTransformerEncoderLayer
    ln = _ln_counter(monkeypatch)
    z = load_golden("layer_encoder")
    layer = _load(DeformableTransformerEncoderLayer(64, 128, 0.0, "relu", 4, 2, 4), z)
    src, pos = _cuda(z["src"], True), _cuda(z["pos"], True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(src, pos, _cuda(z["ref"]), _cuda(z["shapes"]), _cuda(z["level_start"]), _cuda(z["mask"]))
    out.backward(_cuda(z["gout"]).to(out.dtype))
    torch.cuda.synchronize()
    for which in ("forward", "backward"):
        mixed, total = _ln_kernel_calls(ln, which)
        assert total == 2 and mixed >= 1, (which, mixed, total)             # (the FFN's residual is a bf16 GEMM output)
    assert rel_err(out.detach().float().cpu().numpy(), z["out"]) < 3e-2
    assert rel_err(src.grad.float().cpu().numpy(), z["grad_src"]) < 8e-2
    assert torch.isfinite(pos.grad).all()
    for name, p in layer.named_parameters():
        if name.startswith(("norm1.", "norm2.")):
            assert rel_err(p.grad.float().cpu().numpy(), z["pgrad." + name]) < 8e-2, name
        else:
            assert torch.isfinite(p.grad).all(), name


@pytest.mark.parametrize("rows,d", [(1, 256), (7, 64), (600, 256), (33, 512), (129, 1024), (50, 260)])
def test_add_layernorm_bf16_residual_matches_fp64(monkeypatch, rows, d):
    from uvhand_amd.functions.layernorm_func import add_layer_norm
    ln = _ln_counter(monkeypatch)
    g = torch.Generator().manual_seed(rows * 7 + d)
    norm = nn.LayerNorm(d).cuda()
    with torch.no_grad():
        norm.weight.copy_(torch.randn(d, generator=g) * 0.5 + 1.0)
        norm.bias.copy_(torch.randn(d, generator=g) * 0.3)
    x = (torch.randn(rows, d, generator=g) * 2 + 0.7).cuda().requires_grad_(True)
    r = torch.randn(rows, d, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
    gy = torch.randn(rows, d, generator=g).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = add_layer_norm(x, r, norm)
    y.backward(gy)
    assert ln["add_layernorm_forward_bf16res"] == 1 and ln["add_layernorm_backward_bf16res"] == 1
    assert y.dtype == torch.float32 and x.grad.dtype == torch.float32 and r.grad.dtype == torch.bfloat16
    x64 = x.detach().double().requires_grad_(True)
    r64 = r.detach().double().requires_grad_(True)
    w64, b64 = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
    y64 = torch.nn.functional.layer_norm(x64 + r64, (d,), w64, b64, norm.eps)
    y64.backward(gy.double())
    assert rel_err(y.detach().cpu().numpy(), y64.detach().cpu().numpy()) < 1e-5
    assert rel_err(x.grad.cpu().numpy(), x64.grad.cpu().numpy()) < 1e-5
    assert torch.equal(r.grad, x.grad.to(torch.bfloat16))
    assert rel_err(norm.weight.grad.cpu().numpy(), w64.grad.cpu().numpy()) < 1e-5
    assert rel_err(norm.bias.grad.cpu().numpy(), b64.grad.cpu().numpy()) < 1e-5
    # an fp32 residual under the same autocast takes the fp32 kernel: the result of the call outside autocast
    rf = r.detach().float()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y_amp = add_layer_norm(x.detach(), rf, norm)
    assert torch.equal(y_amp, add_layer_norm(x.detach(), rf, norm))
