"""The masked, long-sequence attention core (msda_attn32x_*_f32, include/msda.h) against an fp64 restatement of
dropout(softmax(q k^T * scale + M)) v in torch — the mask added as -inf, the kernel's dropout mask restated in numpy from the
same seed (tests/test_attention_gpu.py:_keep_mask) — over every (query count, key count) the chunking can get wrong, and the
drop-in wrapper, the decoder layer and a graph capture on top of it.

Tolerance (the project's rule for fp32 kernels, tests/test_optim_gpu.py): per tensor the kernel's largest error against fp64 may
be at most 4 times the largest error of the SAME formula evaluated by torch in fp32 on the GPU with the same keep mask; that
yardstick counts as at least one fp32 ulp of the tensor's largest (fp64) value.  One case needs a word: when every query sees a
single key (Lk = 1) the probabilities are the constant 1 and dq, dk are exactly zero — the difference dP - delta of two equal
numbers.  torch's softmax backward forms that difference from one rounded number and returns exact zeros, so the yardstick as
stated is 0 and only an exact zero passes.  The kernel forms dP on the MFMA chain and delta = rowsum(dO * O) as the C ABI
prescribes — two fp32 evaluations of the same sum in different orders — and what is left is the rounding of those terms.  For a
tensor whose fp64 value is identically zero the floor is therefore one fp32 ulp of the sum's CONDITION value — the same formula
with every term replaced by its magnitude, the quantity every a-priori rounding bound of a sum is stated in:
dq: scale * A |k|, dk: scale * A^T |q| with A = P_drop o (|dO| |v|^T) + P o rowsum(|dO| o |O|).  Nothing here comes from the
kernel's own output.

Measured on an MI355X (ratio = kernel error / yardstick, over all the cases below): see README, "Masked, long decoder
self-attention"."""
import copy
import gc
import math

import numpy as np
import pytest
import torch
from torch import nn

from test_attention_gpu import _keep_mask

pytestmark = pytest.mark.gpu

B, C = 128, 64                   # the kernels' query (key) block per workgroup and key (query) chunk (csrc/msda_attn_long.hip)
SCALE = 1.0 / math.sqrt(32)


def _seed_tensor(value):
    return torch.tensor([value - (1 << 64) if value >= (1 << 63) else value], dtype=torch.int64).cuda()


def _formula(q, k, v, go, heads, keep, p, mask, dtype):
    """dropout(softmax(q k^T * scale + M)) v, its gradients and lse in `dtype` on the tensors' device"""
    Lq, N, E = q.shape
    Lk, hd = k.shape[0], E // heads
    qd, kd, vd = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    split = lambda t, L: t.reshape(L, N * heads, hd).transpose(0, 1)
    s = torch.bmm(split(qd, Lq), split(kd, Lk).transpose(1, 2)) * SCALE
    if mask is not None:
        s = s.masked_fill(mask[None], float("-inf"))
    pr = torch.softmax(s, -1)
    if p > 0:
        pr = pr * keep.to(dtype) / (1.0 - float(np.float32(p)))
    out = torch.bmm(pr, split(vd, Lk)).transpose(0, 1).reshape(Lq, N, E)
    out.backward(go.to(dtype))
    res = {"out": out.detach(), "dq": qd.grad, "dk": kd.grad, "dv": vd.grad, "lse": torch.logsumexp(s.detach(), -1)}
    if dtype == torch.float64 and (float(qd.grad.abs().max()) == 0 or float(kd.grad.abs().max()) == 0):
        with torch.no_grad():                            # the condition values of dq and dk (module docstring)
            g, o = split(go.to(dtype), Lq).abs(), split(out.detach(), Lq).abs()
            a = pr * torch.bmm(g, split(vd, Lk).abs().transpose(1, 2)) + torch.softmax(s, -1) * (g * o).sum(-1, keepdim=True)
            res["dq_cond"] = float((torch.bmm(a, split(kd, Lk).abs()) * SCALE).max())
            res["dk_cond"] = float((torch.bmm(a.transpose(1, 2), split(qd, Lq).abs()) * SCALE).max())
    return res


def _ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 0.0


RATIOS = {}


def _rule(what, name, ours, t32, r64, zero_floor=0.0):
    """e(ours) <= 4 * max(e(torch fp32), one fp32 ulp of the largest value); returns the ratio (and keeps the worst per tensor)."""
    e_ours = float((ours.double() - r64).abs().max())
    e_torch = float((t32.double() - r64).abs().max())
    top = float(r64.abs().max())
    yard = max(e_torch, _ulp(top) if top > 0 else _ulp(zero_floor))
    ratio = e_ours / yard if yard else (float("inf") if e_ours else 0.0)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("%s %-3s ours %.3e torch %.3e yardstick %.3e ratio %.2f" % (what, name, e_ours, e_torch, yard, ratio))
    assert e_ours <= 4.0 * yard, (what, name, e_ours, e_torch, yard)
    return ratio


def _tiled_cdn(Lq, Lk):
    """cdn_attention_mask(3, 2, 20) — 32 x 32 — repeated with period 32 over [Lq, Lk] and cropped (the 32 x 32 case: the mask as it
    is); a row the crop leaves without a visible key (Lk <= 12) gets key 0 back."""
    from uvhand_amd.utils import cdn_attention_mask
    m = cdn_attention_mask(3, 2, 20, "cuda")
    m = m.repeat((Lq + 31) // 32, (Lk + 31) // 32)[:Lq, :Lk].contiguous()
    m[:, 0] &= ~m.all(1)
    return m


def _random_mask(Lq, Lk, g):
    m = torch.rand(Lq, Lk, generator=g) < 0.6
    m[torch.arange(Lq), torch.randint(0, Lk, (Lq,), generator=g)] = False      # at least one visible key per row
    return m.cuda()


def _mask(kind, Lq, Lk, g):
    return None if kind == "none" else _random_mask(Lq, Lk, g) if kind == "random" else _tiled_cdn(Lq, Lk)


def _inputs(Lq, Lk, N, heads, g):
    """q and k as column blocks of one packed tensor (what the wrapper passes), v and grad_out dense"""
    E = heads * 32
    qk = torch.randn(max(Lq, Lk), N, 2 * E, generator=g).cuda()
    return qk[:Lq, :, :E], qk[:Lk, :, E:], torch.randn(Lk, N, E, generator=g).cuda(), torch.randn(Lq, N, E, generator=g).cuda()


def _run_core(q, k, v, go, heads, p, seed, mask, packed=True):
    from uvhand_amd import _native
    E = heads * 32
    out, lse = _native.attn32x_forward(q, k, v, heads, SCALE, p, seed if p > 0 else None, mask)
    if packed and q.shape[0] == k.shape[0]:              # gradients into the column blocks of one packed tensor
        g_qk = torch.full((q.shape[0], q.shape[1], 2 * E), float("nan"), device="cuda")
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
    keep = torch.from_numpy(_keep_mask(seed_value, N * heads, Lq, Lk, p)).cuda() if p > 0 else None
    r64 = _formula(q, k, v, go, heads, keep, p, mask, torch.float64)
    t32 = _formula(q, k, v, go, heads, keep, p, mask, torch.float32)
    for name in ("out", "dq", "dk", "dv"):
        _rule(what, name, ours[name], t32[name], r64[name], r64.get(name + "_cond", 0.0))
    _rule(what, "lse", ours["lse"].view(N * heads, Lq), t32["lse"], r64["lse"])
    assert all(torch.isfinite(ours[n]).all() for n in ours)


GRID = [(Lq, Lk) for Lq in (1, B - 1, B, B + 1, 2 * B + 3) for Lk in (1, 17, C - 1, C, C + 1, 2 * C + 5)]
# the query chunk of dK / dV (64) and its key block (128) at their own edges, the exact 32 x 32 denoising mask, the first size
# the resident core refuses
EXTRA = [(C - 1, B - 1), (C + 1, B + 1), (2 * C + 5, 2 * B + 3), (32, 32), (321, 321)]


@pytest.mark.parametrize("kind", ["none", "random", "cdn"])
@pytest.mark.parametrize("Lq,Lk", GRID + EXTRA)
def test_core_matches_fp64(Lq, Lk, kind):
    N, heads = (1, 8) if Lq == 321 else (2, 2)
    for p in (0.0, 0.1):
        _check_core("%dx%d %s p=%g" % (Lq, Lk, kind, p), Lq, Lk, N, heads, p, kind)


@pytest.mark.parametrize("kind", ["none", "random", "cdn"])
def test_core_matches_fp64_at_2048(kind):
    for p in (0.0, 0.1):
        _check_core("2048x2048 %s p=%g" % (kind, p), 2048, 2048, 1, 1, p, kind)


def _hidden_chunk_mask(L):
    """Queries [0, 128) — a whole query block — cannot see keys [64, 128) — a whole key chunk; queries [128, L) cannot see the
    FIRST chunk (their running maximum is still -inf after it); key 150 is hidden from every query."""
    m = torch.zeros(L, L, dtype=torch.bool)
    m[:B, C:2 * C] = True
    m[B:, :C] = True
    m[:, 150] = True
    return m.cuda()


def test_hidden_chunks_reproducible_and_hidden_keys_get_exact_zeros():
    L, N, heads = 200, 2, 2
    g = torch.Generator().manual_seed(77)
    q, k, v, go = _inputs(L, L, N, heads, g)
    mask = _hidden_chunk_mask(L)
    for p in (0.0, 0.1):
        seed_value = 0xABCDEF0123456789
        seed = _seed_tensor(seed_value)
        a = _run_core(q, k, v, go, heads, p, seed, mask)
        b = _run_core(q, k, v, go, heads, p, seed, mask, packed=False)
        for name in a:                                   # forward and both backward launches, bit for bit
            assert torch.equal(a[name], b[name]), name
        keep = torch.from_numpy(_keep_mask(seed_value, N * heads, L, L, p)).cuda() if p > 0 else None
        r64 = _formula(q, k, v, go, heads, keep, p, mask, torch.float64)
        t32 = _formula(q, k, v, go, heads, keep, p, mask, torch.float32)
        for name in ("out", "dq", "dk", "dv"):
            _rule("hidden chunks p=%g" % p, name, a[name], t32[name], r64[name])
        _rule("hidden chunks p=%g" % p, "lse", a["lse"].view(N * heads, L), t32["lse"], r64["lse"])
        # key 150 is visible to no query: exactly nothing arrives
        assert (a["dk"][150] == 0).all() and (a["dv"][150] == 0).all()
        assert a["dk"][149].abs().max() > 0 and a["dv"][151].abs().max() > 0


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
        assert torch.isnan(out1[137]).all()
        rows = torch.arange(L, device="cuda") != 137
        assert torch.equal(out1[rows], out0[rows]) and torch.isfinite(out0).all()
        assert torch.equal(lse1[:, rows], lse0[:, rows])


def test_python_argument_errors_and_mask_views():
    from uvhand_amd import _native
    q = torch.randn(2049, 1, 32, device="cuda")
    with pytest.raises(RuntimeError, match="2048"):
        _native.attn32x_forward(q, q, q, 1, 1.0)
    q = torch.randn(40, 1, 32, device="cuda")
    with pytest.raises(RuntimeError, match="seed"):
        _native.attn32x_forward(q, q, q, 1, 1.0, 0.1, None)
    with pytest.raises(RuntimeError, match="mask"):
        _native.attn32x_forward(q, q, q, 1, 1.0, mask=torch.zeros(40, 41, dtype=torch.bool, device="cuda"))
    with pytest.raises(RuntimeError, match="mask"):
        _native.attn32x_forward(q, q, q, 1, 1.0, mask=torch.zeros(40, 40, device="cuda"))
    # a mask that is a view with a longer row stride is read in place; a transposed one is copied: the same result
    g = torch.Generator().manual_seed(5)
    m = _random_mask(40, 40, g)
    wide = torch.ones(40, 57, dtype=torch.bool, device="cuda")
    wide[:, 3:43] = m
    ref, _ = _native.attn32x_forward(q, q, q, 1, 1.0, mask=m)
    assert torch.equal(_native.attn32x_forward(q, q, q, 1, 1.0, mask=wide[:, 3:43])[0], ref)
    assert torch.equal(_native.attn32x_forward(q, q, q, 1, 1.0, mask=m.t().contiguous().t())[0], ref)


# ---- the wrapper ------------------------------------------------------------------------------------------------------------

def _core_launches(monkeypatch):
    """Launches (msda_launch_count) made inside the core's calls, per entry: the projections' weight-gradient kernels count
    launches of their own around them."""
    from uvhand_amd import _native
    seen = {"attn32x_forward": 0, "attn32x_backward": 0, "attn32_forward": 0, "attn32_backward": 0}
    for name in seen:
        orig = getattr(_native, name)

        def wrapped(*a, _o=orig, _n=name, **kw):
            n0 = _native.launch_count()
            res = _o(*a, **kw)
            seen[_n] += _native.launch_count() - n0
            return res
        monkeypatch.setattr(_native, name, wrapped)
    return seen


def _module_grads(mha, fn, x_qk, x_v, go):
    a, b = x_qk.clone().requires_grad_(True), x_v.clone().requires_grad_(True)
    mha.zero_grad()
    out = fn(a, b)
    out.backward(go)
    return [out.detach(), a.grad, b.grad] + [p.grad.clone() for p in mha.parameters()]


@pytest.mark.parametrize("L", [50, 400])
def test_wrapper_equals_the_module_under_the_denoising_mask(monkeypatch, L):
    from uvhand_amd.functions.attention_func import self_attention
    from uvhand_amd.utils import cdn_attention_mask
    seen = _core_launches(monkeypatch)
    N = 2
    torch.manual_seed(3)
    mha = nn.MultiheadAttention(256, 8, dropout=0.1).cuda().eval()
    m = cdn_attention_mask(3, 2, L - 12, "cuda")
    assert tuple(m.shape) == (L, L)
    x_qk, x_v, go = (torch.randn(L, N, 256, device="cuda") for _ in range(3))
    ours = _module_grads(mha, lambda a, b: self_attention(mha, a, b, attn_mask=m), x_qk, x_v, go)
    assert seen == {"attn32x_forward": 1, "attn32x_backward": 2, "attn32_forward": 0, "attn32_backward": 0}
    stock = _module_grads(mha, lambda a, b: mha(a, a, b, attn_mask=m)[0], x_qk, x_v, go)
    mha64 = copy.deepcopy(mha).double()
    ref = _module_grads(mha64, lambda a, b: mha64(a, a, b, attn_mask=m)[0], x_qk.double(), x_v.double(), go.double())
    names = ["out", "grad_x_qk", "grad_x_v"] + ["grad_" + n for n, _ in mha.named_parameters()]
    for name, a, b, r in zip(names, ours, stock, ref):
        _rule("wrapper L=%d" % L, name, a, b, r)
    # a float mask of the same meaning is the module's: no core launch
    before = dict(seen)
    fm = torch.zeros(L, L, device="cuda").masked_fill(m, float("-inf"))
    out_f = self_attention(mha, x_qk, x_v, attn_mask=fm)
    assert seen == before
    assert torch.allclose(out_f, stock[0], atol=1e-5)


def test_defaults_and_the_opt_in_knob(monkeypatch):
    from uvhand_amd import _native
    from uvhand_amd.functions.attention_func import self_attention
    from uvhand_amd.functions.linear_func import bracket_linear_wb
    seen = _core_launches(monkeypatch)
    monkeypatch.delenv("MSDA_ATTN_LONG", raising=False)
    torch.manual_seed(4)
    mha = nn.MultiheadAttention(256, 8, dropout=0.1).cuda().eval()
    x = torch.randn(400, 2, 256, device="cuda", requires_grad=True)
    n0 = _native.launch_count()
    stock = self_attention(mha, x, x)
    assert _native.launch_count() == n0 and not any(seen.values())          # no mask, no knob: the module, no library launch at all
    monkeypatch.setenv("MSDA_ATTN_LONG", "1")
    out = self_attention(mha, x, x)
    out.sum().backward()
    assert seen == {"attn32x_forward": 1, "attn32x_backward": 2, "attn32_forward": 0, "attn32_backward": 0}
    assert torch.allclose(out, stock, atol=1e-5)
    # L <= 320: the resident core still runs, knob or no knob — its bits
    for knob in ("1", None):
        monkeypatch.setenv("MSDA_ATTN_LONG", knob) if knob else monkeypatch.delenv("MSDA_ATTN_LONG")
        y = torch.randn(300, 2, 256, device="cuda")
        before = dict(seen)
        got = self_attention(mha, y, y)
        assert seen["attn32_forward"] == before["attn32_forward"] + 1 and seen["attn32x_forward"] == before["attn32x_forward"]
        w, b = mha.in_proj_weight, mha.in_proj_bias
        qk, v = bracket_linear_wb(y, w[:512], b[:512]), bracket_linear_wb(y, w[512:], b[512:])      # (the wrapper's projections)
        core, _ = _native.attn32_forward(qk[..., :256], qk[..., 256:], v, 8, SCALE)
        assert torch.equal(got, bracket_linear_wb(core, mha.out_proj.weight, mha.out_proj.bias))
    # autocast and other head sizes keep the module, mask or no mask
    before = dict(seen)
    m = torch.zeros(400, 400, dtype=torch.bool, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        self_attention(mha, x, x, attn_mask=m)
    wide = nn.MultiheadAttention(256, 4).cuda().eval()
    self_attention(wide, x, x, attn_mask=m)
    self_attention(mha, x, x, attn_mask=m[None].expand(16, 400, 400))
    assert seen == before


def test_training_draws_from_torchs_generator():
    from uvhand_amd.functions.attention_func import self_attention
    from uvhand_amd.utils import cdn_attention_mask
    torch.manual_seed(5)
    mha = nn.MultiheadAttention(256, 8, dropout=0.1).cuda().train()
    m = cdn_attention_mask(3, 5, 370, "cuda")
    x = torch.randn(400, 2, 256, device="cuda", requires_grad=True)
    torch.manual_seed(11)
    a = self_attention(mha, x, x, attn_mask=m)
    torch.manual_seed(11)
    b = self_attention(mha, x, x, attn_mask=m)
    c = self_attention(mha, x, x, attn_mask=m)
    assert torch.equal(a, b) and not torch.equal(a, c)
    a.sum().backward()
    assert torch.isfinite(x.grad).all() and torch.isfinite(mha.in_proj_weight.grad).all()


def test_decoder_layer_with_a_self_attention_mask():
    """The layer with self_attn_mask on the long core against the same layer with self_attn run by the stock module (a listener
    on attn_matrix asks for it), eval mode; reference: an fp64 copy of the layer, the module inside."""
    from conftest import load_golden
    from uvhand_amd.modules import DeformableTransformerDecoder, DeformableTransformerDecoderLayer
    from uvhand_amd.utils import cdn_attention_mask
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
        out = mod(tgt, cu("qpos", dt), cu("ref", dt), cu("memory", dt), cu("shapes"), cu("level_start"), cu("mask"),
                  self_attn_mask=m)
        out.backward(cu("gout", dt))
        if handle is not None:
            handle.remove()
        return out.detach(), tgt.grad
    ours = run(layer, torch.float32, False)
    stock = run(layer, torch.float32, True)
    ref = run(copy.deepcopy(layer).double(), torch.float64, True)
    for name, a, b, r in zip(("out", "grad_tgt"), ours, stock, ref):
        _rule("decoder layer", name, a, b, r)
    unmasked = layer(cu("tgt"), cu("qpos"), cu("ref"), cu("memory"), cu("shapes"), cu("level_start"), cu("mask"))
    assert not torch.allclose(unmasked, ours[0], atol=1e-4)                 # the mask took part
    # the decoder hands tgt_mask to every layer
    dec = DeformableTransformerDecoder(layer, 2).cuda().eval()
    valid = torch.ones(z["tgt"].shape[0], 4, 2, device="cuda")
    refp = torch.rand(z["tgt"].shape[0], Q, 2, device="cuda")
    args = (cu("tgt"), refp, cu("memory"), cu("shapes"), cu("level_start"), valid, cu("qpos"), cu("mask"))
    with_mask, _ = dec(*args, tgt_mask=m)
    without, _ = dec(*args)
    assert torch.isfinite(with_mask).all() and not torch.allclose(with_mask, without, atol=1e-4)


def test_masked_node_captures_in_a_graph():
    from uvhand_amd.functions.attention_func import _AttnFn
    from uvhand_amd.utils import cdn_attention_mask
    L, N, heads = 200, 2, 2
    E = heads * 32
    g = torch.Generator().manual_seed(9)
    qk = torch.randn(L, N, 2 * E, generator=g).cuda().requires_grad_(True)
    v = torch.randn(L, N, E, generator=g).cuda().requires_grad_(True)
    go = torch.randn(L, N, E, generator=g).cuda()
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
