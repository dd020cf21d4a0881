"""The opt-in bf16 form of the Swin window attention (csrc/msda_swin.hip, msda_swin_attn_*_bf16; MSDA_SWIN_BF16=1): the node against
an fp64 restatement on the same bf16-rounded inputs and against the fp32 kernels, the route a block takes under bf16 autocast, the
backbone fixtures, reproducibility, host syncs, graph capture, checkpointing, and the knob's default (off).

Error measure and tolerances are those of tests/test_attention_bf16_gpu.py: max|a - b| / (max|b| + 0.1); 1e-2 for activations,
2e-2 for gradients (P, dS and the results are rounded to bf16, 2^-9 relative each).  Where the stock composition under the same
autocast is further from the yardstick than that (it rounds the scores to bf16 too, and in a whole block or backbone both routes
carry the Linears' bf16 rounding), the kernel route may be up to twice as far as the composition: a maximum over a few thousand
elements of two different summation orders fluctuates by about that factor."""
import copy
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import swin_inputs as SI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.swin_func import (relative_position_index, shift_mask, window_attention,  # noqa: E402
                                            window_attention_reference, window_partition)
from uvhand_amd.modules import (BasicLayer, Joiner, PositionEmbeddingSine, SwinTransformer,  # noqa: E402
                                SwinTransformerBlock)
from uvhand_amd.modules.detr import NestedTensor  # noqa: E402
from uvhand_amd.modules.swin import OWN_SHIFT_MASK  # noqa: E402

pytestmark = pytest.mark.gpu

ACT, GRAD, LSE = 1e-2, 2e-2, 1e-4
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16

GEOMETRIES = [  # B, H, W, nH, ws, shift: the small ones of test_swin_gpu.GEOMETRIES
    (1, 7, 7, 1, 7, 0),        # one window of 49 tokens, padded to 64 keys: one full pair and a ragged one
    (2, 9, 11, 2, 7, 3),       # padded and shifted: padded keys, all nine shift regions
    (1, 14, 14, 24, 12, 6),    # the Swin-L stage-2 window: 144 tokens padded to 160, 9 wavefronts, 24 heads
    (4, 5, 13, 3, 12, 0),      # mostly padding, no shift
    (1, 3, 17, 4, 7, 3),       # a strip
    (1, 1, 1, 2, 12, 6),       # one real token in a 144-token window
    (2, 10, 6, 4, 5, 2),       # ws 5: N = 25, padded to 32
    (2, 24, 12, 8, 12, 0),     # no padding: the bias gradient must be exactly zero
    (2, 56, 56, 3, 7, 3),      # many windows
]


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-1)).item()


def _accept(what, err, comp_err, tol):
    """The rule of the module docstring; the figures are printed before the assertion."""
    print("%s: kernel route %.3e, composition %.3e, tolerance %.0e" % (what, err, comp_err, tol))
    assert err <= max(tol, 2.0 * comp_err), (what, err, comp_err)


def _node_inputs(B, H, W, nH, ws, bias=True, seed=0):
    """As test_swin_gpu._node_inputs, qkv and grad_out rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    C = 32 * nH
    qkv = torch.randn(B * H * W, 3 * C, generator=g).to(BF16).to(DEV)
    b = (torch.randn(3 * C, generator=g) * 0.5).to(DEV) if bias else None
    table = (torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5).to(DEV)
    go = torch.randn(B * H * W, C, generator=g).to(BF16).to(DEV)
    return qkv, b, table, go


def _node(geo, qkv, b, table, go):
    out, lse = _native.swin_attn_forward(geo, qkv, b, table)
    gq, gt, gb = _native.swin_attn_backward(geo, qkv, b, table, out, lse, go)
    return out, lse, gq, gt, gb


def _real_queries(geo):
    """[B, nW, nH, N] as the kernels' lse buffer: True where the window position holds a real token (only those are written)."""
    B, H, W, C, nH, ws, s = geo
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    idx = F.pad(torch.ones(B, H, W, 1, dtype=torch.float64), (0, 0, 0, Wp - W, 0, Hp - H))
    if s > 0:
        idx = torch.roll(idx, shifts=(-s, -s), dims=(1, 2))
    return window_partition(idx, ws).view(B, -1, 1, ws * ws).expand(B, -1, nH, ws * ws) > 0


def _fp64(geo, qkv, b, table, go):
    """window_attention_reference on the CPU in float64 (a padded token's k and v: the bias rounded to bf16), and the
    log-sum-exp of its scores with the mask of real queries, both [B, nW, nH, N] as the kernels' lse buffer."""
    B, H, W, C, nH, ws, s = geo
    leaves = [qkv.cpu().double().requires_grad_(True), b.to(BF16).cpu().double().requires_grad_(True) if b is not None else None,
              table.cpu().double().requires_grad_(True)]
    out = window_attention_reference(leaves[0], leaves[1], leaves[2], geo)
    out.backward(go.cpu().double())
    grads = [t.grad if t is not None else None for t in leaves]
    # the scores once more, for the log-sum-exp: the restatement's own steps up to the softmax
    Hp, Wp, N = -(-H // ws) * ws, -(-W // ws) * ws, ws * ws
    with torch.no_grad():
        x = F.pad(leaves[0].view(B, H, W, 3 * C), (0, 0, 0, Wp - W, 0, Hp - H))
        idx = F.pad(torch.ones(B, H, W, 1, dtype=torch.float64), (0, 0, 0, Wp - W, 0, Hp - H))
        if leaves[1] is not None:
            x = x + (1 - idx) * leaves[1]
        if s > 0:
            x, idx = (torch.roll(t, shifts=(-s, -s), dims=(1, 2)) for t in (x, idx))
        xw = window_partition(x, ws).view(-1, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
        attn = (xw[0] * 32 ** -0.5) @ xw[1].transpose(-2, -1)
        attn = attn + leaves[2][relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1).unsqueeze(0)
        if s > 0:
            mask = shift_mask(H, W, ws, s, "cpu").double()
            attn = (attn.view(B, mask.shape[0], nH, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, nH, N, N)
        lse = torch.logsumexp(attn, -1).view(B, -1, nH, N)
    return out.detach(), grads, lse, _real_queries(geo)


def _composition(geo, qkv, b, table, go, monkeypatch):
    """The stock composition under bf16 autocast on the same inputs (MSDA_SWIN_FUSED=0)."""
    monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
    leaves = [t.detach().clone().requires_grad_(True) if t is not None else None for t in (qkv, b, table)]
    n0 = _native.launch_count()
    with torch.autocast("cuda", dtype=BF16):
        out = window_attention(leaves[0], leaves[1], leaves[2], geo)
    out.backward(go.to(out.dtype))
    assert _native.launch_count() == n0
    monkeypatch.delenv("MSDA_SWIN_FUSED")
    return out.detach(), [t.grad if t is not None else None for t in leaves]


@pytest.mark.parametrize("geo6", GEOMETRIES)
@pytest.mark.parametrize("bias", [True, False])
def test_node_matches_fp64(geo6, bias, monkeypatch):
    B, H, W, nH, ws, s = geo6
    geo = (B, H, W, 32 * nH, nH, ws, s)
    args = _node_inputs(B, H, W, nH, ws, bias, seed=sum(geo6))
    out, lse, gq, gt, gb = _node(geo, *args)
    assert out.dtype == gq.dtype == BF16 and lse.dtype == gt.dtype == torch.float32
    assert out.shape == (B * H * W, 32 * nH) and gq.shape == args[0].shape and gt.shape == args[2].shape
    assert (gb is None) == (not bias) and (gb is None or (gb.dtype == torch.float32 and gb.shape == args[1].shape))
    r_out, (r_gq, r_gb, r_gt), r_lse, real = _fp64(geo, *args)
    c_out, (c_gq, c_gb, c_gt) = _composition(geo, *args, monkeypatch)
    _accept("out", _rel(out, r_out), _rel(c_out, r_out), ACT)
    _accept("grad_qkv", _rel(gq, r_gq), _rel(c_gq, r_gq), GRAD)
    _accept("grad_table", _rel(gt, r_gt), _rel(c_gt, r_gt), GRAD)
    if bias:
        C = 32 * nH
        assert torch.count_nonzero(gb[:C]) == 0                            # q part: padded queries produce nothing
        if r_gb is None:                                                    # unpadded: the restatement never reads the bias
            assert torch.count_nonzero(gb) == 0
        else:
            _accept("grad_qkv_bias", _rel(gb, r_gb), _rel(c_gb, r_gb), GRAD)
    got = lse.cpu().double()[:real.numel()].view(real.shape)
    assert real.sum().item() == B * H * W * nH
    err = (got - r_lse)[real].abs().max().item()
    print("lse: %.3e" % err)
    assert err < LSE


@pytest.mark.parametrize("geo6", GEOMETRIES)
@pytest.mark.parametrize("bias", [True, False])
def test_node_matches_the_fp32_kernels(geo6, bias):
    """The same bf16 inputs upcast through msda_swin_attn_*_f32 (the bias rounded to bf16 first: the padded tokens' k and v)."""
    B, H, W, nH, ws, s = geo6
    geo = (B, H, W, 32 * nH, nH, ws, s)
    qkv, b, table, go = _node_inputs(B, H, W, nH, ws, bias, seed=sum(geo6) + 1)
    out, lse, gq, gt, gb = _node(geo, qkv, b, table, go)
    b32 = b.to(BF16).float() if bias else None
    f_out, f_lse, f_gq, f_gt, f_gb = _node(geo, qkv.float(), b32, table, go.float())
    assert f_out.dtype == f_gq.dtype == torch.float32
    assert _rel(out, f_out) < ACT
    assert _rel(gq, f_gq) < GRAD and _rel(gt, f_gt) < GRAD
    real = _real_queries(geo).reshape(-1).to(DEV)
    assert (lse - f_lse)[real].abs().max().item() < LSE
    if bias:
        assert _rel(gb, f_gb) < GRAD
        if H % ws == 0 and W % ws == 0:                                     # unpadded: exactly zero
            assert torch.count_nonzero(gb) == 0


def _block(dim=192, heads=6, ws=12, shift=6, H=14, W=14, seed=0):
    torch.manual_seed(seed)
    blk = SwinTransformerBlock(dim, heads, ws, shift).to(DEV)
    blk.H, blk.W = H, W
    return blk


_BLOCK_GRADS = ("attn.relative_position_bias_table", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "norm1.weight",
                "mlp.fc2.weight")


def _block_step(blk, x, w, autocast):
    """(y, launches forward, launches backward, [x.grad] + the gradients of _BLOCK_GRADS, the dtype the proj Linear was fed)"""
    blk.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    seen = []
    hook = blk.attn.proj.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].dtype))
    n0 = _native.launch_count()
    if autocast is None:
        y = blk(x, OWN_SHIFT_MASK)
    else:
        with torch.autocast("cuda", dtype=autocast):
            y = blk(x, OWN_SHIFT_MASK)
    n1 = _native.launch_count()
    (y.to(w.dtype) * w).sum().backward()
    n2 = _native.launch_count()
    hook.remove()
    params = dict(blk.named_parameters())
    return y.detach(), n1 - n0, n2 - n1, [x.grad] + [params[k].grad for k in _BLOCK_GRADS], seen[0]


def test_block_route_under_autocast(monkeypatch):
    """Fails without the bf16 form: there the knob is ignored and the launch count stays 0."""
    blk = _block(seed=4)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 14 * 14, 192, generator=g).to(DEV)
    w = torch.randn(2, 14 * 14, 192, generator=g).to(DEV)
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    y, nf, nb, grads, node_dtype = _block_step(blk, x, w, BF16)
    assert (nf, nb) == (1, 3)
    assert y.dtype == x.dtype == torch.float32 and node_dtype == BF16
    _, nf16, nb16, _, _ = _block_step(blk, x, w, torch.float16)           # fp16 autocast: the composition
    assert (nf16, nb16) == (0, 0)
    monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
    c_y, cf, cb, c_grads, _ = _block_step(blk, x, w, BF16)
    assert (cf, cb) == (0, 0)
    monkeypatch.delenv("MSDA_SWIN_FUSED")
    ref = copy.deepcopy(blk).cpu().double()
    xr = x.cpu().double().requires_grad_(True)
    r_y = ref(xr, OWN_SHIFT_MASK)
    (r_y * w.cpu().double()).sum().backward()
    rp = dict(ref.named_parameters())
    r_grads = [xr.grad] + [rp[k].grad for k in _BLOCK_GRADS]
    _accept("y", _rel(y, r_y), _rel(c_y, r_y), ACT)
    for name, a, c, r in zip(("x",) + _BLOCK_GRADS, grads, c_grads, r_grads):
        _accept("grad " + name, _rel(a, r), _rel(c, r), GRAD)


def test_knob_off_makes_no_launch(monkeypatch):
    blk = _block(seed=4)
    x = torch.randn(2, 14 * 14, 192, device=DEV)
    w = torch.randn(2, 14 * 14, 192, device=DEV)
    for value in (None, "0"):
        if value is None:
            monkeypatch.delenv("MSDA_SWIN_BF16", raising=False)
        else:
            monkeypatch.setenv("MSDA_SWIN_BF16", value)
        for dtype in (BF16, torch.float16):
            _, nf, nb, _, node_dtype = _block_step(blk, x, w, dtype)
            assert (nf, nb) == (0, 0) and node_dtype == dtype


def _backbone_run(name, z, monkeypatch, fused):
    monkeypatch.setenv("MSDA_SWIN_FUSED", "1" if fused else "0")
    m = SI.build_backbone(SwinTransformer, Joiner, PositionEmbeddingSine, name).to(DEV)
    img, mask = SI.backbone_input(name)
    x = img.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    with torch.autocast("cuda", dtype=BF16):
        feats, _ = m(NestedTensor(x, mask.to(DEV)))
    launches = _native.launch_count() - n0
    SI.weighted_sum([f.tensors.float() for f in feats], SI.BACKBONE_CASES[name]["seed"] + 7).backward()
    errs = {"out%d" % i: _rel(f.tensors, z["out%d" % i]) for i, f in enumerate(feats)}
    errs["grad_x"] = _rel(x.grad, z["grad_x"])
    for k, p in m.named_parameters():
        g = p.grad.detach().cpu().double()
        if k + "/grad/" in z:
            errs["grad " + k] = _rel(g, z[k + "/grad/"])
        else:                                   # kept as sums: relative to the largest of the sums and the gradient itself
            refs = [(g.sum(0), z[k + "/gradsum0/"])] + ([(g.sum(1), z[k + "/gradsum1/"])] if g.dim() > 1 else [])
            scale = max([np.abs(r).max() for _, r in refs] + [g.abs().max().item()]) + 1e-1
            errs["grad " + k] = max(float(np.abs(s.numpy() - r).max()) / scale for s, r in refs)
    return launches, errs


@pytest.mark.parametrize("name", list(SI.BACKBONE_CASES))
def test_backbone_fixture_under_autocast(name, monkeypatch):
    """The goldens are fp32 results of the reference's code; the composition under the same autocast is the comparison route."""
    z = load_golden(name)
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    launches, errs = _backbone_run(name, z, monkeypatch, True)
    assert launches == sum(SI.BACKBONE_CASES[name]["depths"])                  # one launch per block
    c_launches, c_errs = _backbone_run(name, z, monkeypatch, False)
    assert c_launches == 0
    for key in errs:
        _accept(key, errs[key], c_errs[key], ACT if key.startswith("out") else GRAD)


def _assert_same(geo, a, b):
    """The node's five results bit for bit; of the lse buffer the real queries' entries (no kernel writes the others)."""
    assert len(a) == len(b) == 5
    real = _real_queries(geo).reshape(-1).to(DEV)
    for name, u, v in zip(("out", "lse", "grad_qkv", "grad_table", "grad_qkv_bias"), a, b):
        assert torch.equal(u[real], v[real]) if name == "lse" else torch.equal(u, v), name


def test_bitwise_reproducible():
    geo = (3, 14, 14, 768, 24, 12, 6)
    args = _node_inputs(3, 14, 14, 24, 12, seed=7)
    _assert_same(geo, _node(geo, *args), _node(geo, *args))
    geo = (2, 9, 11, 64, 2, 7, 3)                                               # padded: a bias gradient that is not zero
    args = _node_inputs(2, 9, 11, 2, 7, seed=8)
    a = _node(geo, *args)
    assert a[4].abs().max() > 0
    _assert_same(geo, a, _node(geo, *args))


def test_no_host_sync(monkeypatch):
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    geo = (2, 9, 11, 64, 2, 7, 3)
    qkv, b, table, go = _node_inputs(2, 9, 11, 2, 7, seed=9)
    leaves = [t.clone().requires_grad_(True) for t in (qkv, b, table)]
    window_attention(*leaves, geo).backward(go)                                # (first call: module load, LDS opt-in)
    torch.cuda.synchronize()
    n0 = _native.launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        window_attention(*leaves, geo).backward(go)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert _native.launch_count() - n0 == 4


def test_graph_capture(monkeypatch):
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    geo = (1, 14, 14, 192, 6, 12, 6)
    args = _node_inputs(1, 14, 14, 6, 12, seed=10)
    eager = [t.clone() for t in _node(geo, *args)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _node(geo, *args)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _node(geo, *args)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    _assert_same(geo, eager, static)


def test_checkpointed_layer_matches_plain(monkeypatch):
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    depth, H, W = 2, 9, 11

    def layer(use_checkpoint):
        torch.manual_seed(31)
        return BasicLayer(64, depth, 2, window_size=7, use_checkpoint=use_checkpoint).to(DEV)
    plain, ckpt = layer(False), layer(True)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, H * W, 64, generator=g).to(DEV)
    w = torch.randn(2, H * W, 64, generator=g).to(DEV)
    res = []
    for m in (plain, ckpt):
        xx = x.clone().requires_grad_(True)
        n0 = _native.launch_count()
        with torch.autocast("cuda", dtype=BF16):
            y = m(xx, H, W)[0]
        (y * w).sum().backward()
        res.append((_native.launch_count() - n0, y.detach(), xx.grad, [p.grad for p in m.parameters()]))
    (na, ya, xa, pa), (nb, yb, xb, pb) = res
    assert na == depth * (1 + 3) and nb == depth * (1 + 1 + 3)
    assert torch.equal(ya, yb) and torch.equal(xa, xb)
    assert all(torch.equal(u, v) for u, v in zip(pa, pb))
