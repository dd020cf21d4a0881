"""The opt-in HIP glue of the Swin blocks (csrc/msda_swin_glue.hip, msda_swin_glue_*; MSDA_SWIN_GLUE=1): norm, add + norm, add and
merge + norm against torch's own expressions (bit for bit where the issue is an add) and against float64, the route a block and a
backbone take with the knob on and off, drop-path parity, checkpointing, reproducibility, host syncs and graph capture.

Error measure and acceptance rule are those of tests/test_swin_bf16_gpu.py: max|a - b| / (max|b| + 0.1) against a float64
restatement on the same (bf16-rounded where T is bf16) inputs, accepted up to max(floor, 2 x the error of torch's composition on
the GPU on the same inputs).  Floors: bf16 outputs ACT = 1e-2 (activations) and GRAD = 2e-2 (gradients), as there; fp32 outputs
1e-5, about a hundred fp32 ulps of the maximum (a wrong channel, row or statistic shows at 1e-2 and above).  The keep vectors hold
0 and 2 (drop_path 0.5), so the product a * keep is exact in either type and the float64 restatement needs no rounding."""
import copy
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import swin_inputs as SI  # noqa: E402
from test_swin_bf16_gpu import ACT, GRAD, _BLOCK_GRADS, _accept, _block, _block_step, _rel  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.swin_glue_func import add_norm_rows, add_rows, merge_norm, norm_rows  # noqa: E402
from uvhand_amd.modules import (BasicLayer, Joiner, PatchMerging, PositionEmbeddingSine, SwinTransformer,  # noqa: E402
                                SwinTransformerBlock)
from uvhand_amd.modules.detr import NestedTensor  # noqa: E402
from uvhand_amd.modules.swin import OWN_SHIFT_MASK  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = 1e-5
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
EPS = 1e-5

WIDTHS = [8, 96, 192, 1024, 1028, 1536, 3072]          # 96: a partly filled wavefront; 1024 | 1028: registers | LDS column sums
# (samples, rows per sample): 1, 3, 5 rows (fewer than a workgroup's wavefronts), 13 = 4 k + 1 (a ragged last workgroup),
# 3 x 5 (a workgroup straddles samples), 37 rows (three workgroups of partials in the backward)
SAMPLES = [(1, 1), (3, 1), (1, 5), (13, 1), (3, 5), (37, 1)]
MERGES = [((1, 1, 1), 8), ((2, 3, 5), 96), ((1, 4, 6), 8), ((2, 7, 2), 768)]
TYPES = [torch.float32, BF16]


def _floors(T):
    return (F32, F32) if T == torch.float32 else (ACT, GRAD)


def _keep(B, T, seed):
    """0 and 2 with at least one zero."""
    g = torch.Generator().manual_seed(seed)
    k = (torch.rand(B, generator=g) < 0.5).float() * 2
    k[seed % B] = 0
    return k.to(T).view(B, 1, 1)


def _inputs(B, L, C, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, C, generator=g) * 1.5 + 0.3
    a = torch.randn(B, L, C, generator=g).to(T)
    gy = torch.randn(B, L, C, generator=g)
    gz = torch.randn(B, L, C, generator=g).to(T)
    w = torch.randn(C, generator=g) * 0.5 + 1
    b = torch.randn(C, generator=g) * 0.5
    return x, a, gy, gz, w, b


def _norm_module(w, b, device, dtype=torch.float32):
    m = torch.nn.LayerNorm(w.numel(), eps=EPS)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    return m.to(device=device, dtype=dtype)


def _run(fn, tensors, grads, norm):
    """fn(*leaves) -> outputs; backward with `grads`; (outputs, leaf gradients, parameter gradients)."""
    leaves = [t.detach().clone().requires_grad_(True) for t in tensors]
    if norm is not None:
        norm.zero_grad(set_to_none=True)
    outs = fn(*leaves)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward(outs, [g.to(device=o.device, dtype=o.dtype) for o, g in zip(outs, grads)])
    pg = [norm.weight.grad, norm.bias.grad] if norm is not None else []
    return [o.detach() for o in outs], [t.grad for t in leaves], pg


@pytest.fixture(autouse=True)
def _glue_on(monkeypatch):
    monkeypatch.setenv("MSDA_SWIN_GLUE", "1")
    monkeypatch.delenv("MSDA_SWIN_BF16", raising=False)
    monkeypatch.delenv("MSDA_SWIN_FUSED", raising=False)


class _as_T:
    """The autocast state that makes T the glue's branch type."""

    def __init__(self, T):
        self.ctx = torch.autocast("cuda", dtype=BF16, enabled=T == BF16)

    def __enter__(self):
        return self.ctx.__enter__()

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


@pytest.mark.parametrize("T", TYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", WIDTHS)
def test_add_is_torchs_bit_for_bit(C, T):
    for i, (B, L) in enumerate(SAMPLES):
        x, a, gy, _, _, _ = _inputs(B, L, C, T, 100 + C + i)
        for keep in (None, _keep(B, T, i)):
            k = keep.to(DEV) if keep is not None else None
            n0 = _native.launch_count()
            with _as_T(T):
                (y,), (gx, ga), _ = _run(lambda u, v: add_rows(u, v, k), [x.to(DEV), a.to(DEV)], [gy], None)
            launches = _native.launch_count() - n0
            assert launches == (1 if (T == torch.float32 and keep is None) else 2), launches
            (ty,), (tgx, tga), _ = _run(lambda u, v: u + (v if k is None else v * k), [x.to(DEV), a.to(DEV)], [gy], None)
            assert y.dtype == torch.float32 and ga.dtype == T and gx.dtype == torch.float32
            assert torch.equal(y, ty) and torch.equal(gx, tgx) and torch.equal(ga, tga), (B, L, keep is None)
            if keep is not None:
                dropped = (keep.view(-1) == 0).to(DEV)
                assert torch.equal(y[dropped], x.to(DEV)[dropped]) and torch.count_nonzero(ga[dropped]) == 0


@pytest.mark.parametrize("T", TYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", WIDTHS)
def test_add_norm_matches_torch_and_fp64(C, T):
    act, grad = _floors(T)
    for i, (B, L) in enumerate(SAMPLES):
        x, a, gy, gz, w, b = _inputs(B, L, C, T, 200 + C + i)
        for keep in (None, _keep(B, T, i + 1)):
            def comp(norm, k, cast):
                def fn(u, v):
                    y = u + (v if k is None else v * k)
                    z = norm(y)
                    return y, (z.to(cast) if cast is not None else z)
                return fn
            k = keep.to(DEV) if keep is not None else None
            norm = _norm_module(w, b, DEV)
            n0 = _native.launch_count()
            with _as_T(T):
                (y, z), (gx, ga), (gw, gb) = _run(lambda u, v: add_norm_rows(u, v, k, norm), [x.to(DEV), a.to(DEV)], [gy, gz], norm)
            assert _native.launch_count() - n0 == 3                          # one forward, the rows' pass and the reduction
            assert y.dtype == gx.dtype == torch.float32 and z.dtype == ga.dtype == T
            (cy, cz), (cgx, cga), (cgw, cgb) = _run(comp(norm, k, T), [x.to(DEV), a.to(DEV)], [gy, gz], norm)
            assert torch.equal(y, cy), (B, L, keep is None)
            n64 = _norm_module(w, b, "cpu", torch.float64)
            k64 = keep.double() if keep is not None else None
            (ry, rz), (rgx, rga), (rgw, rgb) = _run(comp(n64, k64, None), [x.double(), a.double()], [gy, gz], n64)
            tag = "add_norm C=%d %s B=%d L=%d keep=%s " % (C, T, B, L, keep is not None)
            _accept(tag + "z", _rel(z, rz), _rel(cz, rz), act)
            _accept(tag + "grad_x", _rel(gx, rgx), _rel(cgx, rgx), F32)       # fp32 whatever T
            _accept(tag + "grad_a", _rel(ga, rga), _rel(cga, rga), grad)
            _accept(tag + "grad_gamma", _rel(gw, rgw), _rel(cgw, rgw), F32)
            _accept(tag + "grad_beta", _rel(gb, rgb), _rel(cgb, rgb), F32)
            if keep is not None:
                assert torch.count_nonzero(ga[(keep.view(-1) == 0).to(DEV)]) == 0


@pytest.mark.parametrize("T", TYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("C", WIDTHS)
def test_norm_matches_fp64(C, T):
    act, grad = _floors(T)
    for i, (B, L) in enumerate(SAMPLES):
        x, _, _, gz, w, b = _inputs(B, L, C, T, 300 + C + i)
        norm = _norm_module(w, b, DEV)
        n0 = _native.launch_count()
        with _as_T(T):
            (z,), (gx,), (gw, gb) = _run(lambda u: norm_rows(u, norm), [x.to(DEV)], [gz], norm)
            (z32,), _, _ = _run(lambda u: norm_rows(u, norm, fp32_out=True), [x.to(DEV)], [gz], norm)
        assert _native.launch_count() - n0 == 2 * 3
        assert z.dtype == T and z32.dtype == torch.float32 and gx.dtype == torch.float32
        (cz,), (cgx,), (cgw, cgb) = _run(lambda u: norm(u).to(T), [x.to(DEV)], [gz], norm)
        n64 = _norm_module(w, b, "cpu", torch.float64)
        (rz,), (rgx,), (rgw, rgb) = _run(lambda u: n64(u), [x.double()], [gz], n64)
        tag = "norm C=%d %s B=%d L=%d " % (C, T, B, L)
        _accept(tag + "z", _rel(z, rz), _rel(cz, rz), act)
        _accept(tag + "z fp32", _rel(z32, rz), _rel(norm(x.to(DEV)), rz), F32)
        _accept(tag + "grad_x", _rel(gx, rgx), _rel(cgx, rgx), F32)
        _accept(tag + "grad_gamma", _rel(gw, rgw), _rel(cgw, rgw), F32)
        _accept(tag + "grad_beta", _rel(gb, rgb), _rel(cgb, rgb), F32)


def _merge_reference(x, H, W, norm, cast=None):
    B, L, C = x.shape
    t = F.pad(x.view(B, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
    t = torch.cat([t[:, 0::2, 0::2, :], t[:, 1::2, 0::2, :], t[:, 0::2, 1::2, :], t[:, 1::2, 1::2, :]], -1)
    z = norm(t.view(B, -1, 4 * C))
    return z.to(cast) if cast is not None else z


@pytest.mark.parametrize("T", TYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("bhw,C", MERGES)
def test_merge_norm_matches_fp64(bhw, C, T):
    act, grad = _floors(T)
    B, H, W = bhw
    g = torch.Generator().manual_seed(400 + C + H)
    x = torch.randn(B, H * W, C, generator=g) * 1.5 + 0.3
    L2 = (H + 1) // 2 * ((W + 1) // 2)
    gz = torch.randn(B, L2, 4 * C, generator=g).to(T)
    w, b = torch.randn(4 * C, generator=g) * 0.5 + 1, torch.randn(4 * C, generator=g) * 0.5
    norm = _norm_module(w, b, DEV)
    n0 = _native.launch_count()
    with _as_T(T):
        (z,), (gx,), (gw, gb) = _run(lambda u: merge_norm(u, H, W, norm), [x.to(DEV)], [gz], norm)
    assert _native.launch_count() - n0 == 3
    assert z.dtype == T and tuple(z.shape) == (B, L2, 4 * C)
    assert gx.dtype == torch.float32 and gx.shape == x.shape
    (cz,), (cgx,), (cgw, cgb) = _run(lambda u: _merge_reference(u, H, W, norm, T), [x.to(DEV)], [gz], norm)
    n64 = _norm_module(w, b, "cpu", torch.float64)
    (rz,), (rgx,), (rgw, rgb) = _run(lambda u: _merge_reference(u, H, W, n64), [x.double()], [gz], n64)
    tag = "merge_norm %s C=%d %s " % (bhw, C, T)
    _accept(tag + "z", _rel(z, rz), _rel(cz, rz), act)
    _accept(tag + "grad_x", _rel(gx, rgx), _rel(cgx, rgx), F32)
    _accept(tag + "grad_gamma", _rel(gw, rgw), _rel(cgw, rgw), F32)
    _accept(tag + "grad_beta", _rel(gb, rgb), _rel(cgb, rgb), F32)
    # every real token has a gradient (random data: an exact zero means an element nobody wrote or a leak from a pad position)
    assert torch.count_nonzero(gx) == gx.numel() and torch.isfinite(gx).all()
    assert torch.equal(gx == 0, rgx.to(DEV) == 0)


# ---- a block -------------------------------------------------------------------------------------------------------------
BLOCK_BACKWARD = {None: 7, BF16: 8}      # attention 3, add + norm 2, norm 2, and add's grad_a for bf16 (1)


@pytest.mark.parametrize("autocast", [None, BF16], ids=["f32", "bf16"])
def test_block_route(autocast, monkeypatch):
    """Fails without the glue: there the knob is ignored and the counts stay (1, 3)."""
    act, grad = (F32, F32) if autocast is None else (ACT, GRAD)
    if autocast is not None:
        monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    blk = _block(seed=4)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 14 * 14, 192, generator=g).to(DEV)
    w = torch.randn(2, 14 * 14, 192, generator=g).to(DEV)
    y, nf, nb, grads, node_dtype = _block_step(blk, x, w, autocast)
    assert (nf, nb) == (4, BLOCK_BACKWARD[autocast])                           # forward: 1 attention + 3 glue
    assert y.dtype == torch.float32 and node_dtype == (autocast or torch.float32)
    for value in (None, "0"):                                                  # the glue knob unset or off: today's counts
        if value is None:
            monkeypatch.delenv("MSDA_SWIN_GLUE")
        else:
            monkeypatch.setenv("MSDA_SWIN_GLUE", value)
        o_y, of, ob, o_grads, _ = _block_step(blk, x, w, autocast)
        assert (of, ob) == (1, 3)
    monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
    c_y, cf, cb, c_grads, _ = _block_step(blk, x, w, autocast)
    assert (cf, cb) == (0, 0)
    ref = copy.deepcopy(blk).cpu().double()
    xr = x.cpu().double().requires_grad_(True)
    r_y = ref(xr, OWN_SHIFT_MASK)
    (r_y * w.cpu().double()).sum().backward()
    rp = dict(ref.named_parameters())
    r_grads = [xr.grad] + [rp[k].grad for k in _BLOCK_GRADS]
    _accept("y", _rel(y, r_y), _rel(c_y, r_y), act)
    for name, a, c, r in zip(("x",) + _BLOCK_GRADS, grads, c_grads, r_grads):
        _accept("grad " + name, _rel(a, r), _rel(c, r), grad)


def _drop_block(B, seed=4):
    torch.manual_seed(seed)
    blk = SwinTransformerBlock(192, 6, 12, 6, drop_path=0.5).to(DEV).train()
    blk.H, blk.W = 14, 14
    return blk


@pytest.mark.parametrize("autocast", [None, BF16], ids=["f32", "bf16"])
def test_drop_path_parity(autocast, monkeypatch):
    if autocast is not None:
        monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    B = 8
    blk = _drop_block(B)
    x = torch.randn(B, 14 * 14, 192, generator=torch.Generator().manual_seed(21)).to(DEV)
    res = []
    for knob in ("1", "0"):
        monkeypatch.setenv("MSDA_SWIN_GLUE", knob)
        torch.manual_seed(77)
        n0 = _native.launch_count()
        with torch.autocast("cuda", dtype=BF16, enabled=autocast is not None):
            y = blk(x, OWN_SHIFT_MASK)
        res.append((y.detach(), torch.cuda.get_rng_state(DEV), _native.launch_count() - n0))
    (y1, rng1, n1), (y0, rng0, n0) = res
    assert (n1, n0) == (4, 1)
    assert torch.equal(rng1, rng0)                                             # the Philox stream consumed alike
    same1 = (y1 == x).flatten(1).all(1)
    same0 = (y0 == x).flatten(1).all(1)
    assert torch.equal(same1, same0)                                           # the same samples dropped in both branches
    # ... and the same keep values everywhere: a sample kept on one route and dropped on the other would differ by O(1)
    per_sample = (y1 - y0).abs().flatten(1).amax(1) / (y0.abs().flatten(1).amax(1) + 0.1)
    print("drop-path parity: dropped", same1.tolist(), "per-sample difference", per_sample.tolist())
    assert per_sample.max().item() < (1e-4 if autocast is None else 5e-2)


def test_checkpointed_layer_is_bit_identical(monkeypatch):
    depth, H, W = 2, 9, 11

    def layer(use_checkpoint):
        torch.manual_seed(31)
        return BasicLayer(64, depth, 2, window_size=7, drop_path=0.2, downsample=PatchMerging,
                          use_checkpoint=use_checkpoint).to(DEV).train()
    plain, ckpt = layer(False), layer(True)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(4, H * W, 64, generator=g).to(DEV)
    w = torch.randn(4, H * W, 64, generator=g).to(DEV)
    for autocast in (None, BF16):
        if autocast is not None:
            monkeypatch.setenv("MSDA_SWIN_BF16", "1")
        res = []
        for m in (plain, ckpt):
            m.zero_grad(set_to_none=True)
            xx = x.clone().requires_grad_(True)
            torch.manual_seed(5)
            n0 = _native.launch_count()
            with torch.autocast("cuda", dtype=BF16, enabled=autocast is not None):
                out = m(xx, H, W)
            ((out[0] * w).sum() + out[3].float().sum()).backward()
            res.append((_native.launch_count() - n0, out[0].detach(), out[3].detach(), xx.grad, [p.grad for p in m.parameters()]))
        (na, ya, da, xa, pa), (nb, yb, db, xb, pb) = res
        assert nb == na + depth * 4                                            # the blocks' forward once more
        assert torch.equal(ya, yb) and torch.equal(da, db) and torch.equal(xa, xb)
        assert all(torch.equal(u, v) for u, v in zip(pa, pb))


_NODES = (3, 15, 96, 3, 5)                 # B, L, C and the merge's H x W = L


def _node_inputs(T):
    B, L, C, _, _ = _NODES
    return [t.to(DEV) for t in _inputs(B, L, C, T, 500)] + [_keep(B, T, 1).view(-1).to(DEV)]


def _all_nodes(T, x, a, gy, gz, w, b, keep):
    """Every entry once through the binding, on device tensors: forward and backward results of the four operations."""
    B, L, C, H, W = _NODES
    out = []
    z, mean, rstd = _native.swin_glue_norm_forward(x, w, b, EPS, T)
    out += [z, mean, rstd, *_native.swin_glue_norm_backward(gz, x, w, mean, rstd)]
    y, z, mean, rstd = _native.swin_glue_add_norm_forward(x, a, keep, L, w, b, EPS)
    out += [y, z, mean, rstd, *_native.swin_glue_add_norm_backward(gy, gz, y, keep, L, w, mean, rstd)]
    out += [_native.swin_glue_add_forward(x, a, keep, L), _native.swin_glue_add_backward(gy, keep, L, T)]
    w4, b4 = torch.cat([w] * 4), torch.cat([b] * 4)
    x4 = x.view(B, H, W, C)
    z, mean, rstd = _native.swin_glue_merge_norm_forward(x4, w4, b4, EPS, T)
    gz4 = torch.cat([gz[:, :6]] * 4, -1).contiguous()
    out += [z, mean, rstd, *_native.swin_glue_merge_norm_backward(gz4, x4, w4, mean, rstd)]
    return out


@pytest.mark.parametrize("T", TYPES, ids=["f32", "bf16"])
def test_bitwise_reproducible(T):
    args = _node_inputs(T)
    a, b = _all_nodes(T, *args), _all_nodes(T, *args)
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("T", TYPES, ids=["f32", "bf16"])
def test_graph_capture(T):
    args = _node_inputs(T)
    eager = [t.clone() for t in _all_nodes(T, *args)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _all_nodes(T, *args)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _all_nodes(T, *args)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(eager, static))


@pytest.mark.parametrize("autocast", [None, BF16], ids=["f32", "bf16"])
def test_no_host_sync(autocast, monkeypatch):
    if autocast is not None:
        monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    blk = _drop_block(4)
    x = torch.randn(4, 14 * 14, 192, device=DEV, requires_grad=True)

    def step():
        with torch.autocast("cuda", dtype=BF16, enabled=autocast is not None):
            y = blk(x, OWN_SHIFT_MASK)
        y.sum().backward()
    step()                                                                     # (first call: module load)
    torch.cuda.synchronize()
    n0 = _native.launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert _native.launch_count() - n0 == 4 + 8                                # with a keep vector add's grad_a is a launch


# ---- the backbone fixtures -------------------------------------------------------------------------------------------------
def _backbone_run(name, z, autocast):
    m = SI.build_backbone(SwinTransformer, Joiner, PositionEmbeddingSine, name).to(DEV)
    img, mask = SI.backbone_input(name)
    x = img.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    with torch.autocast("cuda", dtype=BF16, enabled=autocast is not None):
        feats, _ = m(NestedTensor(x, mask.to(DEV)))
    launches = _native.launch_count() - n0
    SI.weighted_sum([f.tensors.float() for f in feats], SI.BACKBONE_CASES[name]["seed"] + 7).backward()
    errs = {"out%d" % i: _rel(f.tensors, z["out%d" % i]) for i, f in enumerate(feats)}
    errs["grad_x"] = _rel(x.grad, z["grad_x"])
    for k, p in m.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().cpu().double()
        if k + "/grad/" in z:
            errs["grad " + k] = _rel(g, z[k + "/grad/"])
        else:                                   # kept as sums: relative to the largest of the sums and the gradient itself
            refs = [(g.sum(0), z[k + "/gradsum0/"])] + ([(g.sum(1), z[k + "/gradsum1/"])] if g.dim() > 1 else [])
            scale = max([np.abs(r).max() for _, r in refs] + [g.abs().max().item()]) + 1e-1
            errs["grad " + k] = max(float(np.abs(s.numpy() - r).max()) / scale for s, r in refs)
    return launches, errs


@pytest.mark.parametrize("autocast", [None, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(SI.BACKBONE_CASES))
def test_backbone_fixture(name, autocast, monkeypatch):
    """The goldens are fp32 results of the reference's code; the same route without the glue knob is the comparison."""
    z = load_golden(name)
    act, grad = (F32, F32) if autocast is None else (ACT, GRAD)
    if autocast is not None:
        monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    depths = SI.BACKBONE_CASES[name]["depths"]
    launches, errs = _backbone_run(name, z, autocast)
    if autocast is None:                       # per block 1 attention + 3 glue; 3 patch mergings; 3 output norms
        assert launches == 4 * sum(depths) + 3 + 3
    else:
        # Under autocast PatchMerging's reduction Linear gives bf16 rows, so from stage 1 on the residual stream is bf16 and
        # keeps torch's glue: stage 0's blocks and its patch merging are what takes the kernels.
        assert launches == sum(depths) + 3 * depths[0] + 1
    assert launches > sum(depths)
    monkeypatch.delenv("MSDA_SWIN_GLUE")
    o_launches, o_errs = _backbone_run(name, z, autocast)
    assert o_launches == sum(depths)
    assert sorted(errs) == sorted(o_errs)
    for key in errs:
        _accept(key, errs[key], o_errs[key], act if key.startswith("out") else grad)
