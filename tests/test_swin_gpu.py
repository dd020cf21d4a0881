"""Swin window attention on the HIP kernels (csrc/msda_swin.hip) against the reference's fixtures (gen_golden_r12.py) and the
torch restatement (MSDA_SWIN_FUSED=0): random geometries, the padded tokens' bias gradient, the table gradient, launch counts,
reproducibility, host syncs, graph capture, checkpointing, the fallbacks and a DeformableDETR over the drop-in Joiner."""
import copy
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import swin_inputs as SI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.swin_func import shift_mask, window_attention, window_attention_reference  # noqa: E402
from uvhand_amd.modules import (BasicLayer, Joiner, PositionEmbeddingSine, SwinTransformer,  # noqa: E402
                                SwinTransformerBlock)
from uvhand_amd.modules.detr import NestedTensor  # noqa: E402
from uvhand_amd.modules.swin import OWN_SHIFT_MASK  # noqa: E402

pytestmark = pytest.mark.gpu

ACT, GRAD = 2e-5, 1e-4           # fp32 MFMA against the CPU: as tests/test_detr_gpu.py
DEV = torch.device("cuda:0")


def _sum_err(got, ref, scale):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / scale)


def _check_grads(z, model, tol):
    """Whole gradients by rel_err; the sums of large ones relative to the largest of the two sums and the gradient itself
    (a sum can cancel to rounding noise: LayerNorm'd inputs sum to zero over their features, softmax gradients over their
    keys)."""
    for k, p in model.named_parameters():
        g = p.grad.detach().cpu()
        if k + "/grad/" in z:
            assert rel_err(g.numpy(), z[k + "/grad/"]) < tol, k
        else:
            refs = [z[k + "/gradsum0/"]] + ([z[k + "/gradsum1/"]] if g.dim() > 1 else [])
            scale = max([np.abs(r).max() for r in refs] + [g.abs().max().item()]) + 1e-30
            assert _sum_err(g.sum(0).numpy(), refs[0], scale) < tol, k
            if g.dim() > 1:
                assert _sum_err(g.sum(1).numpy(), refs[1], scale) < tol, k


@pytest.mark.parametrize("name", list(SI.BACKBONE_CASES))
def test_backbone_fixture(name):
    z = load_golden(name)
    m = SI.build_backbone(SwinTransformer, Joiner, PositionEmbeddingSine, name).to(DEV)
    img, mask = SI.backbone_input(name)
    x = img.to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    feats, pos = m(NestedTensor(x, mask.to(DEV)))
    assert _native.launch_count() - n0 == sum(SI.BACKBONE_CASES[name]["depths"])       # one launch per block
    for i, (f, p) in enumerate(zip(feats, pos)):
        assert rel_err(f.tensors.detach().cpu().numpy(), z["out%d" % i]) < ACT, i
        assert np.array_equal(f.mask.cpu().numpy(), z["mask%d" % i])
        assert rel_err(p.cpu().numpy(), z["pos%d" % i]) < 1e-3           # torch's sin / cos on the GPU against the CPU
    SI.weighted_sum([f.tensors for f in feats], SI.BACKBONE_CASES[name]["seed"] + 7).backward()
    assert rel_err(x.grad.cpu().numpy(), z["grad_x"]) < GRAD
    _check_grads(z, m, GRAD)


def test_layer_fixture():
    name = "swin_l_stage2"
    c = SI.LAYER_CASES[name]
    z = load_golden(name)
    m = SI.build_layer(BasicLayer, name).to(DEV)
    x = SI.layer_input(name).to(DEV).requires_grad_(True)
    y = m(x, c["H"], c["W"])[0]
    SI.weighted_sum([y], c["seed"] + 7).backward()
    for key, t in (("out0", y), ("grad_x", x.grad)):
        t = t.detach().cpu()
        tol = ACT if key == "out0" else GRAD
        assert rel_err(t[:, :SI.LAYER_FULL_TOKENS].numpy(), z[key + "/head"]) < tol, key
        assert rel_err(t.sum(1).numpy(), z[key + "/sum1"]) < tol, key
        assert rel_err(t.sum(2).numpy(), z[key + "/sum2"]) < tol, key
    _check_grads(z, m, GRAD)


def _node_inputs(B, H, W, nH, ws, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = 32 * nH
    qkv = torch.randn(B * H * W, 3 * C, generator=g).to(DEV)
    b = (torch.randn(3 * C, generator=g) * 0.5).to(DEV) if bias else None
    table = (torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5).to(DEV)
    go = torch.randn(B * H * W, C, generator=g).to(DEV)
    return qkv, b, table, go


def _run_node(fn, geo, qkv, b, table, go):
    leaves = [t.detach().clone().requires_grad_(True) if t is not None else None for t in (qkv, b, table)]
    out = fn(leaves[0], leaves[1], leaves[2], geo)
    (out * go).sum().backward()
    return out.detach(), [t.grad if t is not None else None for t in leaves]


GEOMETRIES = [  # B, H, W, nH, ws, shift
    (1, 7, 7, 1, 7, 0), (2, 9, 11, 2, 7, 3), (1, 14, 14, 24, 12, 6), (4, 5, 13, 3, 12, 0), (2, 12, 24, 48, 12, 6),
    (3, 28, 28, 6, 12, 6), (2, 56, 56, 3, 7, 3), (1, 3, 17, 4, 7, 3), (2, 24, 12, 8, 12, 0), (1, 1, 1, 2, 12, 6),
    (2, 10, 6, 4, 5, 2),
]


@pytest.mark.parametrize("geo6", GEOMETRIES)
@pytest.mark.parametrize("bias", [True, False])
def test_node_matches_restatement(geo6, bias):
    B, H, W, nH, ws, s = geo6
    geo = (B, H, W, 32 * nH, nH, ws, s)
    args = _node_inputs(B, H, W, nH, ws, bias, seed=sum(geo6))
    fo, fg = _run_node(window_attention, geo, *args)
    ro, rg = _run_node(window_attention_reference, geo, *args)
    assert rel_err(fo.cpu().numpy(), ro.cpu().numpy()) < ACT
    gscale = rg[0].abs().max().item()
    for name, a, b in zip(("qkv", "bias", "table"), fg, rg):
        assert (a is None) == (args[1] is None and b is None)
        if a is None:
            continue
        if b is None:                                               # unpadded: the restatement never reads the bias
            assert torch.count_nonzero(a) == 0
            continue
        # (a bias gradient can be exactly the padded keys' masked-out e^-100 terms: denormals, flushed by the kernel)
        err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * gscale)
        assert err < GRAD, (name, err, a.abs().max().item())


def test_bias_and_table_gradients_of_a_padded_shifted_block():
    B, H, W, nH, ws, s = 2, 9, 10, 4, 7, 3                      # 14 x 14 padded, shifted: padded keys in most windows
    geo = (B, H, W, 32 * nH, nH, ws, s)
    qkv, b, table, go = _node_inputs(B, H, W, nH, ws, True, seed=5)
    _, (_, gb, gt) = _run_node(window_attention, geo, qkv, b, table, go)
    _, (_, rb, rt) = _run_node(window_attention_reference, geo, qkv, b, table, go)
    C = 32 * nH
    assert torch.count_nonzero(gb[:C]) == 0                     # q part: padded queries produce nothing
    assert gb[C:].abs().max() > 0
    assert rel_err(gb.cpu().numpy(), rb.cpu().numpy()) < GRAD
    assert rel_err(gt.cpu().numpy(), rt.cpu().numpy()) < GRAD
    # unpadded: the node adds nothing to the bias gradient
    geo = (B, 14, 14, 32 * nH, nH, ws, s)
    qkv, b, table, go = _node_inputs(B, 14, 14, nH, ws, True, seed=6)
    _, (_, gb, _) = _run_node(window_attention, geo, qkv, b, table, go)
    assert torch.count_nonzero(gb) == 0


def test_bitwise_reproducible():
    geo = (3, 14, 14, 768, 24, 12, 6)
    args = _node_inputs(3, 14, 14, 24, 12, seed=7)
    a_out, a_g = _run_node(window_attention, geo, *args)
    b_out, b_g = _run_node(window_attention, geo, *args)
    assert torch.equal(a_out, b_out)
    assert all(torch.equal(u, v) for u, v in zip(a_g, b_g))


def test_launch_counts():
    geo = (2, 9, 11, 64, 2, 7, 3)
    qkv, b, table, go = _node_inputs(2, 9, 11, 2, 7)
    leaves = [t.clone().requires_grad_(True) for t in (qkv, b, table)]
    n0 = _native.launch_count()
    out = window_attention(*leaves, geo)
    n1 = _native.launch_count()
    out.backward(go)
    n2 = _native.launch_count()
    assert (n1 - n0, n2 - n1) == (1, 3)


def _block(dim=192, heads=6, ws=12, shift=6, H=14, W=14, seed=0):
    torch.manual_seed(seed)
    blk = SwinTransformerBlock(dim, heads, ws, shift).to(DEV)
    blk.H, blk.W = H, W
    return blk


def test_no_host_sync():
    blk = _block()
    x = torch.randn(2, 14 * 14, 192, device=DEV, requires_grad=True)
    blk(x, OWN_SHIFT_MASK).sum().backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        blk(x, OWN_SHIFT_MASK).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_graph_capture():
    blk = _block(seed=3)
    x = torch.randn(2, 14 * 14, 192, device=DEV, requires_grad=True)
    w = torch.randn(2, 14 * 14, 192, device=DEV)

    def step():
        blk.zero_grad(set_to_none=True)
        x.grad = None
        (blk(x, OWN_SHIFT_MASK) * w).sum().backward()
        return [blk.attn.relative_position_bias_table.grad, blk.attn.qkv.bias.grad, x.grad]

    eager = [t.detach().clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    blk.zero_grad(set_to_none=True)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        (blk(x, OWN_SHIFT_MASK) * w).sum().backward()
    static = [blk.attn.relative_position_bias_table.grad, blk.attn.qkv.bias.grad, x.grad]
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(eager, static))


def _small_swin(use_checkpoint, dilation=False, drop_path_rate=0.3):
    torch.manual_seed(21)
    return SwinTransformer(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7,
                           drop_path_rate=drop_path_rate, out_indices=(1, 2, 3), dilation=dilation,
                           use_checkpoint=use_checkpoint).to(DEV)


def _swin_grads(m, img, mask, seed):
    torch.manual_seed(seed)
    x = img.clone().requires_grad_(True)
    outs = m(NestedTensor(x, mask))
    SI.weighted_sum([outs[k].tensors for k in sorted(outs)], 3).backward()
    return [outs[k].tensors.detach() for k in sorted(outs)], x.grad, {k: p.grad for k, p in m.named_parameters()}


def test_checkpointed_backbone_matches_plain_in_train_mode():
    img, mask = (t.to(DEV) for t in SI.backbone_input("swin_w7"))
    plain = _small_swin(False).train()
    ckpt = _small_swin(True).train()
    ckpt.load_state_dict(plain.state_dict())
    a_out, a_x, a_p = _swin_grads(plain, img, mask, 5)
    b_out, b_x, b_p = _swin_grads(ckpt, img, mask, 5)
    assert all(torch.equal(u, v) for u, v in zip(a_out, b_out))
    assert rel_err(b_x.cpu().numpy(), a_x.cpu().numpy()) < 1e-6
    for k in a_p:
        assert rel_err(b_p[k].cpu().numpy(), a_p[k].cpu().numpy()) < 1e-6, k


def test_autocast_takes_the_composition(monkeypatch):
    blk = _block(seed=4)
    x = torch.randn(2, 14 * 14, 192, device=DEV)
    mask = shift_mask(14, 14, 12, 6, DEV)
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MSDA_SWIN_FUSED", fused)
        n0 = _native.launch_count()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = blk(x, OWN_SHIFT_MASK if fused == "1" else mask)
        assert _native.launch_count() == n0
        res.append(y)
    assert res[0].dtype == res[1].dtype and torch.equal(res[0], res[1])


def test_dilation_last_stage_falls_back(monkeypatch):
    img, mask = (t.to(DEV) for t in SI.backbone_input("swin_w7"))
    m = _small_swin(False, dilation=True, drop_path_rate=0.0).eval()
    twin = copy.deepcopy(m)
    assert m.layers[-1].blocks[0].attn.dim // m.layers[-1].blocks[0].attn.num_heads == 16
    monkeypatch.setenv("MSDA_SWIN_FUSED", "1")
    n0 = _native.launch_count()
    a_out, a_x, a_p = _swin_grads(m, img, mask, 1)
    assert _native.launch_count() - n0 == 4 * (2 + 2 + 2)         # stages 0-2 (head_dim 32): 1 + 3 launches per block
    monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
    n0 = _native.launch_count()
    b_out, b_x, b_p = _swin_grads(twin, img, mask, 1)
    assert _native.launch_count() == n0
    for u, v in zip(a_out, b_out):
        assert rel_err(u.cpu().numpy(), v.cpu().numpy()) < 1e-4
    assert rel_err(a_x.cpu().numpy(), b_x.cpu().numpy()) < 1e-3
    for k in a_p:
        assert rel_err(a_p[k].cpu().numpy(), b_p[k].cpu().numpy()) < 1e-3, k


def test_arctic_detr_over_the_dropin_joiner():
    from uvhand_amd.modules import ArcticDeformableDETR, DeformableTransformer
    torch.manual_seed(0)
    body = SwinTransformer(embed_dim=192, depths=[2, 2, 2, 2], num_heads=[6, 12, 24, 48], window_size=7,
                           out_indices=(1, 2, 3), drop_path_rate=0.2, use_checkpoint=True)
    backbone = Joiner(body, PositionEmbeddingSine(128, normalize=True))
    tr = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=2, dim_feedforward=512,
                               dropout=0.0, return_intermediate_dec=True, num_feature_levels=4, two_stage=True,
                               two_stage_num_proposals=20)
    model = ArcticDeformableDETR(backbone, tr, 14, 20, 4, with_box_refine=True, two_stage=True,
                                 feature_type='origin').to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    samples = NestedTensor(torch.randn(2, 3, 64, 80, generator=g).to(DEV), torch.zeros(2, 64, 80, dtype=torch.bool, device=DEV))
    n0 = _native.launch_count()
    out = model(samples)
    loss = sum(v.float().sum() for v in out.values() if torch.is_tensor(v))
    loss.backward()
    assert _native.launch_count() - n0 >= 8 * 4                                  # every block: 1 forward + 3 backward
    grads = [p.grad for p in body.parameters()]
    assert all(g is not None for g in grads)
    assert all(torch.isfinite(g).all() for g in grads)


def test_window_attention_module_on_partitioned_windows(monkeypatch):
    from uvhand_amd.modules import WindowAttention
    torch.manual_seed(8)
    wa = WindowAttention(96, (7, 7), 3).to(DEV)
    x = torch.randn(5, 49, 96, device=DEV)
    mask = torch.where(torch.rand(5, 49, 49, device=DEV) > 0.8, -100.0, 0.0)
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MSDA_SWIN_FUSED", fused)
        wa.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        n0 = _native.launch_count()
        y = wa(xx)
        assert _native.launch_count() - n0 == (1 if fused == "1" else 0)
        n0 = _native.launch_count()
        assert torch.equal(wa(xx, mask), wa(xx, mask)) and _native.launch_count() == n0      # a mask: the composition
        (y * x).sum().backward()
        res.append((y.detach(), xx.grad, [p.grad for p in wa.parameters()]))
    (a, ax, ap), (b, bx, bp) = res
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < ACT
    assert rel_err(ax.cpu().numpy(), bx.cpu().numpy()) < GRAD
    for u, v in zip(ap, bp):
        assert rel_err(u.cpu().numpy(), v.cpu().numpy()) < GRAD
