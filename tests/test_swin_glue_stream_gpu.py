"""The Swin glue over a bf16 residual stream (csrc/msda_swin_glue.hip, msda_swin_glue_*_sbf16; MSDA_SWIN_GLUE=1 with
MSDA_SWIN_GLUE_BF16=1 under bf16 autocast): norm, add + norm, add and merge + norm on bf16 rows against torch's own bf16 autocast
arithmetic (bit for bit where the issue is an add) and against float64, the rounding points, the route a block and a backbone
take with the knob on and off, drop-path parity, checkpointing, reproducibility, host syncs and graph capture.

Shapes are those of tests/test_swin_glue_gpu.py.  Error measure and acceptance rule are those of tests/test_swin_bf16_gpu.py:
max|a - b| / (max|b| + 0.1) against a float64 restatement on the same bf16 inputs, accepted up to max(floor, 2 x the error of
torch's composition on the GPU on the same inputs); floors ACT = 1e-2 for bf16 activations, GRAD = 2e-2 for bf16 gradients, 1e-5
for fp32 outputs and parameter gradients.  The float64 restatement of add + norm normalises the bf16 y (the contract of
include/msda.h, pinned on the CPU by tests/test_swin_glue_stream_abi.py), not the unrounded sum.

Rounding points: the share of z (and of add + norm's grad_x) elements whose bits differ from the composition's is at most 1 %.
Two correct fp32 LayerNorms flip between 0 and 1e-4 of the bf16 results at these widths (CPU); normalising the unrounded sum
flips 23 to 32 %, one rounding of grad_x instead of two 23 %: the cap is a factor of 100 above the first and 20 below the others."""
import copy
import sys

import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import swin_inputs as SI  # noqa: E402
from test_swin_bf16_gpu import ACT, GRAD, _BLOCK_GRADS, _accept, _block, _block_step, _rel  # noqa: E402
from test_swin_glue_gpu import (DEV, EPS, F32, MERGES, SAMPLES, WIDTHS, _backbone_run, _drop_block, _inputs,  # noqa: E402
                                _merge_reference, _norm_module, _run)
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.swin_glue_func import add_norm_rows, add_rows, merge_norm, norm_rows  # noqa: E402
from uvhand_amd.modules import BasicLayer, PatchMerging  # noqa: E402
from uvhand_amd.modules.swin import OWN_SHIFT_MASK  # noqa: E402

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FLIPS = 1e-2


@pytest.fixture(autouse=True)
def _knobs_on(monkeypatch):
    monkeypatch.setenv("MSDA_SWIN_GLUE", "1")
    monkeypatch.setenv("MSDA_SWIN_GLUE_BF16", "1")
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    monkeypatch.delenv("MSDA_SWIN_FUSED", raising=False)


def _amp():
    return torch.autocast("cuda", dtype=BF16)


def _keeps(B, seed):
    """None; 0 and 2 with at least one zero (exact products); bf16(1 / 0.7) with one zero (the product rounds)."""
    g = torch.Generator().manual_seed(seed)
    two = (torch.rand(B, generator=g) < 0.5).float() * 2
    two[seed % B] = 0
    frac = torch.full((B,), 1 / 0.7)
    frac[(seed + 1) % B] = 0
    return [None, two.to(BF16).view(B, 1, 1), frac.to(BF16).view(B, 1, 1)]


def _bf16_inputs(B, L, C, seed):
    x, a, gy, gz, w, b = _inputs(B, L, C, BF16, seed)
    return x.to(BF16), a, gy.to(BF16), gz, w, b


def _flips(a, b):
    """(elements whose bits differ, elements)."""
    assert a.dtype == b.dtype == BF16 and a.shape == b.shape
    return int((a.view(torch.int16) != b.view(torch.int16)).sum().item()), a.numel()


@pytest.mark.parametrize("C", WIDTHS)
def test_add_is_torchs_bit_for_bit(C):
    for i, (B, L) in enumerate(SAMPLES):
        x, a, gy, _, _, _ = _bf16_inputs(B, L, C, 100 + C + i)
        for keep in _keeps(B, i):
            k = keep.to(DEV) if keep is not None else None
            n0 = _native.launch_count()
            with _amp():
                (y,), (gx, ga), _ = _run(lambda u, v: add_rows(u, v, k), [x.to(DEV), a.to(DEV)], [gy], None)
            launches = _native.launch_count() - n0
            assert launches == (1 if keep is None else 2), launches               # without keep grad_a is grad_y: no launch
            with _amp():
                (ty,), (tgx, tga), _ = _run(lambda u, v: u + (v if k is None else v * k), [x.to(DEV), a.to(DEV)], [gy], None)
            assert y.dtype == gx.dtype == ga.dtype == ty.dtype == BF16
            assert torch.equal(y, ty) and torch.equal(gx, tgx) and torch.equal(ga, tga), (B, L, keep)
            if keep is not None:
                dropped = (keep.view(-1) == 0).to(DEV)
                assert torch.equal(y[dropped], x.to(DEV)[dropped]) and torch.count_nonzero(ga[dropped]) == 0


def _add_norm_composition(norm, k):
    """What the block runs under bf16 autocast on a bf16 stream; z as the consuming Linear casts it."""
    def fn(u, v):
        y = u + (v if k is None else v * k)
        return y, norm(y).to(BF16)
    return fn


def _add_norm_fp64(n64, k64, y_bf16):
    """The float64 restatement: the value of y is the bf16 y, its gradient passes to x and a as through the exact sum."""
    def fn(u, v):
        y = u + (v if k64 is None else v * k64)
        y = y + (y_bf16.double() - y).detach()
        return y, n64(y)
    return fn


@pytest.mark.parametrize("C", WIDTHS)
def test_add_norm_matches_torch_and_fp64(C):
    for i, (B, L) in enumerate(SAMPLES):
        x, a, gy, gz, w, b = _bf16_inputs(B, L, C, 200 + C + i)
        for keep in _keeps(B, i + 1):
            k = keep.to(DEV) if keep is not None else None
            norm = _norm_module(w, b, DEV)
            n0 = _native.launch_count()
            with _amp():
                (y, z), (gx, ga), (gw, gb) = _run(lambda u, v: add_norm_rows(u, v, k, norm), [x.to(DEV), a.to(DEV)], [gy, gz], norm)
            assert _native.launch_count() - n0 == 3                          # one forward, the rows' pass and the reduction
            assert y.dtype == z.dtype == gx.dtype == ga.dtype == BF16 and gw.dtype == gb.dtype == torch.float32
            with _amp():
                (cy, cz), (cgx, cga), (cgw, cgb) = _run(_add_norm_composition(norm, k), [x.to(DEV), a.to(DEV)], [gy, gz], norm)
            assert cy.dtype == BF16 and torch.equal(y, cy), (B, L, keep)
            if keep is None:
                assert torch.equal(ga, gx)
            n64 = _norm_module(w, b, "cpu", torch.float64)
            k64 = keep.double() if keep is not None else None
            (ry, rz), (rgx, rga), (rgw, rgb) = _run(_add_norm_fp64(n64, k64, cy.cpu()), [x.double(), a.double()], [gy, gz], n64)
            assert torch.equal(ry, cy.cpu().double())
            tag = "add_norm C=%d B=%d L=%d keep=%s " % (C, B, L, None if keep is None else keep.view(-1)[:2].tolist())
            _accept(tag + "z", _rel(z, rz), _rel(cz, rz), ACT)
            _accept(tag + "grad_x", _rel(gx, rgx), _rel(cgx, rgx), GRAD)
            _accept(tag + "grad_a", _rel(ga, rga), _rel(cga, rga), GRAD)
            _accept(tag + "grad_gamma", _rel(gw, rgw), _rel(cgw, rgw), F32)
            _accept(tag + "grad_beta", _rel(gb, rgb), _rel(cgb, rgb), F32)
            if keep is not None:
                assert torch.count_nonzero(ga[(keep.view(-1) == 0).to(DEV)]) == 0


@pytest.mark.parametrize("C", WIDTHS)
def test_rounding_points_are_torchs(C):
    """Pooled over SAMPLES: z and add + norm's grad_x differ from the composition's bits in at most 1 % of the elements."""
    zf = gf = total = 0
    for i, (B, L) in enumerate(SAMPLES):
        x, a, gy, gz, w, b = _bf16_inputs(B, L, C, 600 + C + i)
        k = _keeps(B, i + 2)[2].to(DEV)
        norm = _norm_module(w, b, DEV)
        with _amp():
            (y, z), (gx, _), _ = _run(lambda u, v: add_norm_rows(u, v, k, norm), [x.to(DEV), a.to(DEV)], [gy, gz], norm)
            (cy, cz), (cgx, _), _ = _run(_add_norm_composition(norm, k), [x.to(DEV), a.to(DEV)], [gy, gz], norm)
        assert torch.equal(y, cy)
        zf += _flips(z, cz)[0]
        gf += _flips(gx, cgx)[0]
        total += z.numel()
    print("rounding points C=%d: z %d of %d differ (%.3e), grad_x %d of %d (%.3e), cap %.0e"
          % (C, zf, total, zf / total, gf, total, gf / total, FLIPS))
    assert zf <= FLIPS * total and gf <= FLIPS * total


@pytest.mark.parametrize("C", WIDTHS)
def test_norm_matches_fp64(C):
    for i, (B, L) in enumerate(SAMPLES):
        x, _, _, gz, w, b = _bf16_inputs(B, L, C, 300 + C + i)
        norm = _norm_module(w, b, DEV)
        n0 = _native.launch_count()
        with _amp():
            (z,), (gx,), (gw, gb) = _run(lambda u: norm_rows(u, norm), [x.to(DEV)], [gz], norm)
            (z32,), (gx32,), (gw32, gb32) = _run(lambda u: norm_rows(u, norm, fp32_out=True), [x.to(DEV)], [gz], norm)
        assert _native.launch_count() - n0 == 2 * 3
        assert z.dtype == gx.dtype == gx32.dtype == BF16 and z32.dtype == torch.float32
        with _amp():
            (cz,), (cgx,), (cgw, cgb) = _run(lambda u: norm(u).to(BF16), [x.to(DEV)], [gz], norm)
            (cz32,), (cgx32,), (cgw32, cgb32) = _run(lambda u: norm(u), [x.to(DEV)], [gz], norm)
        assert cz32.dtype == torch.float32 and cgx.dtype == BF16
        n64 = _norm_module(w, b, "cpu", torch.float64)
        (rz,), (rgx,), (rgw, rgb) = _run(lambda u: n64(u), [x.double()], [gz], n64)
        tag = "norm C=%d B=%d L=%d " % (C, B, L)
        _accept(tag + "z", _rel(z, rz), _rel(cz, rz), ACT)
        _accept(tag + "z fp32", _rel(z32, rz), _rel(cz32, rz), F32)
        for sub, got, comp in (("", (gx, gw, gb), (cgx, cgw, cgb)), (" (fp32 out)", (gx32, gw32, gb32), (cgx32, cgw32, cgb32))):
            _accept(tag + "grad_x" + sub, _rel(got[0], rgx), _rel(comp[0], rgx), GRAD)
            _accept(tag + "grad_gamma" + sub, _rel(got[1], rgw), _rel(comp[1], rgw), F32)
            _accept(tag + "grad_beta" + sub, _rel(got[2], rgb), _rel(comp[2], rgb), F32)


@pytest.mark.parametrize("bhw,C", MERGES)
def test_merge_norm_matches_fp64(bhw, C):
    B, H, W = bhw
    g = torch.Generator().manual_seed(400 + C + H)
    x = (torch.randn(B, H * W, C, generator=g) * 1.5 + 0.3).to(BF16)
    L2 = (H + 1) // 2 * ((W + 1) // 2)
    gz = torch.randn(B, L2, 4 * C, generator=g).to(BF16)
    w, b = torch.randn(4 * C, generator=g) * 0.5 + 1, torch.randn(4 * C, generator=g) * 0.5
    norm = _norm_module(w, b, DEV)
    n0 = _native.launch_count()
    with _amp():
        (z,), (gx,), (gw, gb) = _run(lambda u: merge_norm(u, H, W, norm), [x.to(DEV)], [gz], norm)
    assert _native.launch_count() - n0 == 3
    assert z.dtype == BF16 and tuple(z.shape) == (B, L2, 4 * C)
    assert gx.dtype == BF16 and gx.shape == x.shape
    with _amp():
        (cz,), (cgx,), (cgw, cgb) = _run(lambda u: _merge_reference(u, H, W, norm, BF16), [x.to(DEV)], [gz], norm)
    n64 = _norm_module(w, b, "cpu", torch.float64)
    (rz,), (rgx,), (rgw, rgb) = _run(lambda u: _merge_reference(u, H, W, n64), [x.double()], [gz], n64)
    tag = "merge_norm %s C=%d " % (bhw, C)
    _accept(tag + "z", _rel(z, rz), _rel(cz, rz), ACT)
    _accept(tag + "grad_x", _rel(gx, rgx), _rel(cgx, rgx), GRAD)
    _accept(tag + "grad_gamma", _rel(gw, rgw), _rel(cgw, rgw), F32)
    _accept(tag + "grad_beta", _rel(gb, rgb), _rel(cgb, rgb), F32)
    # every real token has a gradient (random data: an exact zero means an element nobody wrote or a leak from a pad position)
    assert torch.count_nonzero(gx) == gx.numel() and torch.isfinite(gx.float()).all()
    assert torch.equal(gx == 0, rgx.to(DEV) == 0)
    # a pad position reads zero: the merged rows that hold one are, per row, what the fp64 reference gives with zeros there
    if H % 2 or W % 2:
        padded = torch.zeros(B, (H + 1) // 2, (W + 1) // 2, dtype=torch.bool)
        if H % 2:
            padded[:, -1, :] = True
        if W % 2:
            padded[:, :, -1] = True
        rows = padded.view(B, L2)
        assert rows.any()
        _accept(tag + "z of the rows with a pad position", _rel(z.cpu()[rows], rz[rows]), _rel(cz.cpu()[rows], rz[rows]), ACT)


# ---- a block -------------------------------------------------------------------------------------------------------------
def test_block_route(monkeypatch):
    """Fails without the bf16-stream kernels: there a bf16 x keeps torch's glue and the counts stay (1, 3)."""
    blk = _block(seed=4)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 14 * 14, 192, generator=g).to(DEV).to(BF16)
    w = torch.randn(2, 14 * 14, 192, generator=g).to(DEV)
    y, nf, nb, grads, node_dtype = _block_step(blk, x, w, BF16)
    assert (nf, nb) == (4, 7)                          # attention 1 + 3 glue; attention 3, add + norm 2, norm 2, add none
    assert y.dtype == BF16 and grads[0].dtype == BF16 and node_dtype == BF16
    drop = _drop_block(2)
    torch.manual_seed(9)
    d_y, df, db, _, _ = _block_step(drop, x, w, BF16)
    assert (df, db) == (4, 8) and d_y.dtype == BF16    # in training with drop-path add's grad_a is a launch
    for value in (None, "0"):                          # the new knob unset or off: today's counts
        if value is None:
            monkeypatch.delenv("MSDA_SWIN_GLUE_BF16")
        else:
            monkeypatch.setenv("MSDA_SWIN_GLUE_BF16", value)
        o_y, of, ob, _, _ = _block_step(blk, x, w, BF16)
        assert (of, ob) == (1, 3) and o_y.dtype == BF16
    monkeypatch.setenv("MSDA_SWIN_GLUE_BF16", "1")
    monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
    c_y, cf, cb, c_grads, _ = _block_step(blk, x, w, BF16)
    assert (cf, cb) == (0, 0)
    ref = copy.deepcopy(blk).cpu().double()
    xr = x.cpu().double().requires_grad_(True)
    r_y = ref(xr, OWN_SHIFT_MASK)
    (r_y * w.cpu().double()).sum().backward()
    rp = dict(ref.named_parameters())
    r_grads = [xr.grad] + [rp[k].grad for k in _BLOCK_GRADS]
    _accept("y", _rel(y, r_y), _rel(c_y, r_y), ACT)
    for name, a, c, r in zip(("x",) + _BLOCK_GRADS, grads, c_grads, r_grads):
        _accept("grad " + name, _rel(a, r), _rel(c, r), GRAD)


def test_drop_path_parity(monkeypatch):
    B = 8
    blk = _drop_block(B)
    x = torch.randn(B, 14 * 14, 192, generator=torch.Generator().manual_seed(21)).to(DEV).to(BF16)
    res = []
    for knob in ("1", "0"):
        monkeypatch.setenv("MSDA_SWIN_GLUE_BF16", knob)
        torch.manual_seed(77)
        n0 = _native.launch_count()
        with _amp():
            y = blk(x, OWN_SHIFT_MASK)
        res.append((y.detach(), torch.cuda.get_rng_state(DEV), _native.launch_count() - n0))
    (y1, rng1, n1), (y0, rng0, n0) = res
    assert (n1, n0) == (4, 1) and y1.dtype == y0.dtype == BF16
    assert torch.equal(rng1, rng0)                                             # the Philox stream consumed alike
    same1 = (y1 == x).flatten(1).all(1)
    same0 = (y0 == x).flatten(1).all(1)
    assert torch.equal(same1, same0)                                           # the same samples dropped in both branches
    y1, y0 = y1.float(), y0.float()
    per_sample = (y1 - y0).abs().flatten(1).amax(1) / (y0.abs().flatten(1).amax(1) + 0.1)
    print("drop-path parity: dropped", same1.tolist(), "per-sample difference", per_sample.tolist())
    assert per_sample.max().item() < 5e-2


def test_checkpointed_layer_is_bit_identical():
    depth, H, W = 2, 9, 11

    def layer(use_checkpoint):
        torch.manual_seed(31)
        return BasicLayer(64, depth, 2, window_size=7, drop_path=0.2, downsample=PatchMerging,
                          use_checkpoint=use_checkpoint).to(DEV).train()
    plain, ckpt = layer(False), layer(True)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(4, H * W, 64, generator=g).to(DEV).to(BF16)
    w = torch.randn(4, H * W, 64, generator=g).to(DEV)
    res = []
    for m in (plain, ckpt):
        m.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        torch.manual_seed(5)
        n0 = _native.launch_count()
        with _amp():
            out = m(xx, H, W)
        assert out[0].dtype == out[3].dtype == BF16
        ((out[0].float() * w).sum() + out[3].float().sum()).backward()
        res.append((_native.launch_count() - n0, out[0].detach(), out[3].detach(), xx.grad, [p.grad for p in m.parameters()]))
    (na, ya, da, xa, pa), (nb, yb, db, xb, pb) = res
    # plain: per block 4 forward and 8 backward (7 where the keep vector is None), and the merging's 1 + 2
    assert nb == na + depth * 4                                                # the blocks' forward once more
    assert xa.dtype == BF16
    assert torch.equal(ya, yb) and torch.equal(da, db) and torch.equal(xa, xb)
    assert all(torch.equal(u, v) for u, v in zip(pa, pb))


_NODES = (3, 15, 96, 3, 5)                 # B, L, C and the merge's H x W = L


def _node_inputs():
    B, L, C, _, _ = _NODES
    x, a, gy, gz, w, b = _bf16_inputs(B, L, C, 500)
    keep = _keeps(B, 1)[2].view(-1)
    return [t.to(DEV) for t in (x, a, gy, gz, w, b, keep)]


def _all_nodes(x, a, gy, gz, w, b, keep):
    """Every _sbf16 entry once through the binding, on device tensors: forward and backward results of the four operations."""
    B, L, C, H, W = _NODES
    out = []
    for T in (BF16, torch.float32):
        z, mean, rstd = _native.swin_glue_norm_forward(x, w, b, EPS, T)
        out += [z, mean, rstd, *_native.swin_glue_norm_backward(gz.to(T), x, w, mean, rstd)]
    for k in (keep, None):
        y, z, mean, rstd = _native.swin_glue_add_norm_forward(x, a, k, L, w, b, EPS)
        out += [y, z, mean, rstd, *_native.swin_glue_add_norm_backward(gy, gz, y, k, L, w, mean, rstd)]
        out += [_native.swin_glue_add_forward(x, a, k, L)]
    out += [_native.swin_glue_add_backward(gy, keep, L, BF16)]
    w4, b4 = torch.cat([w] * 4), torch.cat([b] * 4)
    x4 = x.view(B, H, W, C)
    z, mean, rstd = _native.swin_glue_merge_norm_forward(x4, w4, b4, EPS, BF16)
    gz4 = torch.cat([gz[:, :6]] * 4, -1).contiguous()
    out += [z, mean, rstd, *_native.swin_glue_merge_norm_backward(gz4, x4, w4, mean, rstd)]
    assert all(t.dtype in (BF16, torch.float32) for t in out)
    return out


def test_every_entry_is_reached():
    """The ten entries of the bf16 stream are what _all_nodes launches: 4 + 4 norm, 2 x (1 + 2 + 1), 1, 1 + 2 launches."""
    args = _node_inputs()
    n0 = _native.launch_count()
    out = _all_nodes(*args)
    assert _native.launch_count() - n0 == 2 * 3 + 2 * 4 + 1 + 3
    assert out[0].dtype == BF16 and out[6].dtype == torch.float32            # z of the two norm forms
    assert out[3].dtype == out[9].dtype == BF16                              # grad_x of either is the stream's type


def test_bitwise_reproducible():
    args = _node_inputs()
    a, b = _all_nodes(*args), _all_nodes(*args)
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def test_graph_capture():
    args = _node_inputs()
    eager = [t.clone() for t in _all_nodes(*args)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _all_nodes(*args)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _all_nodes(*args)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(eager, static))


def test_no_host_sync():
    blk = _drop_block(4)
    x = torch.randn(4, 14 * 14, 192, device=DEV).to(BF16).requires_grad_(True)

    def step():
        with _amp():
            y = blk(x, OWN_SHIFT_MASK)
        y.float().sum().backward()
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
@pytest.mark.parametrize("name", list(SI.BACKBONE_CASES))
def test_backbone_fixture(name, monkeypatch):
    """Fails without the bf16-stream kernels (the count stays that of stage 0).  The goldens are fp32 results of the
    reference's code; the same route without the new knob is the comparison."""
    z = load_golden(name)
    depths = SI.BACKBONE_CASES[name]["depths"]
    launches, errs = _backbone_run(name, z, BF16)
    assert launches == 4 * sum(depths) + 3 + 3         # the fp32 glue's count: every block, patch merging and output norm
    monkeypatch.delenv("MSDA_SWIN_GLUE_BF16")
    o_launches, o_errs = _backbone_run(name, z, BF16)
    assert o_launches == sum(depths) + 3 * depths[0] + 1
    assert sorted(errs) == sorted(o_errs)
    for key in errs:
        _accept(key, errs[key], o_errs[key], ACT if key.startswith("out") else GRAD)
