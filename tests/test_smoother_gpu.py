"""SmoothNet MotionSmoothers on the HIP kernels (csrc/msda_smoother.hip) against the reference's fixtures, the torch
restatement and, in train mode, the torch composition with the kernels' own dropout masks."""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import smoother_inputs as SI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.arctic_item import get_arctic_item, perturb_arctic_item  # noqa: E402
from uvhand_amd.functions.smoother_func import motion_smoothers  # noqa: E402
from uvhand_amd.modules import ArcticSmoother, MotionSmoother  # noqa: E402

pytestmark = pytest.mark.gpu

ACT, GRAD = 2e-5, 1e-4           # fp32 MFMA against the CPU: as tests/test_detr_gpu.py
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name", list(SI.SMALL_CASES))
def test_fixture_outputs_and_gradients(name):
    z = load_golden("smoother_small")
    m = SI.build_motion(MotionSmoother, name).to(DEV)
    x = torch.from_numpy(z[name + "/x"]).to(DEV).requires_grad_(True)
    n0 = _native.launch_count()
    y = m(x)
    assert _native.launch_count() - n0 == 2 * m.num_blocks + 3
    SI.weighted_sum([y], 7).backward()
    assert rel_err(y.detach().cpu().numpy(), z[name + "/out"]) < ACT
    assert rel_err(x.grad.cpu().numpy(), z[name + "/grad_x"]) < GRAD
    for k, p in m.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), z["%s/grad/%s" % (name, k)]) < GRAD, k


def _both_routes(mods, xs, monkeypatch, seed=3):
    """eval-mode outputs and gradients (inputs and parameters) of the fused route and of MSDA_SMOOTHER_FUSED=0; call i runs
    module i % 2."""
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MSDA_SMOOTHER_FUSED", fused)
        for m in mods:
            m.zero_grad(set_to_none=True)
        leaves = [x.detach().clone().requires_grad_(True) for x in xs]
        outs = motion_smoothers([(i % 2, x) for i, x in enumerate(leaves)], mods, False)
        SI.weighted_sum(outs, seed).backward()
        res.append(([o.detach() for o in outs], [x.grad for x in leaves], [p.grad.clone() for m in mods for p in m.parameters()]))
    return res


@pytest.mark.parametrize("T,B,C", [(3, 2, 5), (8, 1, 1), (32, 3, 23), (64, 2, 40)])
def test_matches_restatement(T, B, C, monkeypatch):
    torch.manual_seed(T)
    mods = [MotionSmoother(T, T, 64, 32, 2).to(DEV).eval(), MotionSmoother(T, T, 64, 32, 2).to(DEV).eval()]
    xs = [torch.randn(B, T, C, device=DEV) for _ in range(3)]                 # calls 0, 2 share module 0
    (fo, fx, fp), (ro, rx, rp) = _both_routes(mods, xs, monkeypatch)
    for a, b in zip(fo, ro):
        assert rel_err(a.cpu().numpy(), b.contiguous().cpu().numpy()) < ACT
    for a, b in zip(fx + fp, rx + rp):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < GRAD


def test_arctic_fixture():
    z = load_golden("smoother_arctic")
    a = SI.build_arctic(ArcticSmoother).to(DEV)
    xs = [torch.from_numpy(z["x%d" % i]).to(DEV).requires_grad_(True) for i in range(9)]
    ys = SI.flatten(a(SI.structure(xs)))
    SI.weighted_sum(ys, 8).backward()
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert rel_err(y.detach().cpu().numpy(), z["out%d" % i]) < ACT, i
        assert rel_err(x.grad.cpu().numpy(), z["grad_x%d" % i]) < GRAD, i


def _arctic_step(a, xs):
    ys = SI.flatten(a(SI.structure(xs)))
    loss = sum((y * (0.5 + 0.25 * i)).sum() for i, y in enumerate(ys))           # no host tensors: capturable
    return ys, torch.autograd.grad(loss, [x for x in xs if x.requires_grad] + list(a.parameters()))


@pytest.mark.parametrize("B", [1, 8])
def test_launch_counts(B):
    torch.manual_seed(0)
    a = ArcticSmoother(B, 32).to(DEV).train()
    xs = [t.to(DEV) for t in SI.arctic_inputs(B=B)]
    for want_x in (False, True):
        leaves = [x.clone().requires_grad_(want_x) for x in xs]
        n0 = _native.launch_count()
        ys = SI.flatten(a(SI.structure(leaves)))
        n1 = _native.launch_count()
        loss = sum(y.sum() for y in ys)
        n2 = _native.launch_count()
        loss.backward()
        n3 = _native.launch_count()
        assert n1 - n0 == 9
        assert n3 - n2 <= 11
        assert n3 - n2 == (11 if want_x else 9)


def test_whole_module_matches_composition(monkeypatch):
    torch.manual_seed(4)
    a = ArcticSmoother(2, 32).to(DEV).eval()
    xs = [t.to(DEV) for t in SI.arctic_inputs(B=2)]
    res = []
    for fused in ("1", "0"):
        monkeypatch.setenv("MSDA_SMOOTHER_FUSED", fused)
        leaves = [x.clone().requires_grad_(True) for x in xs]
        ys, grads = _arctic_step(a, leaves)
        res.append(([y.detach() for y in ys], grads))
    for u, v in zip(res[0][0], res[1][0]):
        assert rel_err(u.cpu().numpy(), v.cpu().numpy()) < ACT
    for u, v in zip(res[0][1], res[1][1]):
        assert rel_err(u.cpu().numpy(), v.cpu().numpy()) < GRAD


# ---- train mode --------------------------------------------------------------------------------------------------------------
def _masked_composition(m, x, masks, p):
    """MotionSmoother.forward with dropout = multiplication by masks[(s, layer)] / (1 - p) (rows b * C + c)."""
    B, T, C = x.shape
    xp = x.permute(0, 2, 1)
    vel = xp[..., 1:] - xp[..., :-1]
    acc = vel[..., 1:] - vel[..., :-1]
    outs = []
    for s, (sm, inp) in enumerate(zip((m.pos_smoother, m.vel_smoother, m.acc_smoother), (xp, vel, acc))):
        h = F.leaky_relu(sm.encoder[0](inp), 0.1)
        for j, blk in enumerate(sm.res_blocks, start=1):
            mk1 = masks[(s, 2 * j - 1)].view(B, C, -1)
            mk2 = masks[(s, 2 * j)].view(B, C, -1)
            u = F.leaky_relu(blk.linear1(h) * mk1 * (1.0 / (1.0 - p)), 0.2)
            h = F.leaky_relu(blk.linear2(u) * mk2 * (1.0 / (1.0 - p)), 0.2) + h
        outs.append(sm.decoder(h))
    return m.fusion_layer(torch.cat(outs, dim=2)).permute(0, 2, 1)


def test_train_mode_matches_masked_composition():
    torch.manual_seed(7)
    m = MotionSmoother(16, 16, 64, 32, 2, dropout=0.7).to(DEV).train()
    x = torch.randn(3, 16, 21, device=DEV, requires_grad=True)
    torch.cuda.manual_seed(1234)
    y = m(x)
    w = torch.randn_like(y)
    gx, *gp = torch.autograd.grad((y * w).sum(), [x] + list(m.parameters()))
    torch.cuda.manual_seed(1234)
    seed = torch.empty((), dtype=torch.int64, device=DEV).random_().view(1)
    rows = 3 * 21
    masks = {(s, l): _native.smoother_dropout_mask(seed, s, l, rows, 32 if l % 2 else 64, 0.7)
             for s in range(3) for l in range(1, 5)}
    assert 0 < masks[(0, 1)].mean().item() < 1
    y2 = _masked_composition(m, x, masks, 0.7)
    gx2, *gp2 = torch.autograd.grad((y2 * w).sum(), [x] + list(m.parameters()))
    assert rel_err(y.detach().cpu().numpy(), y2.detach().cpu().numpy()) < ACT
    assert rel_err(gx.cpu().numpy(), gx2.cpu().numpy()) < GRAD
    for a, b in zip(gp, gp2):
        assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < GRAD


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def test_keep_rate():
    mask = _native.smoother_dropout_mask(_seed(-8312745), 4, 3, 1024, 1024, 0.9)
    rate = mask.mean().item()
    sigma = (0.1 * 0.9 / mask.numel()) ** 0.5
    assert abs(rate - 0.1) < 5 * sigma


def _corr(a, b):
    a = a.flatten().double() - a.double().mean()
    b = b.flatten().double() - b.double().mean()
    return (a @ b / (a.norm() * b.norm())).item()


def test_masks_uncorrelated_and_reproducible():
    n = 512 * 512
    bound = 5.0 / n ** 0.5
    base = _native.smoother_dropout_mask(_seed(12345), 0, 1, 512, 512, 0.9)
    assert torch.equal(base, _native.smoother_dropout_mask(_seed(12345), 0, 1, 512, 512, 0.9))
    for other in (_native.smoother_dropout_mask(_seed(12346), 0, 1, 512, 512, 0.9),     # next seed
                  _native.smoother_dropout_mask(_seed(12345 + (1 << 32)), 0, 1, 512, 512, 0.9),   # high seed bits
                  _native.smoother_dropout_mask(_seed(12345), 0, 2, 512, 512, 0.9),     # other layer
                  _native.smoother_dropout_mask(_seed(12345), 1, 1, 512, 512, 0.9),     # other problem
                  _native.smoother_dropout_mask(_seed(12345), 3, 1, 512, 512, 0.9)):    # other module
        assert abs(_corr(base, other)) < bound
    # neighbouring rows / columns of one mask
    assert abs(_corr(base[1:], base[:-1])) < bound * 1.01
    assert abs(_corr(base[:, 1:], base[:, :-1])) < bound * 1.01


def test_train_mode_reproducible_under_manual_seed():
    torch.manual_seed(2)
    a = ArcticSmoother(1, 32).to(DEV).train()
    xs = [t.to(DEV) for t in SI.arctic_inputs()]
    runs = []
    for _ in range(2):
        torch.manual_seed(99)
        ys, grads = _arctic_step(a, xs)
        runs.append([y.detach() for y in ys] + list(grads))
    assert all(torch.equal(u, v) for u, v in zip(*runs))
    ys3, _ = _arctic_step(a, xs)                                            # a fresh draw: other masks
    assert not all(torch.equal(u, v) for u, v in zip(runs[0][:9], ys3))


def test_bitwise_reproducible_eval():
    torch.manual_seed(3)
    a = ArcticSmoother(8, 32).to(DEV).eval()
    xs = [t.to(DEV).requires_grad_(True) for t in SI.arctic_inputs(B=8)]
    r1 = _arctic_step(a, xs)
    r2 = _arctic_step(a, xs)
    assert all(torch.equal(u, v) for u, v in zip(list(r1[0]) + list(r1[1]), list(r2[0]) + list(r2[1])))


def _item_outputs(bs, Q=30):
    g = torch.Generator().manual_seed(11)
    srcs = [torch.randn(bs, Q, w, generator=g).to(DEV) for w in _native.ARCTIC_ITEM_WIDTHS]
    return {"pred_logits": torch.randn(bs, Q, 14, generator=g).to(DEV), "pred_cams": srcs[0:2],
            "pred_mano_params": srcs[2:4], "pred_obj_params": srcs[4:6]}


def test_no_host_sync():
    torch.manual_seed(5)
    a = ArcticSmoother(1, 32).to(DEV).train()
    o = _item_outputs(32)

    def step():
        with torch.no_grad():
            items = perturb_arctic_item(get_arctic_item(o, SI.Cfg()))
        ys = SI.flatten(a(items))
        sum(y.sum() for y in ys).backward()

    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_no_grad_saves_nothing():
    a = ArcticSmoother(1, 32).to(DEV).eval()
    xs = [t.to(DEV) for t in SI.arctic_inputs()]
    with torch.no_grad():
        ys = SI.flatten(a(SI.structure(xs)))
    assert all(y.grad_fn is None for y in ys)


def test_graph_capture():
    torch.manual_seed(6)
    a = ArcticSmoother(1, 32).to(DEV)
    xs = [t.to(DEV) for t in SI.arctic_inputs()]
    for train in (False, True):
        a.train(train)
        eager = [t.detach().clone() for t in _arctic_step(a, xs)[0]] if not train else None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _arctic_step(a, xs)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = _arctic_step(a, xs)
        graph.replay()
        torch.cuda.synchronize()
        first = [t.detach().clone() for t in static[0]]
        if not train:
            assert all(torch.equal(u, v) for u, v in zip(eager, first))
        else:
            graph.replay()
            torch.cuda.synchronize()
            assert not all(torch.equal(u, v) for u, v in zip(first, static[0]))    # fresh masks per replay
