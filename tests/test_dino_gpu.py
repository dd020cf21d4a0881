"""The DINO decoder's kernels (csrc/msda_dino.hip) on the GPU: the sine table, the one-launch and the table query_pos routes with
their backward, and the refinement with its backward.  The rule is the project's own (tests/test_attention_long_gpu.py,
tests/test_optim_gpu.py): per tensor the kernel's largest error against an fp64 evaluation is at most 4 times that of the torch
fp32 composition on the GPU, which counts as at least one fp32 ulp of the tensor's largest value (dino_inputs.hold).  The row
code of the refinement must equal a numpy statement of the rule on the same fp32 logits in every row."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_inputs as DI  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = {}
# 63, 64, 65 and 129 rows around the 64-row panel, frames that do not divide it, one row, more than one workgroup
SHAPES = [(1, 1), (1, 3), (21, 3), (32, 2), (13, 5), (43, 3), (257, 1)]


def _dev():
    return torch.device("cuda:0")


def _points(L, N, W, seed):
    g = torch.Generator().manual_seed(seed)
    ref = torch.rand(L, N, W, generator=g) * 2 - 1
    flat = ref.view(-1)
    for i, v in enumerate((-1.0, 0.0, 1.0)):                     # the ends and the middle of the range, exactly
        if i < flat.numel():
            flat[(i * 17) % flat.numel()] = v
    ratios = torch.rand(N, 2, 2, generator=g) * 0.5 + 0.5         # [N, levels, 2] in [0.5, 1]
    ratios[0] = 1.0                                               # one frame exactly 1
    return ref.to(_dev()), ratios.to(_dev())


def _head(seed):
    from uvhand_amd.modules.detr import MLP
    torch.manual_seed(seed)
    return MLP(256, 256, 256, 2).to(_dev())


@pytest.mark.parametrize("W", [2, 42])
@pytest.mark.parametrize("L,N", SHAPES)
def test_sine_table(L, N, W):
    from uvhand_amd.functions import dino_func as DF
    ref, ratios = _points(L, N, W, 100 + L + N + W)
    for valid in (ratios[:, 0].contiguous(), None):
        ours = DF.sine_embed_for_position(ref, valid)
        assert ours.shape == (L, N, 256)
        t32 = DF.sine_embed_composition(ref, valid)
        r64 = DF.sine_embed_composition(ref.double(), valid.double() if valid is not None else None)
        DI.hold("pe W=%d valid=%s" % (W, valid is not None), ours, t32, r64, RATIOS)
        assert torch.equal(ours, DF.sine_embed_for_position(ref, valid))          # two runs, bit for bit


@pytest.mark.parametrize("route", ["fused", "table"])
@pytest.mark.parametrize("W", [2, 42])
@pytest.mark.parametrize("L,N", SHAPES)
def test_query_pos(L, N, W, route):
    from uvhand_amd import _native as MSDA
    from uvhand_amd.functions import dino_func as DF
    ref, ratios = _points(L, N, W, 200 + L + N + W)
    head = _head(7)
    head64 = copy.deepcopy(head).double()
    head32 = copy.deepcopy(head)
    gy = torch.randn(L, N, 256, generator=torch.Generator().manual_seed(L * N)).to(_dev())

    before = MSDA.launch_count()
    y = DF.query_pos(ref, ratios, head, route=route)
    fwd_launches = MSDA.launch_count() - before
    assert fwd_launches == 1                                      # fused: the whole forward; table: the table kernel
    y.backward(gy)
    y32 = DF.query_pos_composition(ref, ratios, head32)
    y32.backward(gy)
    y64 = DF.query_pos_composition(ref.double(), ratios.double(), head64)
    y64.backward(gy.double())
    tag = "%s W=%d " % (route, W)
    DI.hold(tag + "y", y.detach(), y32.detach(), y64.detach(), RATIOS)
    for (k, p), p32, p64 in zip(head.named_parameters(), head32.parameters(), head64.parameters()):
        DI.hold(tag + "grad " + k, p.grad, p32.grad, p64.grad, RATIOS)
    if route == "fused":
        dim_t = DF._dim_t64(ref.device)
        l1, l2 = head.layers
        args = (ref.view(L * N, W), ratios[:, 0].contiguous(), N, dim_t, l1.weight.detach(), l1.bias.detach(), l2.weight.detach(),
                l2.bias.detach())
        h, y2 = MSDA.dino_query_pos_forward(*args)
        pe32 = DF.sine_embed_composition(ref, ratios[:, 0])
        pe64 = DF.sine_embed_composition(ref.double(), ratios[:, 0].double())
        DI.hold(tag + "h", h.view(L, N, 256), torch.relu(head32.layers[0](pe32)).detach(),
                torch.relu(head64.layers[0](pe64)).detach(), RATIOS)
        assert torch.equal(y2.view(L, N, 256), y.detach())
        h3, y3 = MSDA.dino_query_pos_forward(*args)               # two runs, bit for bit
        assert torch.equal(h3, h) and torch.equal(y3, y2)


def test_query_pos_launch_counts_with_frozen_layers():
    """The fused node's backward is library launches only, and a frozen layer costs none of its own."""
    from uvhand_amd import _native as MSDA
    from uvhand_amd.functions import dino_func as DF
    L, N, W = 43, 3, 42
    ref, ratios = _points(L, N, W, 9)
    gy = torch.randn(L, N, 256, device=_dev())

    def count(fn):
        before = MSDA.launch_count()
        fn()
        return MSDA.launch_count() - before

    a, b = torch.randn(L * N, 256, device=_dev()), torch.randn(L * N, 256, device=_dev())
    w = torch.randn(256, 256, device=_dev())
    n_w = count(lambda: MSDA.linear_wgrad(a, b))
    n_d = count(lambda: MSDA.linear_dgrad(a, w))
    n_r = count(lambda: MSDA.relu_dropout_backward_(a.clone(), b, 1.0))
    n_s = count(lambda: MSDA.dino_sine_embed(ref.view(L * N, W), None, N, DF._dim_t64(ref.device)))
    assert (n_d, n_r, n_s) == (1, 1, 1)

    def backward_launches(freeze0, freeze1):
        head = _head(11)
        for p in head.layers[0].parameters():
            p.requires_grad_(not freeze0)
        for p in head.layers[1].parameters():
            p.requires_grad_(not freeze1)
        y = DF.query_pos(ref, ratios, head, route="fused")
        if not y.requires_grad:
            return 0
        return count(lambda: y.backward(gy))

    assert backward_launches(False, False) == 2 * n_w + n_d + n_r + n_s
    assert backward_launches(True, False) == n_w                  # layer 0 frozen: the second layer's weight gradient alone
    assert backward_launches(False, True) == n_w + n_d + n_r + n_s
    assert backward_launches(True, True) == 0


def _numpy_codes(cls, hand=(12, 13)):
    c = np.argmax(cls, axis=-1)                                    # first maximum; numpy ranks NaN highest, first NaN wins
    is_hand = (c == hand[0]) | (c == hand[1])
    return np.where(is_hand, 2, np.where(c != 0, 1, 0)).astype(np.uint8)


def _refine_inputs(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    ref = torch.rand(M, 42, generator=g) * 2 - 1
    for i, v in enumerate((-1.0, 0.0, 1e-5, 1 - 1e-5, 1.0)):
        ref.view(-1)[(i * 5) % ref.numel()] = v
    cls = torch.randn(M, K, generator=g)
    rows = list(range(0, M, max(1, M // 9)))
    for j, r in enumerate(rows):
        kind = j % 5
        if kind == 0 and K > 1:
            cls[r, :] = cls[r].max() + 1.0                         # every class ties: the first wins
        elif kind == 1 and K > 1:
            cls[r, K - 1] = cls[r, K // 2] = cls[r].max() + 1.0    # a tie between two classes
        elif kind == 2:
            cls[r, (3 * j) % K] = float("nan")
        elif kind == 3:
            cls[r, (5 * j) % K] = float("inf")
        elif kind == 4:
            cls[r, :] = float("-inf")
    dk, do = torch.randn(M, 42, generator=g), torch.randn(M, 42, generator=g)
    go = torch.randn(M, 42, generator=g)
    return [t.to(_dev()) for t in (ref, cls, dk, do, go)]


@pytest.mark.parametrize("K", [1, 2, 13, 14, 15, 64])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1025])
def test_refine(M, K):
    from uvhand_amd import _native as MSDA
    from uvhand_amd.functions import dino_func as DF
    ref, cls, dk, do, go = _refine_inputs(M, K, 1000 * K + M)
    out, code = MSDA.dino_refine_forward(ref, cls, dk, do)
    want = _numpy_codes(cls.cpu().numpy())
    assert np.array_equal(code.cpu().numpy(), want)                # every row
    if K == 1:
        assert not want.any()
    if K <= 12:
        assert (want != 2).all()                                   # no hand class at all (at K = 13 class 13 alone is absent)

    dk_, do_ = dk.clone().requires_grad_(True), do.clone().requires_grad_(True)
    ours = DF.refine(ref, cls, dk_, do_)
    assert torch.equal(ours.detach(), out)
    ours.backward(go)
    outs, grads = [], []
    for dt in (torch.float32, torch.float64):
        a, b = dk.to(dt).requires_grad_(True), do.to(dt).requires_grad_(True)
        o = DF.refine_composition(ref.to(dt), cls, a, b)
        o.backward(go.to(dt))
        outs.append(o.detach())
        grads.append(tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in (a, b)))   # (None: the delta never used)
    DI.hold("refine out", out, outs[0], outs[1], RATIOS)
    DI.hold("refine grad_key", dk_.grad, grads[0][0], grads[1][0], RATIOS)
    DI.hold("refine grad_obj", do_.grad, grads[0][1], grads[1][1], RATIOS)
    code_t = torch.from_numpy(want).to(_dev())
    assert (dk_.grad[code_t != 2] == 0).all() and (do_.grad[code_t != 1] == 0).all()
    out2, code2 = MSDA.dino_refine_forward(ref, cls, dk, do)       # two runs, bit for bit
    g1 = MSDA.dino_refine_backward(go, out, code)
    g2 = MSDA.dino_refine_backward(go, out2, code2)
    assert torch.equal(out, out2) and torch.equal(code, code2) and torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    assert torch.equal(g1[0], dk_.grad) and torch.equal(g1[1], do_.grad)


def test_zz_print_ratios():
    for k in sorted(RATIOS):
        print("worst ratio %-40s %.2f" % (k, RATIOS[k]))
