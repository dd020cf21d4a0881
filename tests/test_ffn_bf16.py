"""The host side of the bf16-autocast FFN (uvhand_amd/functions/linear_func.py): the torch restatement of the node's rounding
points against an fp64 evaluation, the host restatement of the kernel's dropout hash, and the routes that do not change — on
the CPU, without a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from uvhand_amd.functions import linear_func
from uvhand_amd.functions.linear_func import ffn_keep_mask, fused_ffn, fused_ffn_bf16_reference

BF = torch.bfloat16


def _inputs(M=37, C=64, Fh=128, seed=0, bf16_valued=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g)
    w1, b1 = torch.randn(Fh, C, generator=g) / math.sqrt(C), torch.randn(Fh, generator=g) * 0.1
    w2, b2 = torch.randn(C, Fh, generator=g) / math.sqrt(Fh), torch.randn(C, generator=g) * 0.1
    if bf16_valued:
        x, w1, w2 = (t.to(BF).float() for t in (x, w1, w2))
    return x, w1, b1, w2, b2


def _fp64(x, w1, b1, w2, b2, p, keep):
    x, w1, b1, w2, b2 = (t.double() for t in (x, w1, b1, w2, b2))
    a = torch.relu(x @ w1.t() + b1)
    if keep is not None and p > 0:
        a = a * keep.double() / (1.0 - p)
    return a @ w2.t() + b2


def _ulp(x):
    m = float(x.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 7)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_reference_against_fp64_on_bf16_valued_inputs(p):
    """On bf16-valued operands the restatement differs from fp64 only by its three roundings (h, a, y) and fp32 summation: y
    within 4 bf16 ulps of the tensor's largest magnitude (one for y itself, the rest h's and a's roundings carried through W2,
    a sum of 128 terms of random sign: sqrt(128) * 2^-9 * |a| |w2| ~ 0.02 at these scales, under one ulp of max |y| ~ 4)."""
    x, w1, b1, w2, b2 = _inputs()
    keep = ffn_keep_mask(1234, x.shape[0], w1.shape[0], p) if p > 0 else None
    y = fused_ffn_bf16_reference(x, w1, b1, w2, b2, p, keep)
    ref = _fp64(x, w1, b1, w2, b2, p, keep)
    assert y.dtype == BF and y.shape == ref.shape
    assert float((y.double() - ref).abs().max()) <= 4 * _ulp(ref)
    # a bf16 x gives the same bits, with x's leading shape
    y3 = fused_ffn_bf16_reference(x.to(BF).view(1, *x.shape), w1, b1, w2, b2, p, keep)
    assert y3.shape == (1,) + tuple(y.shape) and torch.equal(y3[0], y)


def test_reference_gradients_round_where_the_node_rounds():
    """Parameter gradients and an fp32 x's gradient arrive unrounded fp32; a bf16 x's gradient is bf16; all are close to fp64's
    (8e-2 of max: the amp tolerance of tests/test_stack_gpu.py for gradients, here through two roundings)."""
    x, w1, b1, w2, b2 = _inputs()
    go = torch.randn(x.shape[0], w2.shape[0], generator=torch.Generator().manual_seed(5)).to(BF)
    outs = {}
    for name, xin in (("f32", x), ("bf16", x.to(BF))):
        leaves = [t.clone().requires_grad_(True) for t in (xin, w1, b1, w2, b2)]
        fused_ffn_bf16_reference(*leaves, 0.0, None).backward(go)
        outs[name] = [t.grad for t in leaves]
    leaves = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    _fp64(*leaves, 0.0, None).backward(go.double())
    assert outs["f32"][0].dtype == torch.float32 and outs["bf16"][0].dtype == BF
    assert not torch.equal(outs["f32"][0], outs["f32"][0].to(BF).float())            # not rounded to bf16
    assert torch.equal(outs["bf16"][0], outs["f32"][0].to(BF))                       # rounded once
    for got, ref in zip(outs["f32"], leaves):
        assert got.dtype == torch.float32
        assert float((got.double() - ref.grad).abs().max()) <= 8e-2 * float(ref.grad.abs().max())
    assert not torch.equal(outs["f32"][1], outs["f32"][1].to(BF).float())


def test_keep_mask_is_deterministic_in_the_seed():
    a, b = ffn_keep_mask(77, 130, 1024, 0.1), ffn_keep_mask(77, 130, 1024, 0.1)
    assert a.dtype == torch.bool and a.shape == (130, 1024) and torch.equal(a, b)
    assert torch.equal(a, ffn_keep_mask(torch.tensor([77]), 130, 1024, 0.1))         # a tensor seed: the same mask
    assert not torch.equal(a, ffn_keep_mask(78, 130, 1024, 0.1))
    assert not torch.equal(a, ffn_keep_mask(77 + (1 << 32), 130, 1024, 0.1))         # the high half counts
    neg = ffn_keep_mask(-5, 4, 64, 0.5)                                              # random_() seeds are non-negative; any int64 works
    assert torch.equal(neg, ffn_keep_mask(torch.tensor(-5), 4, 64, 0.5))
    assert torch.equal(neg, ffn_keep_mask((1 << 64) - 5, 4, 64, 0.5))


def test_keep_mask_p_zero_keeps_everything():
    assert bool(ffn_keep_mask(3, 5, 64, 0.0).all())


@pytest.mark.parametrize("seed", [1, 2 ** 40 + 17, 2 ** 62 + 3])
def test_keep_mask_drops_p_of_the_elements(seed):
    n, p = 130 * 1024, 0.1
    dropped = int((~ffn_keep_mask(seed, 130, 1024, p)).sum())
    assert abs(dropped - n * p) <= 6 * math.sqrt(n * p * (1 - p))


def test_keep_mask_is_the_kernel_hash():
    """Element (row, col) against a scalar restatement of at_mix / at_hash (csrc/msda_attn_tile.h) in Python integers."""
    seed, rows, Fh, p = (0x9E3779B97F4A7C15 & ((1 << 63) - 1)), 3, 64, 0.25
    m = 0xFFFFFFFF
    mix = ((seed & m) + ((seed >> 32) * 0x85EBCA6B)) & m
    thresh = int(min(4294967295.0, p * 4294967296.0))
    keep = ffn_keep_mask(seed, rows, Fh, p)
    for idx in (0, 1, 63, 64, 100, rows * Fh - 1):
        x = (idx + mix) & m
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & m
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & m
        assert bool(keep.view(-1)[idx]) == (x >= thresh), idx


def _layers(C=64, Fh=128):
    torch.manual_seed(0)
    return nn.Linear(C, Fh), nn.Dropout(0.0), nn.Linear(Fh, C)


@pytest.mark.parametrize("knob", [None, "1"])
def test_cpu_tensors_keep_todays_route(monkeypatch, knob):
    """Knob off, and knob on with CPU tensors (inside and outside CPU bf16 autocast): the composition's grad_fn, not the new
    node's, and the composition's values."""
    if knob is None:
        monkeypatch.delenv("MSDA_FFN_BF16", raising=False)
    else:
        monkeypatch.setenv("MSDA_FFN_BF16", knob)
    l1, drop, l2 = _layers()
    x = torch.randn(5, 64, requires_grad=True)
    y = fused_ffn(x, l1, F.relu, drop, l2)
    want = l2(drop(F.relu(l1(x))))
    assert type(y.grad_fn) is type(want.grad_fn) and torch.equal(y, want)
    assert "FusedFFNAmpFn" not in type(y.grad_fn).__name__
    with torch.autocast("cpu", dtype=BF):
        y = fused_ffn(x, l1, F.relu, drop, l2)
        want = l2(drop(F.relu(l1(x))))
    assert type(y.grad_fn) is type(want.grad_fn) and torch.equal(y, want)


def test_the_knob_is_read_at_call_time(monkeypatch):
    for value, on in ((None, False), ("", False), ("0", False), ("1", True)):
        if value is None:
            monkeypatch.delenv("MSDA_FFN_BF16", raising=False)
        else:
            monkeypatch.setenv("MSDA_FFN_BF16", value)
        assert linear_func._ffn_bf16_knob() is on
