"""``bracket_linear`` — ``F.linear`` for the four projections around the sampling kernel
(UVHand models/ops/modules/ms_deform_attn.py:96,100,101,139) with the weight / bias gradient on the
hand-written split-M MFMA kernel (``msda_linear_wgrad_f32``, include/msda.h).

The forward ``x @ W^T + b`` and the input gradient ``dy @ W`` run at 38-97 TFLOP/s on the vendor BLAS at
these shapes and stay there when the layer is large; small layers take the library's own plain-launch kernels
(``_own_rows`` below: host cost).  The weight gradient ``dy^T @ x`` with few rows (600 at the
300-query decoder shape) is run by hipBLASLt as one 256x256 tile on one CU — 141 us, 0.6 TFLOP/s
(tools/gemm_baseline.py).  Numerics: fp32 MFMA is an exact fp32 fma chain; the split-M partial sums
are combined in a fixed order, so the result is reproducible run to run.

Under ``torch.autocast(bfloat16)`` the same is done on bf16 operands (``_BracketLinearAmpFn``).  Falls back to
``F.linear`` — PyTorch's own implementation of the same layer, not an alternative implementation of the op —
whenever the kernels' preconditions do not hold (CPU tensors, other dtypes, fp16 autocast, feature counts not
multiples of 4), so the module keeps working everywhere nn.Linear does.

``fused_ffn`` — the layers' FFN as one node: ``_FusedFFNFn`` in fp32, and under bf16 autocast with ``MSDA_FFN_BF16=1`` the
library's own bf16 MFMA kernels (``_FusedFFNAmpFn``, csrc/msda_ffn_bf16.hip); ``ffn_keep_mask`` and
``fused_ffn_bf16_reference`` restate that node's dropout mask and rounding points in torch ops.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as MSDA


def _own_rows(a2, weight, reduce_dim):
    """The library's plain-launch fp32-MFMA forward / input-gradient kernels (msda_linear_forward_f32 / _dgrad_f32) take the
    layer while it is small — ~7 us of host time per call against ~18-27 us for a GEMM through torch, and as fast on the
    GPU up to ~5000 rows at 256 features (tools/gemm_time.py); beyond, the vendor BLAS's large macro-tiles run 1.3x faster.
    The same rule as own_linear() in csrc/torch_ext/msda_torch.cpp, so both forms of the module run the same kernels."""
    return (a2.shape[0] * weight.shape[0] <= 4800 * 256 and weight.shape[1] <= 512
            and MSDA.linear_rows_supported(a2, weight, reduce_dim))


def _rows_forward(x, weight, bias, mask=None):
    x2 = x.reshape(-1, x.shape[-1])
    if (x2.is_contiguous() and _own_rows(x2, weight, 1) and bias is not None and bias.is_contiguous()
            and bias.data_ptr() % 16 == 0):
        return MSDA.linear_forward(x2, weight, bias, mask).view(*x.shape[:-1], weight.shape[0])
    y = F.linear(x, weight, bias)
    if mask is not None:
        MSDA.zero_masked_rows_(y.view(-1, y.shape[-1]), mask)
    return y


def _rows_dgrad(go2, weight, mask=None):
    """go2: contiguous [rows, out]; a fresh [rows, in] buffer."""
    if _own_rows(go2, weight, 0):
        return MSDA.linear_dgrad(go2, weight, mask)
    gx2 = go2 @ weight
    return MSDA.zero_masked_rows_(gx2, mask) if mask is not None else gx2


class _BracketLinearFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _rows_forward(x, weight, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        go2 = grad_out.reshape(-1, grad_out.shape[-1])
        grad_x = grad_w = grad_b = None
        if need_x:
            grad_x = _rows_dgrad(go2.contiguous(), weight).view_as(x)
        if need_w or (need_b and ctx.has_bias):
            x2 = x.reshape(-1, x.shape[-1])
            go2c, x2c = go2.contiguous(), x2.contiguous()
            if MSDA.linear_wgrad_supported(go2c, x2c):
                grad_w, grad_b = MSDA.linear_wgrad(go2c, x2c, want_bias=ctx.has_bias and need_b)
            else:
                grad_w = go2c.t() @ x2c
                grad_b = go2c.sum(0) if (ctx.has_bias and need_b) else None
            if not need_w:
                grad_w = None
        return grad_x, grad_w, grad_b


class _BracketLinearAmpFn(Function):
    """The same layer under ``torch.autocast(dtype=torch.bfloat16)``: the forward is what autocast would run (operands
    rounded to bf16, bf16 output); the backward takes the bf16-operand weight-gradient kernel — fp32 products and
    accumulation, an fp32 result handed to the fp32 master parameter without a bf16 rounding in between — instead of the
    vendor's small-M bf16 GEMM (49.7 us at M = 600, 2 x 118 us at M = 33 440: profiles/r02_notes.md section 7)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xb, wb = x.to(torch.bfloat16), weight.to(torch.bfloat16)
        ctx.save_for_backward(xb, wb)
        ctx.has_bias = bias is not None
        ctx.x_dtype = x.dtype
        return F.linear(xb, wb, bias.to(torch.bfloat16) if bias is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        xb, wb = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        go2 = grad_out.reshape(-1, grad_out.shape[-1]).to(torch.bfloat16)
        grad_x = grad_w = grad_b = None
        if need_x:
            grad_x = (go2 @ wb).view_as(xb).to(ctx.x_dtype)
        if need_w or (need_b and ctx.has_bias):
            x2 = xb.reshape(-1, xb.shape[-1])
            go2c, x2c = go2.contiguous(), x2.contiguous()
            if MSDA.linear_wgrad_supported(go2c, x2c):
                grad_w, grad_b = MSDA.linear_wgrad(go2c, x2c, want_bias=ctx.has_bias and need_b)
            else:
                grad_w = (go2c.t() @ x2c).float()
                grad_b = go2c.float().sum(0) if (ctx.has_bias and need_b) else None
            if not need_w:
                grad_w = None
        return grad_x, grad_w, grad_b


class _MaskedBracketLinearFn(Function):
    """``F.linear(x, weight, bias).masked_fill(row_mask[..., None], 0)`` (value_proj + padding mask,
    models/ops/modules/ms_deform_attn.py:96-98) touching only the masked rows: the forward zeroes them in the
    GEMM output in place; the backward hands the mask to the weight-gradient kernel (masked rows of grad_out
    count as zero) and zeroes the same rows of the input gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, row_mask):
        mask = row_mask.reshape(-1).contiguous()
        y = _rows_forward(x, weight, bias, mask)
        ctx.save_for_backward(x, weight, mask)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight, mask = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        go2 = grad_out.reshape(-1, grad_out.shape[-1]).contiguous()
        grad_x = grad_w = grad_b = None
        if need_x:
            grad_x = _rows_dgrad(go2, weight, mask).view_as(x)
        if need_w or (need_b and ctx.has_bias):
            x2 = x.reshape(-1, x.shape[-1]).contiguous()
            if MSDA.linear_wgrad_supported(go2, x2):
                grad_w, grad_b = MSDA.linear_wgrad(go2, x2, want_bias=ctx.has_bias and need_b, row_mask=mask)
            else:                                                   # same escape as _BracketLinearFn (odd view offset, huge M)
                gom = go2.masked_fill(mask[:, None], 0)
                grad_w = gom.t() @ x2
                grad_b = gom.sum(0) if (ctx.has_bias and need_b) else None
            if not need_w:
                grad_w = None
        return grad_x, grad_w, grad_b, None


class _FusedFFNFn(Function):
    """``linear2(dropout(relu(linear1(x))))`` — the FFN of the layers (models/arctic_transformer.py:283-287, :366-370) — as ONE
    autograd node:
    * forward: bias + ReLU in the epilogue of linear1's GEMM (``torch._addmm_activation``: hipBLASLt's RELU_BIAS epilogue, or
      addmm + an in-place relu where the epilogue is not offered); dropout is PyTorch's own fused kernel
      (``torch.native_dropout``: the very call ``nn.Dropout`` makes, so the Philox stream is consumed exactly as in the
      reference's loop) — its mask is NOT kept;
    * backward: the dropout and ReLU gradients are one in-place pass over linear2's input gradient
      (``grad * scale * (a > 0)`` with ``a`` = linear2's saved input; msda_relu_dropout_backward_f32), and both weight
      gradients take the split-M MFMA kernel.
    Saved: x, a = dropout(relu(h)), the two weights — not h, not relu(h), not the mask (at the training shape 137 + 137 + 34
    MB per encoder layer less).  One difference from the reference's composition: where h is NaN the reference's
    threshold_backward lets the gradient through and this node blocks it (NaN > 0 is false) — the loss is NaN either way."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, p, training):
        x2 = x.reshape(-1, x.shape[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        h = torch._addmm_activation(b1, x2, w1.t())                      # relu(x2 @ w1^T + b1)
        drop = bool(training) and 0.0 < p < 1.0
        a = torch.native_dropout(h, p, True)[0] if drop else h
        y = torch.addmm(b2, a, w2.t())
        ctx.save_for_backward(x2, a, w1, w2)
        ctx.scale = 1.0 / (1.0 - p) if drop else 1.0
        ctx.x_shape = x.shape
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x2, a, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        go2 = grad_out.reshape(-1, grad_out.shape[-1]).contiguous()
        gw2 = gb2 = gw1 = gb1 = gx = None
        if need[3] or need[4]:
            if MSDA.linear_wgrad_supported(go2, a):
                gw2, gb2 = MSDA.linear_wgrad(go2, a, want_bias=need[4])
            else:
                gw2, gb2 = go2.t() @ a, (go2.sum(0) if need[4] else None)
            if not need[3]:
                gw2 = None
        if need[0] or need[1] or need[2]:
            gh = go2 @ w2                                                  # gradient of a, then of h in place
            MSDA.relu_dropout_backward_(gh, a, ctx.scale)
            if need[1] or need[2]:
                if MSDA.linear_wgrad_supported(gh, x2):
                    gw1, gb1 = MSDA.linear_wgrad(gh, x2, want_bias=need[2])
                else:
                    gw1, gb1 = gh.t() @ x2, (gh.sum(0) if need[2] else None)
                if not need[1]:
                    gw1 = None
            if need[0]:
                gx = (gh @ w1).view(ctx.x_shape)
        return gx, gw1, gb1, gw2, gb2, None, None


_M32 = 0xFFFFFFFF


def ffn_keep_mask(seed, rows, F, p):
    """The dropout keep mask [rows, F] (bool) of the bf16 FFN node for ``seed`` (an int, or a one-element int64 tensor on any
    device: the mask is built there, without a host read): the host restatement of the kernel's counter hash (at_mix /
    at_hash, csrc/msda_attn_tile.h) in integer torch ops — element (row, col) has the counter ``row * F + col`` and is kept
    iff its 32 hash bits are >= p * 2^32.  p == 0 keeps everything."""
    dev = seed.device if torch.is_tensor(seed) else torch.device("cpu")
    if p <= 0:
        return torch.ones((rows, F), dtype=torch.bool, device=dev)
    s = seed.reshape(()).to(torch.int64) if torch.is_tensor(seed) else torch.tensor(
        (int(seed) & 0xFFFFFFFFFFFFFFFF) - (1 << 64 if int(seed) & (1 << 63) else 0), dtype=torch.int64)
    mix = ((s & _M32) + ((s >> 32) & _M32) * 0x85EBCA6B) & _M32
    x = (torch.arange(rows * F, dtype=torch.int64, device=dev) + mix) & _M32
    x = ((x ^ (x >> 16)) * 0x85EBCA6B) & _M32
    x = ((x ^ (x >> 13)) * 0xC2B2AE35) & _M32
    return (x >= int(min(4294967295.0, float(p) * 4294967296.0))).view(rows, F)


def fused_ffn_bf16_reference(x, w1, b1, w2, b2, p, keep):
    """The rounding points of the bf16 FFN node (_FusedFFNAmpFn) in plain torch ops, on any device and differentiable:
    operands rounded to bf16, fp32 products and sums, the fp32 bias added before the one rounding of ``h``,
    ``a = rnd(relu(h) * keep / (1 - p))`` (``keep``: a bool mask [rows, F], or None for evaluation / p == 0) and
    ``y = rnd(a @ W2^T + b2)``, bf16 with ``x``'s leading shape.  Its autograd rounds where the node's backward rounds (the
    gradient of ``h`` once to bf16; ``gx`` once when ``x`` is bf16; parameter gradients unrounded fp32)."""
    bf, f32 = torch.bfloat16, torch.float32

    def rnd(t):                             # fp32 tensor of bf16 values; the gradient passes through unrounded
        t = t.to(f32)
        return t + (t.to(bf).to(f32) - t).detach()

    with torch.autocast(x.device.type, enabled=False):             # the roundings are spelled out: no autocast inside
        x2 = x.reshape(-1, x.shape[-1])
        x2 = x2.to(f32) if x2.dtype == bf else rnd(x2)              # a bf16 x receives its gradient rounded once to bf16
        h = (x2 @ rnd(w1).t() + b1.to(f32)).to(bf)                  # the one bf16 tensor inside: its gradient is gh, rounded once
        a = torch.relu(h.to(f32))
        if keep is not None and p > 0:
            a = rnd(a * torch.tensor(1.0 / (1.0 - p), dtype=f32, device=a.device) * keep.to(f32))
        y = (a @ rnd(w2).t() + b2.to(f32)).to(bf)
        return y.view(*x.shape[:-1], w2.shape[0])


class _FusedFFNAmpFn(Function):
    """``linear2(dropout(relu(linear1(x))))`` under ``torch.autocast(dtype=torch.bfloat16)`` as one node on the library's bf16
    MFMA kernels (csrc/msda_ffn_bf16.hip; opt-in: ``MSDA_FFN_BF16=1``).  Rounding points as ``fused_ffn_bf16_reference``:
    ``h`` exists in registers only, ``a`` is written once as bf16 and saved together with the bf16 ``x`` (written by the same
    launch when ``x`` is fp32) — no ``h``, no mask, no seed.  The dropout mask is the kernel's counter hash (``ffn_keep_mask``)
    of a seed drawn with one ``random_()`` on a device scalar: reproducible under ``manual_seed``, capturable in a HIP graph,
    not ``nn.Dropout``'s Philox stream.  The weights are rounded to bf16 in the kernels' staging loads: no bf16 copies.
    Library launches: forward 1; backward at most 5 (gh, gx, the two weight gradients' first stages, their one second stage),
    fewer when a gradient is not needed.  No host sync."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, p, training):
        x2 = x.reshape(-1, x.shape[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        if x2.data_ptr() % 16:                                            # a view at an odd offset: the kernels move 16 bytes
            x2 = x2.clone()
        drop = bool(training) and 0.0 < p < 1.0
        seed = torch.empty((), dtype=torch.int64, device=x.device).random_().view(1) if drop else None
        xb, a, y = MSDA.ffn_forward_bf16(x2, w1, b1, w2, b2, p if drop else 0.0, seed)
        ctx.save_for_backward(xb, a, w1, w2)
        ctx.p = p if drop else 0.0
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        ctx.seed = seed                                                   # for tests; the backward does not read it
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        xb, a, w1, w2 = ctx.saved_tensors
        need = ctx.needs_input_grad
        go2 = grad_out.reshape(-1, grad_out.shape[-1]).to(torch.bfloat16).contiguous()
        if go2.data_ptr() % 16:
            go2 = go2.clone()
        gx, gw1, gb1, gw2, gb2 = MSDA.ffn_backward_bf16(go2, xb, a, w1, w2, ctx.p, ctx.x_dtype, need[0], need[1], need[2],
                                                        need[3], need[4])
        return (gx.view(ctx.x_shape) if gx is not None else None), gw1, gb1, gw2, gb2, None, None


def _ffn_bf16_knob():
    return os.environ.get("MSDA_FFN_BF16", "") not in ("", "0")      # opt-in, read at call time


def _ffn_amp_applies(x, linear1, activation, dropout, linear2):
    return (_ffn_bf16_knob() and torch.is_autocast_enabled() and _autocast_dtype() == torch.bfloat16
            and activation is F.relu and type(linear1) is nn.Linear and type(linear2) is nn.Linear
            and type(dropout) is nn.Dropout and not dropout.inplace and dropout.p < 1.0
            and linear1.bias is not None and linear2.bias is not None
            and all(t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 == 0
                    for t in (linear1.weight, linear1.bias, linear2.weight, linear2.bias))
            and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.numel() > 0
            and linear1.in_features == linear2.out_features and linear1.out_features == linear2.in_features
            and MSDA.ffn_bf16_supported(linear1.in_features, linear1.out_features)
            and (x.numel() // x.shape[-1]) * linear1.out_features < 2 ** 31)


_FUSED_FFN = os.environ.get("MSDA_FUSED_FFN", "1") != "0"            # A/B knob: 0 = the composition of bracket_linear / F.relu / nn.Dropout


def fused_ffn(x, linear1, activation, dropout, linear2):
    """``linear2(dropout(activation(linear1(x))))`` for two ``nn.Linear`` layers and an ``nn.Dropout``: one autograd node
    (_FusedFFNFn) when the activation is ReLU and the layers are plain float32 CUDA layers with biases outside autocast;
    under bf16 autocast with ``MSDA_FFN_BF16=1`` the bf16 node (_FusedFFNAmpFn) where its kernels take the widths; else the
    composition of the same modules (bracket_linear keeps the weight-gradient kernel there)."""
    if _ffn_amp_applies(x, linear1, activation, dropout, linear2):
        return _FusedFFNAmpFn.apply(x, linear1.weight, linear1.bias, linear2.weight, linear2.bias, float(dropout.p),
                                    dropout.training)
    if (_FUSED_FFN and _ENABLED and activation is F.relu and type(linear1) is nn.Linear and type(linear2) is nn.Linear
            and type(dropout) is nn.Dropout and not dropout.inplace and dropout.p < 1.0
            and linear1.bias is not None and linear2.bias is not None and x.is_cuda and x.dtype == torch.float32
            and all(t.dtype == torch.float32 and t.is_cuda for t in (linear1.weight, linear1.bias, linear2.weight, linear2.bias))
            and not torch.is_autocast_enabled() and linear1.out_features % 4 == 0 and linear1.in_features % 4 == 0
            and linear2.out_features % 4 == 0 and x.numel() > 0):
        return _FusedFFNFn.apply(x, linear1.weight, linear1.bias, linear2.weight, linear2.bias, float(dropout.p),
                                 dropout.training)
    return bracket_linear(dropout(activation(bracket_linear(x, linear1))), linear2)


_ENABLED = os.environ.get("MSDA_BRACKET_LINEAR", "1") != "0"       # A/B knob: 0 = always the plain layer
_MASKED_ROWS = os.environ.get("MSDA_MASKED_ROWS", "1") != "0"      # A/B knob: 0 = masked_fill after the layer


def _kernel_applies(x, weight):
    return (_ENABLED and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
            and not torch.is_autocast_enabled() and torch.is_grad_enabled()
            and weight.shape[1] % 4 == 0 and weight.shape[0] % 4 == 0)


def _autocast_dtype():
    try:
        return torch.get_autocast_dtype("cuda")
    except (AttributeError, TypeError):                      # older torch
        return torch.get_autocast_gpu_dtype()


def _amp_kernel_applies(x, weight):
    """bf16 autocast on CUDA around an fp32 layer (the reference trains its transformer this way when --amp is on)."""
    return (_ENABLED and x.is_cuda and torch.is_autocast_enabled() and _autocast_dtype() == torch.bfloat16
            and weight.dtype == torch.float32 and x.dtype in (torch.float32, torch.bfloat16) and torch.is_grad_enabled()
            and weight.shape[1] % 4 == 0 and weight.shape[0] % 4 == 0)


def bracket_linear_wb(x, weight, bias):
    """``F.linear(x, weight, bias)``; custom weight-gradient kernel when applicable."""
    if _kernel_applies(x, weight):
        return _BracketLinearFn.apply(x, weight, bias)
    if _amp_kernel_applies(x, weight):
        return _BracketLinearAmpFn.apply(x, weight, bias)
    return F.linear(x, weight, bias)


def bracket_linear_masked(x, layer, row_mask):
    """``layer(x).masked_fill(row_mask[..., None], 0)`` for an ``nn.Linear`` ``layer`` and a bool mask over the
    leading dimensions of ``x``; the masked rows only are touched when the kernels apply."""
    if (_MASKED_ROWS and _kernel_applies(x, layer.weight) and row_mask.dtype == torch.bool and row_mask.is_cuda
            and row_mask.shape == x.shape[:-1]):
        return _MaskedBracketLinearFn.apply(x, layer.weight, layer.bias, row_mask)
    return bracket_linear(x, layer).masked_fill(row_mask[..., None], float(0))


def bracket_linear(x, layer):
    """``layer(x)`` for an ``nn.Linear`` ``layer``; custom weight-gradient kernel when applicable."""
    if _kernel_applies(x, layer.weight):
        return _BracketLinearFn.apply(x, layer.weight, layer.bias)
    if _amp_kernel_applies(x, layer.weight):
        return _BracketLinearAmpFn.apply(x, layer.weight, layer.bias)
    return layer(x)
