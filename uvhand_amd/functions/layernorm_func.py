"""``add_layer_norm(x, residual, norm)`` — ``norm(x + residual)`` for an ``nn.LayerNorm`` over the last dimension as
ONE kernel per direction (``msda_add_layernorm_*_f32``, include/msda.h) instead of an add and a LayerNorm
(UVHand models/arctic_transformer.py:279-282, 294-295, 366-368, 377-378, 385-386: ``x = x + dropout(x2); x = norm(x)``).

The dropout stays the caller's (PyTorch's own ``nn.Dropout`` on ``residual``), so training keeps the framework's random
stream.  Under bf16 autocast the layers pass the fp32 residual stream as ``x`` and the dropout of a bf16 projection output
as ``residual``; stock PyTorch then adds in fp32 (type promotion) and runs LayerNorm in fp32 (autocast's fp32 list), so the
output is fp32.  Here that is ``msda_add_layernorm_*_f32_bf16res`` (the residual widened exactly on load, the fp32 kernels'
arithmetic; its gradient is the fp32 one rounded to bf16, as the promotion's backward rounds it), or the fp32 kernel when
``residual`` is fp32 too.  Falls back to ``norm(x + residual)`` — the framework's implementation of the same two layers —
when the kernels' preconditions do not hold (CPU tensors, x not fp32, autocast to another type, no residual under autocast,
widths beyond 1024 or not a multiple of 4, LayerNorm without affine parameters), so the layers work wherever the
reference's do."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as MSDA
from .linear_func import _autocast_dtype


class _AddLayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps):
        y, mean, rstd = MSDA.add_layernorm_forward(x, residual, weight, bias, eps)
        ctx.save_for_backward(x, residual, weight, mean, rstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, residual, weight, mean, rstd = ctx.saved_tensors
        gs, gw, gb = MSDA.add_layernorm_backward(grad_y.contiguous(), x, residual, weight, mean, rstd)
        need = ctx.needs_input_grad
        return (gs if need[0] else None, gs if need[1] else None, gw if need[2] else None, gb if need[3] else None, None)


class _AddLayerNormBf16ResFn(Function):
    """x fp32, residual bf16 -> fp32 y; the residual's gradient is x's rounded to bf16 (one kernel writes both)."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps):
        y, mean, rstd = MSDA.add_layernorm_forward_bf16res(x, residual, weight, bias, eps)
        ctx.save_for_backward(x, residual, weight, mean, rstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, residual, weight, mean, rstd = ctx.saved_tensors
        gx, gr, gw, gb = MSDA.add_layernorm_backward_bf16res(grad_y.float().contiguous(), x, residual, weight, mean, rstd)
        need = ctx.needs_input_grad
        return (gx if need[0] else None, gr if need[1] else None, gw if need[2] else None, gb if need[3] else None, None)


def _amp_bf16():
    return torch.is_autocast_enabled() and _autocast_dtype() == torch.bfloat16


def add_layer_norm(x, residual, norm):
    """``norm(x + residual)`` (``residual`` may be None: plain ``norm(x)``)."""
    if (norm.elementwise_affine and norm.bias is not None and len(norm.normalized_shape) == 1
            and x.is_cuda and x.dtype == torch.float32):
        if not torch.is_autocast_enabled():
            xc = x.contiguous()
            rc = residual.contiguous() if residual is not None else None
            if MSDA.add_layernorm_supported(xc, rc, norm.weight, norm.bias):
                return _AddLayerNormFn.apply(xc, rc, norm.weight, norm.bias, norm.eps)
        elif residual is not None and residual.dtype in (torch.float32, torch.bfloat16) and _amp_bf16():
            xc, rc = x.contiguous(), residual.contiguous()
            if rc.dtype == torch.bfloat16:
                if MSDA.add_layernorm_bf16res_supported(xc, rc, norm.weight, norm.bias):
                    return _AddLayerNormBf16ResFn.apply(xc, rc, norm.weight, norm.bias, norm.eps)
            elif MSDA.add_layernorm_supported(xc, rc, norm.weight, norm.bias):
                return _AddLayerNormFn.apply(xc, rc, norm.weight, norm.bias, norm.eps)
    return norm(x if residual is None else x + residual)
