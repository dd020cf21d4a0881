"""The memory-bound glue of a Swin block (models/swin_transformer.py:209-245: norm1, shortcut + drop_path, norm2, x + drop_path)
and of PatchMerging (:263-287: pad, 2 x 2 gather, concatenation, norm) as four autograd nodes over ``csrc/msda_swin_glue.hip``.

``MSDA_SWIN_GLUE=1`` switches them on (opt-in, read at call time; unset, ``""`` and ``"0"`` mean off).  The residual stream is
fp32; T, the type of the normalised rows and of the branch, is bfloat16 under bf16 autocast and float32 outside autocast.

``MSDA_SWIN_GLUE_BF16=1`` (opt-in as well, read at call time, only with ``MSDA_SWIN_GLUE`` on) lets a bfloat16 residual stream
under bf16 autocast take the same four nodes: from the first PatchMerging on, whose reduction Linear returns bfloat16 there.
y, grad_x and the rows the nodes save are then bfloat16, rounded where torch's bf16 arithmetic rounds (include/msda.h: y is
rounded before it is normalised; grad_x is rounded twice, by the cast's backward and by autograd's accumulation).

  ``norm_rows(x, norm)``                        LN(x) as T (``fp32_out=True``: float32 under autocast too, what F.layer_norm gives)
  ``add_norm_rows(x, branch, keep, norm)``      (y, z): y = x + branch * keep in one launch with z = LN(y) as T
  ``add_rows(x, branch, keep)``                 y = x + branch * keep
  ``merge_norm(x, H, W, norm)``                 [B, H*W, C] -> LN(cat of the 2 x 2 neighbours) [B, ceil(H/2) ceil(W/2), 4C] as T

``keep`` is drop_path's per-sample tensor [B, 1, 1] of the branch's type (``draw_keep`` draws it exactly as ``drop_path`` does, so
the Philox stream is consumed as in the composition and checkpoint recomputation replays it) or None.  The product is rounded to
the branch's type before the fp32 add, as torch does, so y is bit for bit ``x + drop_path(branch)``; the backward rounds
where torch's autograd rounds.  No kernel generates random numbers.

Everything else runs exactly the torch expressions: CPU tensors, fp16 autocast, an x that is neither fp32 nor (second knob, bf16
autocast) bfloat16, bfloat16 rows outside autocast, a width the kernels do not take (C % 4 != 0 or C > 3072), a norm that is not
an affine 1-d nn.LayerNorm, a branch of another type, and the knob off."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native
from .linear_func import _autocast_dtype

__all__ = ["glue_route", "norm_rows", "add_norm_rows", "add_rows", "merge_norm", "draw_keep"]


def _glue_enabled():
    return os.environ.get("MSDA_SWIN_GLUE", "0") not in ("", "0")       # opt-in (default off)


def _glue_bf16_stream_enabled():
    return os.environ.get("MSDA_SWIN_GLUE_BF16", "0") not in ("", "0")  # opt-in (default off)


def glue_route(device, dtype, C):
    """True when rows of this device, type and width take the HIP glue: the knob on, CUDA, C % 4 == 0 and C <= 3072, and either
    fp32 rows with no autocast or bf16 autocast, or bfloat16 rows under bf16 autocast with MSDA_SWIN_GLUE_BF16 on as well."""
    if not (_glue_enabled() and device.type == "cuda" and C % 4 == 0 and 0 < C <= _native.SWIN_GLUE_MAX_WIDTH):
        return False
    bf16_autocast = torch.is_autocast_enabled() and _autocast_dtype() == torch.bfloat16
    if dtype == torch.float32:
        return not torch.is_autocast_enabled() or bf16_autocast
    return dtype == torch.bfloat16 and bf16_autocast and _glue_bf16_stream_enabled()


def _branch_dtype():
    """T: what a Linear gives (and takes) on this route."""
    return torch.bfloat16 if torch.is_autocast_enabled() else torch.float32


def affine_layernorm(norm, C, device):
    """True for an nn.LayerNorm over the last dimension of width C with fp32 weight and bias on `device`."""
    return (isinstance(norm, nn.LayerNorm) and tuple(norm.normalized_shape) == (C,) and norm.weight is not None
            and norm.bias is not None and all(p.dtype == torch.float32 and p.device == device and p.is_contiguous()
                                              and p.data_ptr() % 16 == 0 for p in (norm.weight, norm.bias)))


def draw_keep(branch, drop_prob, training, scale_by_keep=True):
    """drop_path's random tensor for `branch` ([B, 1, ..., 1] of its type), drawn exactly as drop_path draws it; None where
    drop_path returns its input."""
    if drop_prob == 0. or not training:
        return None
    keep_prob = 1 - drop_prob
    shape = (branch.shape[0],) + (1,) * (branch.ndim - 1)
    random_tensor = branch.new_empty(shape).bernoulli_(keep_prob)
    if keep_prob > 0.0 and scale_by_keep:
        random_tensor.div_(keep_prob)
    return random_tensor


def _rows(t, align):
    """t contiguous with an aligned base (a view into the middle of a storage may have neither)."""
    t = t.contiguous()
    return t if t.data_ptr() % align == 0 else t.clone(memory_format=torch.contiguous_format)


def _align(dtype):
    return 16 if dtype == torch.float32 else 8


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _grad(g, like_dtype):
    return _rows(g if g.dtype == like_dtype else g.to(like_dtype), _align(like_dtype))


def _keep_ok(keep, branch):
    """keep: None, or one entry per sample of the branch, of the branch's type."""
    return keep is None or (branch.dim() >= 2 and keep.dtype == branch.dtype and keep.device == branch.device
                            and keep.numel() == branch.shape[0] and not keep.requires_grad)


def _rows_per_sample(branch):
    return max(1, branch.numel() // max(1, branch.shape[0] * branch.shape[-1]))


class _NormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype):
        z, mean, rstd = _native.swin_glue_norm_forward(x, weight, bias, eps, out_dtype)
        ctx.out_dtype = out_dtype
        ctx.save_for_backward(x, weight, mean, rstd)
        return z

    @staticmethod
    def backward(ctx, grad_z):
        x, weight, mean, rstd = ctx.saved_tensors
        gx, gw, gb = _native.swin_glue_norm_backward(_grad(grad_z, ctx.out_dtype), x, weight, mean, rstd)
        return gx, gw, gb, None, None


class _AddNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, keep, rows_per_sample, weight, bias, eps):
        y, z, mean, rstd = _native.swin_glue_add_norm_forward(x, a, keep, rows_per_sample, weight, bias, eps)
        ctx.rows_per_sample, ctx.branch_dtype, ctx.stream_dtype = rows_per_sample, a.dtype, x.dtype
        ctx.save_for_backward(y, keep, weight, mean, rstd)
        return y, z

    @staticmethod
    def backward(ctx, grad_y, grad_z):
        y, keep, weight, mean, rstd = ctx.saved_tensors
        gx, ga, gw, gb = _native.swin_glue_add_norm_backward(_grad(grad_y, ctx.stream_dtype), _grad(grad_z, ctx.branch_dtype), y,
                                                             keep, ctx.rows_per_sample, weight, mean, rstd)
        return gx, ga, None, None, gw, gb, None


class _AddFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, keep, rows_per_sample):
        ctx.rows_per_sample, ctx.branch_dtype, ctx.stream_dtype = rows_per_sample, a.dtype, x.dtype
        ctx.save_for_backward(keep)
        return _native.swin_glue_add_forward(x, a, keep, rows_per_sample)

    @staticmethod
    def backward(ctx, grad_y):
        keep, = ctx.saved_tensors
        grad_y = _grad(grad_y, ctx.stream_dtype)
        return grad_y, _native.swin_glue_add_backward(grad_y, keep, ctx.rows_per_sample, ctx.branch_dtype), None, None


class _MergeNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, out_dtype):
        z, mean, rstd = _native.swin_glue_merge_norm_forward(x, weight, bias, eps, out_dtype)
        ctx.out_dtype = out_dtype
        ctx.save_for_backward(x, weight, mean, rstd)
        return z

    @staticmethod
    def backward(ctx, grad_z):
        x, weight, mean, rstd = ctx.saved_tensors
        gx, gw, gb = _native.swin_glue_merge_norm_backward(_grad(grad_z, ctx.out_dtype), x, weight, mean, rstd)
        return gx, gw, gb, None, None


def norm_rows(x, norm, fp32_out=False):
    """norm(x) over the last dimension of fp32 or (glue_route) bfloat16 rows: one launch, as T (fp32_out: float32 whatever the
    autocast state)."""
    C = x.shape[-1] if x.dim() else 0
    if not (glue_route(x.device, x.dtype, C) and affine_layernorm(norm, C, x.device)):
        return norm(x)
    out_dtype = torch.float32 if fp32_out else _branch_dtype()
    x = _rows(x, _align(x.dtype))
    if not _needs_grad(x, norm.weight, norm.bias):
        return _native.swin_glue_norm_forward(x, norm.weight, norm.bias, norm.eps, out_dtype)[0]
    return _NormFunction.apply(x, norm.weight, norm.bias, norm.eps, out_dtype)


def _composition(x, branch, keep):
    return x + (branch if keep is None else branch * keep)


def _add_route(x, branch, keep):
    C = x.shape[-1] if x.dim() else 0
    return (glue_route(x.device, x.dtype, C) and branch.shape == x.shape and branch.device == x.device
            and branch.dtype == _branch_dtype() and _keep_ok(keep, branch))


def add_norm_rows(x, branch, keep, norm):
    """(y, z) = (x + branch * keep, norm(y)): one launch; y of x's type, z as T."""
    if not (_add_route(x, branch, keep) and affine_layernorm(norm, x.shape[-1], x.device)):
        y = _composition(x, branch, keep)
        return y, norm(y)
    x, branch = _rows(x, _align(x.dtype)), _rows(branch, _align(branch.dtype))
    keep = keep.reshape(-1) if keep is not None else None
    rps = _rows_per_sample(branch)
    if not _needs_grad(x, branch, norm.weight, norm.bias):
        return _native.swin_glue_add_norm_forward(x, branch, keep, rps, norm.weight, norm.bias, norm.eps)[:2]
    return _AddNormFunction.apply(x, branch, keep, rps, norm.weight, norm.bias, norm.eps)


def add_rows(x, branch, keep):
    """y = x + branch * keep: one launch, of x's type."""
    if not _add_route(x, branch, keep):
        return _composition(x, branch, keep)
    x, branch = _rows(x, _align(x.dtype)), _rows(branch, _align(branch.dtype))
    keep = keep.reshape(-1) if keep is not None else None
    rps = _rows_per_sample(branch)
    if not _needs_grad(x, branch):
        return _native.swin_glue_add_forward(x, branch, keep, rps)
    return _AddFunction.apply(x, branch, keep, rps)


def _merge_composition(x, H, W, norm):
    """PatchMerging.forward up to and including its norm (models/swin_transformer.py:270-285)."""
    B, L, C = x.shape
    x = x.view(B, H, W, C)
    if (H % 2 == 1) or (W % 2 == 1):
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x0 = x[:, 0::2, 0::2, :]
    x1 = x[:, 1::2, 0::2, :]
    x2 = x[:, 0::2, 1::2, :]
    x3 = x[:, 1::2, 1::2, :]
    x = torch.cat([x0, x1, x2, x3], -1)
    x = x.view(B, -1, 4 * C)
    return norm(x)


def merge_norm(x, H, W, norm):
    """x [B, H*W, C] -> norm(cat of the 2 x 2 neighbours) [B, ceil(H/2) ceil(W/2), 4C] as T: one launch."""
    B, L, C = x.shape
    if not (L == H * W and glue_route(x.device, x.dtype, 4 * C) and affine_layernorm(norm, 4 * C, x.device)):
        return _merge_composition(x, H, W, norm)
    x = _rows(x, _align(x.dtype)).view(B, H, W, C)
    out_dtype = _branch_dtype()
    if not _needs_grad(x, norm.weight, norm.bias):
        return _native.swin_glue_merge_norm_forward(x, norm.weight, norm.bias, norm.eps, out_dtype)[0]
    return _MergeNormFunction.apply(x, norm.weight, norm.bias, norm.eps, out_dtype).view(B, -1, 4 * C)
