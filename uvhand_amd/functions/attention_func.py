"""Decoder self-attention of the drop-in layers (UVHand models/arctic_transformer.py:351, :374-376:
``nn.MultiheadAttention(d_model, n_heads, dropout)`` called sequence-first with q = k = tgt + query_pos, v = tgt, no masks) with
the attention core — ``dropout(softmax(q k^T / sqrt(d))) v`` — on the library's own kernels (msda_attn32_*_f32, include/msda.h)
when it fits them: head_dim 32, at most 320 queries, fp32 inputs outside autocast or under bf16 autocast, no masks.  The module, its parameters and state_dict keys stay
``nn.MultiheadAttention``'s; the in- and out-projections are ``nn.Linear``'s arithmetic on the module's own weights (q and k share
their input, so their two projections are ONE GEMM on the first two thirds of ``in_proj_weight``), with the weight gradients on the
library's MFMA kernel like every other projection of the drop-in layers (``functions/linear_func.py``).

What differs from the stock module: no [N*heads, L, L] tensor is ever written (scores, probabilities, dropout mask), and the
attention dropout draws its mask from the kernel's own hash of (seed, head, query, key) — the seed comes from torch's generator
(one ``random_()`` on a device scalar: reproducible under ``manual_seed``, capturable in a HIP graph), the stream is not
``nn.functional.dropout``'s.  Anything the kernels do not take goes to the module itself.

Under ``torch.autocast("cuda", dtype=torch.bfloat16)`` the inputs are still the fp32 residual stream; the projections take their
amp path and return bf16, and the core runs on the bf16 kernels (msda_attn32_*_bf16): bf16 operands, fp32 softmax and
accumulation, bf16 output and bf16 gradients of the projections' outputs — the dtypes the stock module has under the same
autocast.  The attention dropout then draws from the same kernel hash (for one seed the bf16 and fp32 cores drop the same
entries), not from ``nn.functional.dropout``.  fp16 autocast stays with the module.

Masked and long inputs (DINO's decoder, models/dino/deformable_transformer.py:966: ``pad_size + num_queries`` rows, about 1100,
under the contrastive-denoising mask of models/dino/dn_components.py:125-137).  A 2-D ``torch.bool`` CUDA ``attn_mask`` [L, L]
(True = hidden) routes the core through the streaming kernels (msda_attn32x_*_f32: head_dim 32, fp32, 1 <= L <= 2048) outside
autocast; ``MSDA_ATTN_LONG=1`` (read at call time) sends unmasked inputs of 320 < L <= 2048 there too — the 900-query
evaluation.  The projections, their weight gradients and the dropout stream are the ones above.  Float masks, 3-D masks, other
head sizes, L > 2048 and CPU tensors go to the module with the mask.
A query row whose every key is hidden is NaN, as the module's; its gradients are outside the kernels' contract.

Under bf16 autocast the same two rules apply only when ``MSDA_ATTN_LONG_BF16=1`` is set (read at call time, off by default): the
projections return bf16 and the core runs on the streaming bf16 kernels (msda_attn32x_*_bf16: bf16 operands, fp32 online softmax
and accumulation, bf16 output and gradients).  A 2-D bool CUDA mask routes there; unmasked 320 < L <= 2048 needs
``MSDA_ATTN_LONG=1`` as well; unmasked L <= 320 stays on the resident bf16 core.  With the knob unset every masked or long input
under autocast is the module's, as before; fp16 autocast always is."""
import math
import os

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as MSDA
from .linear_func import _autocast_dtype, bracket_linear_wb


class _AttnFn(Function):
    """core(family, qk [L, N, 2E] = packed q | k projections, v [L, N, E], mask [L, L] bool or None) -> [L, N, E].  family
    "attn32": the resident kernels (msda_attn32_*, no mask); "attn32x": the streaming ones (msda_attn32x_*).  fp32 or bf16:
    dispatch on qk's dtype."""

    @staticmethod
    def forward(ctx, family, qk, v, mask, heads, dropout_p):
        E = v.shape[2]
        q, k = qk[..., :E], qk[..., E:]
        scale = 1.0 / math.sqrt(E // heads)
        seed = torch.empty((), dtype=torch.int64, device=v.device).random_().view(1) if dropout_p > 0 else None
        extra = (mask,) if family == "attn32x" else ()   # (the resident binding takes no mask; the public names, looked up per call)
        out, lse = getattr(MSDA, family + "_forward")(q, k, v, heads, scale, dropout_p, seed, *extra)
        ctx.save_for_backward(qk, v, out, lse, *([mask] if mask is not None else []), *([seed] if seed is not None else []))
        ctx.family, ctx.heads, ctx.scale, ctx.dropout_p, ctx.masked = family, heads, scale, dropout_p, mask is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        qk, v, out, lse = ctx.saved_tensors[:4]
        rest = list(ctx.saved_tensors[4:])
        mask = rest.pop(0) if ctx.masked else None
        seed = rest.pop(0) if rest else None
        E = v.shape[2]
        g_qk = torch.empty_like(qk, memory_format=torch.contiguous_format)
        if grad_out.dtype != qk.dtype:                   # (the core's output type: fp32, or bf16 under autocast)
            grad_out = grad_out.to(qk.dtype)
        extra = (mask,) if ctx.family == "attn32x" else ()
        _, _, g_v = getattr(MSDA, ctx.family + "_backward")(qk[..., :E], qk[..., E:], v, out, lse, grad_out, ctx.heads, ctx.scale,
                                                            ctx.dropout_p, seed, *extra, grad_q=g_qk[..., :E], grad_k=g_qk[..., E:])
        return None, g_qk, g_v, None, None, None


def _takes_common(mha, x_qk, x_v):
    E = mha.embed_dim
    return (type(mha) is nn.MultiheadAttention and mha._qkv_same_embed_dim and not mha.batch_first and mha.bias_k is None
            and mha.bias_v is None and not mha.add_zero_attn and mha.in_proj_bias is not None and mha.head_dim == 32
            and x_qk.is_cuda and x_qk.dtype == torch.float32 and x_v.dtype == torch.float32 and x_qk.dim() == 3
            and x_qk.shape == x_v.shape and x_qk.shape[2] == E)


def _takes_long(mha, x_qk, x_v, attn_mask):
    """The streaming core: _takes' conditions with its length bound, for a 2-D bool CUDA mask [L, L] — or, unmasked, for
    320 < L when MSDA_ATTN_LONG=1.  Outside autocast (fp32), or under bf16 autocast when MSDA_ATTN_LONG_BF16=1."""
    if attn_mask is None:
        if os.environ.get("MSDA_ATTN_LONG", "0") in ("", "0"):
            return False
    elif not (torch.is_tensor(attn_mask) and attn_mask.dtype == torch.bool and attn_mask.is_cuda and attn_mask.dim() == 2
              and attn_mask.shape[0] == attn_mask.shape[1] == x_qk.shape[0] and attn_mask.device == x_qk.device):
        return False
    if not _takes_common(mha, x_qk, x_v):
        return False
    if torch.is_autocast_enabled() and (_autocast_dtype() != torch.bfloat16
                                        or os.environ.get("MSDA_ATTN_LONG_BF16", "0") in ("", "0")):
        return False                                     # (bf16 autocast: the bf16 kernels, opt-in; fp16: the module)
    L = x_qk.shape[0]
    if attn_mask is None and MSDA.attn32_supported(L, L, mha.head_dim):
        return False                                     # (unmasked and short: the resident core's)
    return MSDA.attn32x_supported(L, L, mha.head_dim)


def _takes(mha, x_qk, x_v):
    return (_takes_common(mha, x_qk, x_v)
            and (not torch.is_autocast_enabled() or _autocast_dtype() == torch.bfloat16)
            and MSDA.attn32_supported(x_qk.shape[0], x_v.shape[0], mha.head_dim))


def self_attention(mha, x_qk, x_v, attn_mask=None):
    """``mha(x_qk, x_qk, x_v, attn_mask=attn_mask, need_weights=False)[0]`` for sequence-first inputs [L, N, E]."""
    long_core = _takes_long(mha, x_qk, x_v, attn_mask)
    if not long_core and (attn_mask is not None or not _takes(mha, x_qk, x_v)):
        return mha(x_qk, x_qk, x_v, attn_mask=attn_mask, need_weights=False)[0]
    E = mha.embed_dim
    w, b = mha.in_proj_weight, mha.in_proj_bias
    # (the three projections through bracket_linear_wb: nn.Linear's forward, the weight gradients on the library's split-M MFMA
    # kernel — torch runs the 9600-row ones at a third of its rate, 61 against 26 us each, tools/wgrad_time.py)
    qk = bracket_linear_wb(x_qk, w[:2 * E], b[:2 * E])
    v = bracket_linear_wb(x_v, w[2 * E:], b[2 * E:])
    p = float(mha.dropout) if mha.training else 0.0
    core = _AttnFn.apply("attn32x" if long_core else "attn32", qk, v, attn_mask, mha.num_heads, p)     # (resident: no mask got here)
    return bracket_linear_wb(core, mha.out_proj.weight, mha.out_proj.bias)
