"""Swin window attention (models/swin_transformer.py:68-142 WindowAttention, :199-245 the block's pad / roll / partition /
reverse / crop, :339-357 BasicLayer's shift mask) as one autograd node over the REAL tokens.

``window_attention(qkv_rows, qkv_bias, table, geometry)``: qkv_rows [B*H*W, 3C] is the qkv Linear's output on the real tokens
(columns (3, nH, 32)), geometry = (B, H, W, C, nH, ws, shift); returns out_rows [B*H*W, C] for the proj Linear.  norm1 runs
before F.pad in the reference, so a padded token's qkv is exactly ``qkv_bias``: padded keys and values are the bias's parts,
padded queries are cropped away.  The backward returns the gradients of qkv_rows, of the table and of the padded part of
qkv_bias (autograd adds it to the Linear's own bias gradient).

On CUDA fp32 with head_dim 32 and windows up to 12 it is ``_SwinAttnFunction``: one HIP launch forward, three backward
(``csrc/msda_swin.hip``), no host synchronisation, bitwise reproducible.  Everything else runs ``window_attention_reference``,
a torch restatement of the reference's path: CPU tensors, autocast, other dtypes, head_dim != 32 and ``MSDA_SWIN_FUSED=0``
(A/B knob).

``MSDA_SWIN_BF16=1`` (opt-in, read at call time, default off) adds the bf16 form: under bf16 autocast the qkv Linear's bf16 rows
go through the same node on the bf16 MFMA kernels (out and grad_qkv bf16; table, bias, log-sum-exp and their gradients fp32),
and so do bf16 rows outside autocast.  fp16 autocast keeps the restatement."""
import os

import torch
import torch.nn.functional as F

from .. import _native
from .linear_func import _autocast_dtype

HEAD_DIM = 32


def relative_position_index(ws):
    """WindowAttention's relative_position_index (models/swin_transformer.py:92-102) for a ws x ws window."""
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij"))
    coords_flatten = torch.flatten(coords, 1)
    rel = (coords_flatten[:, :, None] - coords_flatten[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def window_partition(x, window_size):
    """models/swin_transformer.py:38-49: (B, H, W, C) -> (num_windows*B, ws, ws, C)."""
    B, H, W, C = x.shape
    x = x.view(B, H // window_size, window_size, W // window_size, window_size, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, window_size, window_size, C)


def window_reverse(windows, window_size, H, W):
    """models/swin_transformer.py:52-65: (num_windows*B, ws, ws, C) -> (B, H, W, C)."""
    B = int(windows.shape[0] / (H * W / window_size / window_size))
    x = windows.view(B, H // window_size, W // window_size, window_size, window_size, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def shift_mask(H, W, window_size, shift_size, device):
    """BasicLayer's attention mask for SW-MSA (models/swin_transformer.py:339-357): [nW, N, N], 0 / -100."""
    Hp = -(-H // window_size) * window_size
    Wp = -(-W // window_size) * window_size
    img_mask = torch.zeros((1, Hp, Wp, 1), device=device)
    slices = (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None))
    cnt = 0
    for h in slices:
        for w in slices:
            img_mask[:, h, w, :] = cnt
            cnt += 1
    mask_windows = window_partition(img_mask, window_size).view(-1, window_size * window_size)
    attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
    return attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))


def window_attention_reference(qkv_rows, qkv_bias, table, geometry, rel_index=None, mask=None):
    """The reference's attention path on the real rows, restated in torch (the yardstick of the fused node)."""
    B, H, W, C, nH, ws, s = (int(g) for g in geometry)
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    N = ws * ws
    x = qkv_rows.view(B, H, W, 3 * C)
    if Hp != H or Wp != W:
        x = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))
        if qkv_bias is not None:                         # the padded tokens' qkv: the Linear on a zero row
            pad = torch.ones(Hp, Wp, 1, dtype=x.dtype, device=x.device)
            pad[:H, :W] = 0
            x = x + pad * qkv_bias.to(x.dtype)
    if s > 0:
        x = torch.roll(x, shifts=(-s, -s), dims=(1, 2))
    xw = window_partition(x, ws).view(-1, N, 3 * C)
    B_ = xw.shape[0]
    qkv = xw.reshape(B_, N, 3, nH, C // nH).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * (C // nH) ** -0.5
    attn = q @ k.transpose(-2, -1)
    if rel_index is None:
        rel_index = relative_position_index(ws).to(table.device)
    bias = table[rel_index.view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    if s > 0:
        if mask is None:
            mask = shift_mask(H, W, ws, s, x.device)
        nW = mask.shape[0]
        attn = attn.view(B_ // nW, nW, nH, N, N) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, nH, N, N)
    attn = attn.softmax(dim=-1)
    o = (attn @ v).transpose(1, 2).reshape(B_, N, C)
    o = window_reverse(o.view(-1, ws, ws, C), ws, Hp, Wp)
    if s > 0:
        o = torch.roll(o, shifts=(s, s), dims=(1, 2))
    if Hp != H or Wp != W:
        o = o[:, :H, :W, :].contiguous()
    return o.reshape(B * H * W, C)


def _fused_enabled():
    return os.environ.get("MSDA_SWIN_FUSED", "1") != "0"        # A/B knob: 0 = the torch restatement


def _bf16_enabled():
    return os.environ.get("MSDA_SWIN_BF16", "0") not in ("", "0")      # opt-in: the bf16 form of the node (default off)


def fused_route(device, dtype, C, nH, ws):
    """True when a block of this kind takes the HIP node: CUDA, head_dim 32, ws <= 12, knob on, and fp32 outside autocast.
    With MSDA_SWIN_BF16=1 also under bf16 autocast (dtype: the fp32 residual stream, or the qkv Linear's bf16 output) and for
    bf16 rows outside autocast.  fp16 autocast always takes the composition."""
    if not (_fused_enabled() and device.type == "cuda" and nH > 0 and C == HEAD_DIM * nH and 1 <= ws <= _native.SWIN_MAX_WINDOW):
        return False
    if torch.is_autocast_enabled():
        return _bf16_enabled() and _autocast_dtype() == torch.bfloat16 and dtype in (torch.float32, torch.bfloat16)
    return dtype == torch.float32 or (dtype == torch.bfloat16 and _bf16_enabled())


def _fused_ok(qkv_rows, qkv_bias, table, geometry):
    """The node takes qkv_rows as they are: fp32 rows run the fp32 kernels, bf16 rows the bf16 ones."""
    B, H, W, C, nH, ws, _ = geometry
    if not fused_route(qkv_rows.device, qkv_rows.dtype, C, nH, ws):
        return False
    if table.dtype != torch.float32 or table.device != qkv_rows.device or not table.is_contiguous():
        return False
    if qkv_bias is not None and (qkv_bias.dtype != torch.float32 or qkv_bias.device != qkv_rows.device
                                 or not qkv_bias.is_contiguous() or qkv_bias.data_ptr() % 16):
        return False
    if tuple(qkv_rows.shape) != (B * H * W, 3 * C):
        return False
    return _native.swin_attn_supported(geometry)


class _SwinAttnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, geometry, qkv_rows, qkv_bias, table):
        out, lse = _native.swin_attn_forward(geometry, qkv_rows, qkv_bias, table)
        ctx.geometry = geometry
        ctx.save_for_backward(qkv_rows, qkv_bias, table, out, lse)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qkv_rows, qkv_bias, table, out, lse = ctx.saved_tensors
        if grad_out.dtype != out.dtype:                  # (the node's output type: fp32, or bf16 under autocast)
            grad_out = grad_out.to(out.dtype)
        gq, gt, gb = _native.swin_attn_backward(ctx.geometry, qkv_rows, qkv_bias, table, out, lse, grad_out.contiguous())
        return None, gq, gb, gt


def window_attention(qkv_rows, qkv_bias, table, geometry, rel_index=None, mask=None):
    """out_rows [B*H*W, C] of the window attention of one block; see the module docstring.  ``rel_index`` / ``mask`` (the
    reference's buffers) are used by the restatement only."""
    geometry = tuple(int(g) for g in geometry)
    if not _fused_ok(qkv_rows, qkv_bias, table, geometry):
        return window_attention_reference(qkv_rows, qkv_bias, table, geometry, rel_index, mask)
    qkv_rows = qkv_rows.contiguous()
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (qkv_rows, qkv_bias, table)):
        return _native.swin_attn_forward(geometry, qkv_rows, qkv_bias, table)[0]
    return _SwinAttnFunction.apply(geometry, qkv_rows, qkv_bias, table)
