"""Drop-in Swin backbone (models/swin_transformer.py, models/position_encoding.py:18-56 PositionEmbeddingSine, models/backbone.py
Joiner and build_backbone's Swin branch).

Constructors, submodule and buffer names (the persistent ``relative_position_index`` included), creation order and the
``trunc_normal_`` init are the reference's, so a reference checkpoint loads with ``strict=True`` and one seed builds a
bit-identical ``state_dict``.

``SwinTransformerBlock`` on CUDA fp32 with head_dim 32 runs norm1 -> qkv Linear on the REAL rows -> ``window_attention`` (one
HIP launch, ``functions/swin_func.py``) -> proj on the real rows: no pad, roll, partition, reverse or crop tensors, no score
tensor, and the Linears skip the padded rows (a padded token's qkv is exactly qkv.bias).  ``BasicLayer`` then passes its blocks
``OWN_SHIFT_MASK`` instead of the mask tensor and builds the reference's mask only when a block takes the composition (CPU,
autocast, other dtypes, head_dim != 32, attention dropout in training, a qk_scale override, ``MSDA_SWIN_FUSED=0``).  A block
handed a mask tensor of its caller's takes the composition with that mask.  The MLP, LayerNorms and GEMMs stay on torch.

``MSDA_SWIN_GLUE=1`` (opt-in, read at call time, default off; ``functions/swin_glue_func.py``) moves the memory-bound glue of
such a block to HIP as well: norm1, shortcut + drop_path with norm2 in one launch, and the closing x + drop_path; PatchMerging's
pad / gather / concatenation / norm in one launch; the per-stage output norms.  The drop-path tensor stays torch's own draw.
With ``MSDA_SWIN_GLUE_BF16=1`` as well, the bfloat16 residual stream of stages 1 to 3 under bf16 autocast takes the same nodes."""
import math
from typing import List

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

from ..functions.swin_func import fused_route, shift_mask, window_attention, window_partition, window_reverse
from ..functions.swin_glue_func import (add_norm_rows, add_rows, affine_layernorm, draw_keep, glue_route, merge_norm,
                                        norm_rows)
from .detr import NestedTensor

__all__ = ["Mlp", "WindowAttention", "SwinTransformerBlock", "PatchMerging", "BasicLayer", "PatchEmbed", "SwinTransformer",
           "build_swin_transformer", "PositionEmbeddingSine", "Joiner", "build_backbone", "DropPath", "OWN_SHIFT_MASK"]

trunc_normal_ = nn.init.trunc_normal_                   # timm's trunc_normal_: the same algorithm


def to_2tuple(x):
    """timm.models.layers.to_2tuple."""
    if isinstance(x, (list, tuple)):
        return tuple(x)
    return (x, x)


def drop_path(x, drop_prob: float = 0., training: bool = False, scale_by_keep: bool = True):
    """timm's drop_path: per-sample stochastic depth, bernoulli_(keep) then / keep."""
    if drop_prob == 0. or not training:
        return x
    keep_prob = 1 - drop_prob
    shape = (x.shape[0],) + (1,) * (x.ndim - 1)
    random_tensor = x.new_empty(shape).bernoulli_(keep_prob)
    if keep_prob > 0.0 and scale_by_keep:
        random_tensor.div_(keep_prob)
    return x * random_tensor


class DropPath(nn.Module):
    """timm.models.layers.DropPath."""

    def __init__(self, drop_prob: float = 0., scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, x):
        return drop_path(x, self.drop_prob, self.training, self.scale_by_keep)


class _OwnShiftMask:
    """What BasicLayer hands its blocks in place of the mask tensor when they compute the mask from coordinates."""

    def __repr__(self):
        return "OWN_SHIFT_MASK"


OWN_SHIFT_MASK = _OwnShiftMask()


class Mlp(nn.Module):
    """models/swin_transformer.py:17-35."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        x = self.fc1(x)
        x = self.act(x)
        x = self.drop(x)
        x = self.fc2(x)
        x = self.drop(x)
        return x


class WindowAttention(nn.Module):
    """models/swin_transformer.py:68-142.  ``forward(x, mask=None)`` on partitioned windows [B_, N, C]: without a mask the
    kernel's route treats them as B_ images of ws x ws with shift 0."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim = dim
        self.window_size = window_size  # Wh, Ww
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.relative_position_bias_table = nn.Parameter(
            torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        coords_h = torch.arange(self.window_size[0])
        coords_w = torch.arange(self.window_size[1])
        coords = torch.stack(torch.meshgrid([coords_h, coords_w], indexing="ij"))
        coords_flatten = torch.flatten(coords, 1)
        relative_coords = coords_flatten[:, :, None] - coords_flatten[:, None, :]
        relative_coords = relative_coords.permute(1, 2, 0).contiguous()
        relative_coords[:, :, 0] += self.window_size[0] - 1
        relative_coords[:, :, 1] += self.window_size[1] - 1
        relative_coords[:, :, 0] *= 2 * self.window_size[1] - 1
        relative_position_index = relative_coords.sum(-1)
        self.register_buffer("relative_position_index", relative_position_index)
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        trunc_normal_(self.relative_position_bias_table, std=.02)
        self.softmax = nn.Softmax(dim=-1)

    def fused_for(self, x):
        """True when this module's attention takes the HIP node for input x."""
        ws = self.window_size[0]
        return (self.window_size[0] == self.window_size[1] and fused_route(x.device, x.dtype, self.dim, self.num_heads, ws)
                and self.scale == (self.dim // self.num_heads) ** -0.5 and (self.attn_drop.p == 0 or not self.training))

    def attend_rows(self, x_rows, geometry):
        """norm1'd real rows [B*H*W, C] -> the proj Linear's output [B*H*W, C] through the kernel's route."""
        qkv = self.qkv(x_rows)
        out = window_attention(qkv, self.qkv.bias, self.relative_position_bias_table, geometry, self.relative_position_index)
        return self.proj_drop(self.proj(out))

    def forward(self, x, mask=None):
        B_, N, C = x.shape
        if mask is None and self.fused_for(x) and N == self.window_size[0] * self.window_size[1]:
            ws = self.window_size[0]
            geometry = (B_, ws, ws, C, self.num_heads, ws, 0)
            return self.attend_rows(x.reshape(B_ * N, C), geometry).view(B_, N, C)
        qkv = self.qkv(x).reshape(B_, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        q = q * self.scale
        attn = (q @ k.transpose(-2, -1))
        relative_position_bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(
            self.window_size[0] * self.window_size[1], self.window_size[0] * self.window_size[1], -1)
        relative_position_bias = relative_position_bias.permute(2, 0, 1).contiguous()
        attn = attn + relative_position_bias.unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            attn = attn.view(B_ // nW, nW, self.num_heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, self.num_heads, N, N)
            attn = self.softmax(attn)
        else:
            attn = self.softmax(attn)
        attn = self.attn_drop(attn)
        x = (attn @ v).transpose(1, 2).reshape(B_, N, C)
        x = self.proj(x)
        x = self.proj_drop(x)
        return x


class SwinTransformerBlock(nn.Module):
    """models/swin_transformer.py:145-245."""

    def __init__(self, dim, num_heads, window_size=7, shift_size=0,
                 mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.num_heads = num_heads
        self.window_size = window_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(
            dim, window_size=to_2tuple(self.window_size), num_heads=num_heads,
            qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.H = None
        self.W = None

    def fused_for(self, x):
        return self.attn.fused_for(x)

    def forward(self, x, mask_matrix):
        B, L, C = x.shape
        H, W = self.H, self.W
        assert L == H * W, "input feature has wrong size"
        own_mask = mask_matrix is OWN_SHIFT_MASK
        if own_mask and self.fused_for(x) and self.glue_for(x):
            return self._forward_glue(x)
        if own_mask and self.fused_for(x):
            shortcut = x
            x = self.norm1(x)
            geometry = (B, H, W, C, self.num_heads, self.window_size, self.shift_size)
            x = self.attn.attend_rows(x.reshape(B * L, C), geometry).view(B, L, C)
        else:
            if own_mask:
                mask_matrix = shift_mask(H, W, self.window_size, self.shift_size, x.device) if self.shift_size > 0 else None
            shortcut = x
            x = self._attention_composition(x, mask_matrix)
        x = shortcut + self.drop_path(x)
        x = x + self.drop_path(self.mlp(self.norm2(x)))
        return x

    def glue_for(self, x):
        """True when this block's norms, residual adds and drop-path products take the HIP glue for input x (MSDA_SWIN_GLUE=1)."""
        C = x.shape[-1]
        return (glue_route(x.device, x.dtype, C) and affine_layernorm(self.norm1, C, x.device)
                and affine_layernorm(self.norm2, C, x.device) and isinstance(self.drop_path, (DropPath, nn.Identity)))

    def _keep(self, branch):
        """drop_path's per-sample tensor for this branch, drawn where and as ``self.drop_path(branch)`` draws it (None: identity)."""
        dp = self.drop_path
        if not isinstance(dp, DropPath):
            return None
        return draw_keep(branch, dp.drop_prob, dp.training, dp.scale_by_keep)

    def _forward_glue(self, x):
        """The fused branch of forward with the glue on HIP: norm -> attention -> add + norm -> MLP -> add."""
        B, L, C = x.shape
        geometry = (B, self.H, self.W, C, self.num_heads, self.window_size, self.shift_size)
        z = norm_rows(x, self.norm1)
        branch = self.attn.attend_rows(z.reshape(B * L, C), geometry).view(B, L, C)
        x, z = add_norm_rows(x, branch, self._keep(branch), self.norm2)
        branch = self.mlp(z)
        return add_rows(x, branch, self._keep(branch))

    def _attention_composition(self, x, mask_matrix):
        """models/swin_transformer.py:209-243: norm1, pad, roll, partition, W-MSA / SW-MSA, reverse, roll back, crop."""
        B, L, C = x.shape
        H, W = self.H, self.W
        x = self.norm1(x)
        x = x.view(B, H, W, C)
        pad_l = pad_t = 0
        pad_r = (self.window_size - W % self.window_size) % self.window_size
        pad_b = (self.window_size - H % self.window_size) % self.window_size
        x = F.pad(x, (0, 0, pad_l, pad_r, pad_t, pad_b))
        _, Hp, Wp, _ = x.shape
        if self.shift_size > 0:
            shifted_x = torch.roll(x, shifts=(-self.shift_size, -self.shift_size), dims=(1, 2))
            attn_mask = mask_matrix
        else:
            shifted_x = x
            attn_mask = None
        x_windows = window_partition(shifted_x, self.window_size)
        x_windows = x_windows.view(-1, self.window_size * self.window_size, C)
        attn_windows = self.attn(x_windows, mask=attn_mask)
        attn_windows = attn_windows.view(-1, self.window_size, self.window_size, C)
        shifted_x = window_reverse(attn_windows, self.window_size, Hp, Wp)
        if self.shift_size > 0:
            x = torch.roll(shifted_x, shifts=(self.shift_size, self.shift_size), dims=(1, 2))
        else:
            x = shifted_x
        if pad_r > 0 or pad_b > 0:
            x = x[:, :H, :W, :].contiguous()
        return x.view(B, H * W, C)


class PatchMerging(nn.Module):
    """models/swin_transformer.py:248-287."""

    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        if glue_route(x.device, x.dtype, 4 * C) and affine_layernorm(self.norm, 4 * C, x.device):
            return self.reduction(merge_norm(x, H, W, self.norm))
        x = x.view(B, H, W, C)
        pad_input = (H % 2 == 1) or (W % 2 == 1)
        if pad_input:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x0 = x[:, 0::2, 0::2, :]
        x1 = x[:, 1::2, 0::2, :]
        x2 = x[:, 0::2, 1::2, :]
        x3 = x[:, 1::2, 1::2, :]
        x = torch.cat([x0, x1, x2, x3], -1)
        x = x.view(B, -1, 4 * C)
        x = self.norm(x)
        x = self.reduction(x)
        return x


class BasicLayer(nn.Module):
    """models/swin_transformer.py:290-375.  The shift mask tensor is built only when a block takes the composition."""

    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0.,
                 attn_drop=0., drop_path=0., norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        self.window_size = window_size
        self.shift_size = window_size // 2
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(
                dim=dim,
                num_heads=num_heads,
                window_size=window_size,
                shift_size=0 if (i % 2 == 0) else window_size // 2,
                mlp_ratio=mlp_ratio,
                qkv_bias=qkv_bias,
                qk_scale=qk_scale,
                drop=drop,
                attn_drop=attn_drop,
                drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                norm_layer=norm_layer)
            for i in range(depth)])
        if downsample is not None:
            self.downsample = downsample(dim=dim, norm_layer=norm_layer)
        else:
            self.downsample = None

    def _mask_tensor(self, x, H, W):
        """The reference's attention mask for SW-MSA (:339-357)."""
        Hp = int(np.ceil(H / self.window_size)) * self.window_size
        Wp = int(np.ceil(W / self.window_size)) * self.window_size
        img_mask = torch.zeros((1, Hp, Wp, 1), device=x.device)
        h_slices = (slice(0, -self.window_size), slice(-self.window_size, -self.shift_size), slice(-self.shift_size, None))
        w_slices = (slice(0, -self.window_size), slice(-self.window_size, -self.shift_size), slice(-self.shift_size, None))
        cnt = 0
        for h in h_slices:
            for w in w_slices:
                img_mask[:, h, w, :] = cnt
                cnt += 1
        mask_windows = window_partition(img_mask, self.window_size)
        mask_windows = mask_windows.view(-1, self.window_size * self.window_size)
        attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
        return attn_mask.masked_fill(attn_mask != 0, float(-100.0)).masked_fill(attn_mask == 0, float(0.0))

    def forward(self, x, H, W):
        if all(blk.fused_for(x) for blk in self.blocks):
            attn_mask = OWN_SHIFT_MASK
        else:
            attn_mask = self._mask_tensor(x, H, W)
        for blk in self.blocks:
            blk.H, blk.W = H, W
            if self.use_checkpoint:
                x = checkpoint.checkpoint(blk, x, attn_mask, use_reentrant=False)
            else:
                x = blk(x, attn_mask)
        if self.downsample is not None:
            x_down = self.downsample(x, H, W)
            Wh, Ww = (H + 1) // 2, (W + 1) // 2
            return x, H, W, x_down, Wh, Ww
        else:
            return x, H, W, x, H, W


class PatchEmbed(nn.Module):
    """models/swin_transformer.py:378-416."""

    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        patch_size = to_2tuple(patch_size)
        self.patch_size = patch_size
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        if norm_layer is not None:
            self.norm = norm_layer(embed_dim)
        else:
            self.norm = None

    def forward(self, x):
        _, _, H, W = x.size()
        if W % self.patch_size[1] != 0:
            x = F.pad(x, (0, self.patch_size[1] - W % self.patch_size[1]))
        if H % self.patch_size[0] != 0:
            x = F.pad(x, (0, 0, 0, self.patch_size[0] - H % self.patch_size[0]))
        x = self.proj(x)
        if self.norm is not None:
            Wh, Ww = x.size(2), x.size(3)
            x = x.flatten(2).transpose(1, 2)
            x = self.norm(x)
            x = x.transpose(1, 2).view(-1, self.embed_dim, Wh, Ww)
        return x


class SwinTransformer(nn.Module):
    """models/swin_transformer.py:419-688 (forward takes a NestedTensor and returns {index: NestedTensor})."""

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=[2, 2, 6, 2],
                 num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0.2, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 out_indices=(0, 1, 2, 3), frozen_stages=-1, dilation=False, use_checkpoint=False):
        super().__init__()
        self.pretrain_img_size = pretrain_img_size
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.ape = ape
        self.patch_norm = patch_norm
        self.out_indices = out_indices
        self.frozen_stages = frozen_stages
        self.dilation = dilation
        self.patch_embed = PatchEmbed(
            patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
            norm_layer=norm_layer if self.patch_norm else None)
        if self.ape:
            pretrain_img_size = to_2tuple(pretrain_img_size)
            patch_size = to_2tuple(patch_size)
            patches_resolution = [pretrain_img_size[0] // patch_size[0], pretrain_img_size[1] // patch_size[1]]
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, patches_resolution[0], patches_resolution[1]))
            trunc_normal_(self.absolute_pos_embed, std=.02)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList()
        downsamplelist = [PatchMerging for i in range(self.num_layers)]
        downsamplelist[-1] = None
        num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        if self.dilation:
            downsamplelist[-2] = None
            num_features[-1] = int(embed_dim * 2 ** (self.num_layers - 1)) // 2
        for i_layer in range(self.num_layers):
            layer = BasicLayer(
                dim=num_features[i_layer],
                depth=depths[i_layer],
                num_heads=num_heads[i_layer],
                window_size=window_size,
                mlp_ratio=mlp_ratio,
                qkv_bias=qkv_bias,
                qk_scale=qk_scale,
                drop=drop_rate,
                attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i_layer]):sum(depths[:i_layer + 1])],
                norm_layer=norm_layer,
                downsample=downsamplelist[i_layer],
                use_checkpoint=use_checkpoint)
            self.layers.append(layer)
        self.num_features = num_features
        for i_layer in out_indices:
            layer = norm_layer(num_features[i_layer])
            layer_name = f'norm{i_layer}'
            self.add_module(layer_name, layer)
        self._freeze_stages()

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for param in self.patch_embed.parameters():
                param.requires_grad = False
        if self.frozen_stages >= 1 and self.ape:
            self.absolute_pos_embed.requires_grad = False
        if self.frozen_stages >= 2:
            self.pos_drop.eval()
            for i in range(0, self.frozen_stages - 1):
                m = self.layers[i]
                m.eval()
                for param in m.parameters():
                    param.requires_grad = False

    def forward_raw(self, x):
        """The stages' outputs [B, C_i, H_i, W_i] for the out_indices."""
        x = self.patch_embed(x)
        Wh, Ww = x.size(2), x.size(3)
        if self.ape:
            absolute_pos_embed = F.interpolate(self.absolute_pos_embed, size=(Wh, Ww), mode='bicubic')
            x = (x + absolute_pos_embed).flatten(2).transpose(1, 2)
        else:
            x = x.flatten(2).transpose(1, 2)
        x = self.pos_drop(x)
        outs = []
        for i in range(self.num_layers):
            layer = self.layers[i]
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            if i in self.out_indices:
                norm_layer = getattr(self, f'norm{i}')
                x_out = norm_rows(x_out, norm_layer, fp32_out=True)      # (norm_layer(x_out) unless MSDA_SWIN_GLUE=1)
                out = x_out.view(-1, H, W, self.num_features[i]).permute(0, 3, 1, 2).contiguous()
                outs.append(out)
        return tuple(outs)

    def forward(self, tensor_list: NestedTensor):
        outs = self.forward_raw(tensor_list.tensors)
        outs_dict = {}
        for idx, out_i in enumerate(outs):
            m = tensor_list.mask
            assert m is not None
            mask = F.interpolate(m[None].float(), size=out_i.shape[-2:]).to(torch.bool)[0]
            outs_dict[idx] = NestedTensor(out_i, mask)
        return outs_dict

    def train(self, mode=True):
        """Convert the model into training mode while keep layers freezed."""
        super(SwinTransformer, self).train(mode)
        self._freeze_stages()
        return self


_SWIN_CONFIGS = {
    'swin_T_224_1k': dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7),
    'swin_B_224_22k': dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=7),
    'swin_B_384_22k': dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=12),
    'swin_L_224_22k': dict(embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48], window_size=7),
    'swin_L_384_22k': dict(embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48], window_size=12),
}


def build_swin_transformer(modelname, pretrain_img_size, **kw):
    """models/swin_transformer.py:691-727."""
    assert modelname in ['swin_T_224_1k', 'swin_B_224_22k', 'swin_B_384_22k', 'swin_L_224_22k', 'swin_L_384_22k']
    kw_cgf = {k: (list(v) if isinstance(v, list) else v) for k, v in _SWIN_CONFIGS[modelname].items()}
    kw_cgf.update(kw)
    return SwinTransformer(pretrain_img_size=pretrain_img_size, **kw_cgf)


class PositionEmbeddingSine(nn.Module):
    """models/position_encoding.py:18-56."""

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        self.num_pos_feats = num_pos_feats
        self.temperature = temperature
        self.normalize = normalize
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        if scale is None:
            scale = 2 * math.pi
        self.scale = scale

    def forward(self, tensor_list: NestedTensor):
        x = tensor_list.tensors
        mask = tensor_list.mask
        assert mask is not None
        not_mask = ~mask
        y_embed = not_mask.cumsum(1, dtype=torch.float32)
        x_embed = not_mask.cumsum(2, dtype=torch.float32)
        if self.normalize:
            eps = 1e-6
            y_embed = (y_embed - 0.5) / (y_embed[:, -1:, :] + eps) * self.scale
            x_embed = (x_embed - 0.5) / (x_embed[:, :, -1:] + eps) * self.scale
        dim_t = torch.arange(self.num_pos_feats, dtype=torch.float32, device=x.device)
        dim_t = self.temperature ** (2 * (dim_t // 2) / self.num_pos_feats)
        pos_x = x_embed[:, :, :, None] / dim_t
        pos_y = y_embed[:, :, :, None] / dim_t
        pos_x = torch.stack((pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos_y = torch.stack((pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos = torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)
        return pos


class Joiner(nn.Sequential):
    """models/backbone.py Joiner: (features sorted by key, their position encodings)."""

    def __init__(self, backbone, position_embedding):
        super().__init__(backbone, position_embedding)
        if backbone.__class__.__name__ != 'SwinTransformer':
            self.strides = backbone.strides
            self.num_channels = backbone.num_channels
        else:
            self.strides = [8, 16, 32]
            self.num_channels = [384, 768, 1536]

    def forward(self, tensor_list: NestedTensor):
        xs = self[0](tensor_list)
        out: List[NestedTensor] = []
        pos = []
        for name, x in sorted(xs.items()):
            out.append(x)
        for x in out:
            pos.append(self[1](x).to(x.tensors.dtype))
        return out, pos


def build_backbone(args):
    """models/backbone.py build_backbone, Swin branch, with build_position_encoding's sine encoding."""
    if args.position_embedding not in ('v2', 'sine'):
        raise ValueError("only the sine position encoding is provided (%r)" % (args.position_embedding,))
    position_embedding = PositionEmbeddingSine(args.hidden_dim // 2, normalize=True)
    if args.backbone not in _SWIN_CONFIGS:
        raise ValueError("only the Swin backbones are provided (%r)" % (args.backbone,))
    pretrain_img_size = int(args.backbone.split('_')[-2])
    backbone = build_swin_transformer(args.backbone, pretrain_img_size=pretrain_img_size, out_indices=(1, 2, 3),
                                      dilation=args.dilation, use_checkpoint=True)
    return Joiner(backbone, position_embedding)
