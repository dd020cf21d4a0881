"""The input-projection neck of DeformableDETR.forward (models/actic_detr.py:191-225, models/assembly_detr.py:145-171): per
feature level ``Conv2d`` -> ``GroupNorm(32, hidden)`` -> (ARCTIC training) ``* (uniform > 0.3)``.

``input_proj_levels`` runs the convolutions as ``F.conv2d(x, weight, bias=None)`` and everything after them, for all levels
of the call, as one autograd node (``csrc/msda_neck.hip``): one HIP launch forward, two backward, no host synchronisation.
The conv bias moves into the kernel, which also returns its gradient; the node hands ``dy`` back and autograd carries it
through the convolution.  It retains the conv outputs, the group statistics and a one-byte-per-element mask — not the
normalised output and not the uniforms.

Everything else runs ``input_proj_levels_reference``, the literal composition in plain torch ops (any dtype, every
gradient): CPU tensors, dtypes other than fp32, active autocast, ``GroupNorm`` without affine, levels that disagree on batch
size / hidden size / groups / eps, more than 8 levels, and ``MSDA_NECK_FUSED=0`` (A/B knob)."""
import os

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import _native

THRESHOLD = 0.3                     # models/actic_detr.py:200,219: keep where uniform > 0.3


def _conv_tensors(conv):
    """(weight, bias, stride, padding, dilation, groups) of an nn.Conv2d, or the same tuple passed through."""
    if isinstance(conv, torch.nn.Module):
        if conv.padding_mode != "zeros" or isinstance(conv.padding, str):
            raise ValueError("input_proj_levels: Conv2d with zero padding given as numbers")
        return conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups
    return conv


def _norm_tensors(norm):
    """(num_groups, weight, bias, eps) of an nn.GroupNorm, or the same tuple passed through."""
    if isinstance(norm, torch.nn.Module):
        return norm.num_groups, norm.weight, norm.bias, norm.eps
    return norm


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def output_shapes(xs, convs):
    """[N, C, H_l, W_l] of every level's projection, from the conv arithmetic alone (what the uniforms are drawn for)."""
    shapes = []
    for x, conv in zip(xs, convs):
        w, _, stride, padding, dilation, _ = _conv_tensors(conv)
        hw = [(x.shape[2 + i] + 2 * _pair(padding)[i] - _pair(dilation)[i] * (w.shape[2 + i] - 1) - 1) // _pair(stride)[i] + 1
              for i in range(2)]
        shapes.append((x.shape[0], w.shape[0], hw[0], hw[1]))
    return shapes


def input_proj_levels_reference(xs, convs, norms, uniforms=None):
    """The reference's composition per level: conv with bias, F.group_norm, ``* (u > 0.3)``."""
    outs = []
    for l, (x, conv, norm) in enumerate(zip(xs, convs, norms)):
        w, b, stride, padding, dilation, groups = _conv_tensors(conv)
        num_groups, gamma, beta, eps = _norm_tensors(norm)
        src = F.group_norm(F.conv2d(x, w, b, stride, padding, dilation, groups), num_groups, gamma, beta, eps)
        outs.append(src * (uniforms[l] > THRESHOLD) if uniforms is not None else src)
    return outs


class _NeckFunction(torch.autograd.Function):
    """outs = GroupNorm(y + bias) [* (u > 0.3)] for all levels: msda_neck_forward_f32 / msda_neck_backward_f32.
    apply(groups, eps, L, masked, *ys, *biases, *gammas, *betas, *uniforms); a missing bias is None."""

    @staticmethod
    def forward(ctx, groups, eps, L, masked, *tensors):
        ys = [t.contiguous() for t in tensors[:L]]
        biases = list(tensors[L:2 * L])
        gammas = list(tensors[2 * L:3 * L])
        betas = list(tensors[3 * L:4 * L])
        uniforms = [t.contiguous() for t in tensors[4 * L:5 * L]] if masked else None
        outs, means, rstds, masks = _native.neck_forward(ys, [b.contiguous() if b is not None else None for b in biases],
                                                         [g.contiguous() for g in gammas], [b.contiguous() for b in betas],
                                                         uniforms, groups, eps)
        ctx.groups, ctx.L, ctx.masked = groups, L, masked
        ctx.has_bias = [b is not None for b in biases]
        ctx.save_for_backward(*ys, *[b for b in biases if b is not None], *gammas, *means, *rstds, *(masks or []))
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outs):
        L = ctx.L
        saved = list(ctx.saved_tensors)
        ys, saved = saved[:L], saved[L:]
        nb = sum(ctx.has_bias)
        it = iter(saved[:nb])
        biases = [next(it).contiguous() if h else None for h in ctx.has_bias]
        saved = saved[nb:]
        gammas, means, rstds = saved[:L], saved[L:2 * L], saved[2 * L:3 * L]
        masks = saved[3 * L:4 * L] if ctx.masked else None
        gys, ggs, gbs, gcs = _native.neck_backward([g.contiguous() for g in grad_outs], ys, biases,
                                                   [g.contiguous() for g in gammas], means, rstds, masks, ctx.groups)
        return (None, None, None, None, *gys, *gcs, *ggs, *gbs, *([None] * L if ctx.masked else []))


def _fused_enabled():
    return os.environ.get("MSDA_NECK_FUSED", "1") != "0"     # A/B knob: 0 = the torch composition


def _fused_ok(xs, convs, norms, uniforms):
    """Whether the kernels take this call: fp32 CUDA everywhere, affine GroupNorms that agree on groups and eps."""
    if not (_fused_enabled() and 1 <= len(xs) <= _native.NECK_MAX_LEVELS) or torch.is_autocast_enabled():
        return False
    dev = xs[0].device
    tensors = list(xs) + list(uniforms or [])
    for conv, norm in zip(convs, norms):
        if norm[1] is None or norm[2] is None or (norm[0], norm[3]) != (norms[0][0], norms[0][3]):
            return False
        tensors += [conv[0], norm[1], norm[2]] + ([conv[1]] if conv[1] is not None else [])
    if not all(t.is_cuda and t.device == dev and t.dtype == torch.float32 for t in tensors):
        return False
    return all(x.dim() == 4 and x.shape[0] == xs[0].shape[0] and c[0].shape[0] == convs[0][0].shape[0]
               for x, c in zip(xs, convs))


def input_proj_levels(xs, convs, norms, uniforms=None):
    """Per level ``GroupNorm(conv(x))``, times ``(uniform > 0.3)`` where uniforms are given: a list of [N, C, H_l, W_l].

    xs: the conv inputs; convs, norms: the ``nn.Conv2d`` / ``nn.GroupNorm`` modules, or their tensors as
    ``(weight, bias, stride, padding, dilation, groups)`` and ``(num_groups, weight, bias, eps)``; uniforms: None, or one
    tensor of the projection's shape per level (``output_shapes``)."""
    xs, L = list(xs), len(xs)
    convs = [_conv_tensors(c) for c in convs]
    norms = [_norm_tensors(n) for n in norms]
    if not (len(convs) == len(norms) == L and (uniforms is None or len(uniforms) == L)):
        raise ValueError("input_proj_levels: one conv, one norm and (optionally) one uniform tensor per level")
    if not _fused_ok(xs, convs, norms, uniforms):
        return input_proj_levels_reference(xs, convs, norms, uniforms)
    ys = [F.conv2d(x, c[0], None, c[2], c[3], c[4], c[5]) for x, c in zip(xs, convs)]
    if (uniforms is not None and any(u.shape != y.shape for u, y in zip(uniforms, ys))) \
            or not _native.neck_supported(ys, norms[0][0]):
        return input_proj_levels_reference(xs, convs, norms, uniforms)
    outs = _NeckFunction.apply(norms[0][0], norms[0][3], L, uniforms is not None, *ys, *[c[1] for c in convs],
                               *[n[1] for n in norms], *[n[2] for n in norms], *(uniforms or []))
    return list(outs)
