"""DINO's contrastive-denoising queries (UVHand models/dino/dn_components.py:20-150, prepare_for_cdn) on HIP (csrc/msda_cdn.hip,
include/msda.h) as ONE autograd node: the forward writes ``input_query_label`` [B, pad, H], ``input_query_key`` [B, pad, W] and
the noised labels in one launch, from the packed targets (``matcher.pack_targets``) and ``label_enc``'s weight; the backward is
the embedding's weight gradient in one launch with a fixed summation order (no atomics: bitwise reproducible).  Only the
weight gets a gradient: the reference's keypoints are targets.

The label flips (:74-78) — and, as an option, the key noise the reference computes and drops (:94-105) — are drawn from the
library's counter hash of a seed that is one ``random_()`` on a device scalar: reproducible under ``manual_seed``, capturable
in a graph, not torch's stream (``utils.denoising.cdn_draws`` restates it in integer torch ops)."""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as MSDA

FUSED = os.environ.get("MSDA_CDN_FUSED", "1") != "0"                # A/B knob: 0 = the reference's composition


class _CdnPrepareFn(Function):
    """(input_query_label, input_query_key, noised_labels [B, pad] int32[, the keys before inverse_sigmoid]) of the packed
    targets; gradient to ``weight`` alone.  Saved: the noised labels."""

    @staticmethod
    def forward(ctx, weight, labels, offsets, keypoints, seed, single_pad, groups, num_classes, flip_threshold, key_noise_scale,
                key_debug):
        outs = MSDA.cdn_prepare_forward(labels, offsets, keypoints, weight, seed, single_pad, groups, num_classes, flip_threshold,
                                        key_noise_scale, key_debug)
        ctx.save_for_backward(outs[2])
        ctx.rows_book = weight.shape[0]
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_label, *unused):
        if not ctx.needs_input_grad[0]:
            return (None,) * 11
        (noised,) = ctx.saved_tensors
        g = grad_label.contiguous()
        if g.data_ptr() % 16:                                           # a view at an odd offset: the kernel moves 16 bytes
            g = g.clone()
        return (MSDA.cdn_prepare_backward(g, noised, ctx.rows_book),) + (None,) * 10


def cdn_prepare(weight, labels, offsets, keypoints, single_pad, groups, num_classes, label_noise_ratio, key_noise_scale=0.0,
                seed=None, key_debug=False):
    """The node: ``weight`` [rows, H] (contiguous fp32 CUDA, 16-byte aligned), the packed ``labels`` / ``offsets`` /
    ``keypoints`` and the host counts.  ``seed`` (a one-element int64 CUDA tensor) is drawn with one ``random_()`` when draws are
    needed and none is given."""
    thr = MSDA.cdn_flip_threshold(label_noise_ratio)
    scale = max(0.0, float(key_noise_scale))
    if seed is None and (thr or scale > 0.0):
        seed = torch.empty(1, dtype=torch.int64, device=weight.device).random_()
    return _CdnPrepareFn.apply(weight, labels, offsets, keypoints, seed, int(single_pad), int(groups), int(num_classes), thr, scale,
                               bool(key_debug))
