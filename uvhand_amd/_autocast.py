"""``MSDA_SMALL_LOSS_BF16=1`` (read at call time, off by default): the ARCTIC small-loss nodes under bf16 autocast.

``get_arctic_item``, ``mano_many``, ``objects_many`` and ``small_loss_many`` call the C ABI directly, so autocast does not touch
their arithmetic; with the knob off they still send every autocast region to their torch restatements, as before the knob
existed.  With it on, bf16 autocast alone no longer does (fp16 autocast still does), and ``get_arctic_item`` takes bf16
sources."""
import os

import torch

from .functions.linear_func import _autocast_dtype


def small_loss_bf16_enabled():
    return os.environ.get("MSDA_SMALL_LOSS_BF16", "0") not in ("", "0")


def bf16_autocast():
    return torch.is_autocast_enabled() and _autocast_dtype() == torch.bfloat16


def autocast_refuses():
    """Whether the current autocast state sends a small-loss node to its restatement."""
    return torch.is_autocast_enabled() and not (small_loss_bf16_enabled() and _autocast_dtype() == torch.bfloat16)


def no_autocast():
    """The context the Python glue between the nodes runs in: no torch op in it is autocast."""
    return torch.autocast("cuda", enabled=False)
