"""DINO's contrastive-denoising query preparation (UVHand models/dino/dn_components.py):

  * ``cdn_attention_mask``            the decoder self-attention mask (:125-137) from ``arange`` comparisons;
  * ``prepare_for_cdn``               drop-in for the reference's function (:20-150): the noised label embeddings and the
    un-sigmoided keypoints of every denoising row in ONE launch of the library (csrc/msda_cdn.hip), with no host sync and
    capturable in a graph, the label embedding trained through it by a one-launch, atomic-free backward;
  * ``prepare_for_cdn_composition``   the reference's structure in torch ops with torch's generator, on any device: the route
    of everything the kernels do not take, and — with ``draws=`` — the kernels' oracle;
  * ``cdn_draws``                     the kernels' random draws restated in integer torch ops;
  * ``cdn_group_arithmetic``          the host arithmetic of :46-58 and :79-81;
  * ``dn_post_process``               the reference's split of the heads' outputs (:153-200), views only.

Two facts of the reference that the drop-in keeps.  The counts are host data: ``targets['labels']`` is a list of per-frame
Python lists, so ``single_pad``, the group count and every shape are known without reading the device (the reference reads
them back, :49-54, :79).  And the key noise is dead: :94-103 compute ``known_key_``, but the two lines that would write it
back (:104-105) are commented out and :109 embeds the un-noised clone, so ``input_query_key`` is ``inverse_sigmoid(keys)``
replicated and ``box_noise_scale`` has no effect on any output; the only live randomness is the label flip (:74-78)."""
from typing import NamedTuple, Optional

import torch
from torch import nn

_M32 = 0xFFFFFFFF


def cdn_attention_mask(single_pad, dn_number, num_queries, device=None):
    """The boolean decoder self-attention mask of models/dino/dn_components.py:125-137, True = the key is hidden:
    ``[pad + num_queries, pad + num_queries]`` with ``pad = 2 * single_pad * dn_number`` denoising rows in front of the matching
    queries.  ``single_pad`` is the largest target count of a frame, ``dn_number`` the number of denoising groups AFTER the
    reference's own division (its ``dn_meta['num_dn_group']``).  Matching queries see no denoising row, and a denoising row sees
    its own group (``2 * single_pad`` rows: positives and negatives) and every matching query:

        mask[i, j] = j < pad and (i >= pad or i // (2 * single_pad) != j // (2 * single_pad))

    Built from ``arange`` comparisons on ``device``: no loop over the groups, nothing read back."""
    single_pad, dn_number, num_queries = int(single_pad), int(dn_number), int(num_queries)
    if single_pad < 0 or dn_number < 0 or num_queries < 0:
        raise ValueError("cdn_attention_mask: single_pad, dn_number and num_queries must not be negative")
    group = 2 * single_pad
    pad = group * dn_number
    idx = torch.arange(pad + num_queries, device=device)
    gid = torch.div(idx, max(group, 1), rounding_mode="floor")
    i, j = idx[:, None], idx[None, :]
    return (j < pad) & ((i >= pad) | (gid[:, None] != gid[None, :]))


def cdn_group_arithmetic(sizes, dn_number):
    """(single_pad, groups) of :46-58 and :79 from the host's per-frame target counts: ``dn_number`` is doubled, divided by
    ``2 * max(sizes)`` only when the doubled number is at least 100, and floored to 1; a step without any target has one group.
    ``pad_size = 2 * single_pad * groups``; the targets are repeated ``2 * groups`` times."""
    single_pad = max(sizes, default=0)
    groups = int(dn_number) * 2
    if single_pad == 0:
        groups = 1
    elif groups >= 100:
        groups = groups // (single_pad * 2)
    elif groups < 1:
        groups = 1
    if groups == 0:
        groups = 1
    return single_pad, groups


class CdnDraws(NamedTuple):
    """The draws of one step over E = 2 * groups * T flat elements (element e = repetition * T + target)."""
    flip: torch.Tensor                   # [E] bool: the label is replaced
    new_label: torch.Tensor              # [E] int64 in [0, num_classes)
    sign: Optional[torch.Tensor]         # [E, W] fp32 in {-1, +1}, or None without key noise
    magnitude: Optional[torch.Tensor]    # [E, W] fp32 in [0, 1)


def cdn_draws(seed, E, W, num_classes, label_noise_ratio, key_noise=False):
    """The draws of ``prepare_for_cdn``'s kernel for ``seed`` (an int, or a one-element int64 tensor on any device: the draws are
    made there, without a host read): the restatement of its counter hash (at_mix / at_hash, csrc/msda_attn_tile.h) in integer
    torch ops.  With base = mix(seed, 0): element e flips iff hash(base + 2e) < min(2^32 - 1, floor(ratio * 0.5 * 2^32)), to the
    label (hash(base + 2e + 1) * num_classes) >> 32; with ``key_noise`` column c of element e has the counters
    k = 2E + 2 (e W + c): sign = +1 iff bit 31 of hash(base + k), magnitude = (hash(base + k + 1) >> 8) * 2^-24."""
    from .. import _native as MSDA
    dev = seed.device if torch.is_tensor(seed) else torch.device("cpu")
    s = seed.reshape(()).to(torch.int64) if torch.is_tensor(seed) else torch.tensor(
        (int(seed) & 0xFFFFFFFFFFFFFFFF) - (1 << 64 if int(seed) & (1 << 63) else 0), dtype=torch.int64)
    mix = ((s & _M32) + ((s >> 32) & _M32) * 0x85EBCA6B) & _M32

    def hashed(counter):
        x = (counter + mix) & _M32
        x = ((x ^ (x >> 16)) * 0x85EBCA6B) & _M32
        return ((x ^ (x >> 13)) * 0xC2B2AE35) & _M32

    e = torch.arange(int(E), dtype=torch.int64, device=dev)
    flip = hashed(2 * e) < MSDA.cdn_flip_threshold(label_noise_ratio)
    new_label = (hashed(2 * e + 1) * int(num_classes)) >> 32
    if not key_noise:
        return CdnDraws(flip, new_label, None, None)
    k = 2 * int(E) + 2 * torch.arange(int(E) * int(W), dtype=torch.int64, device=dev)
    sign = torch.where((hashed(k) >> 31) != 0, 1.0, -1.0).to(torch.float32).view(int(E), int(W))
    magnitude = ((hashed(k + 1) >> 8).to(torch.float32) * 2.0 ** -24).view(int(E), int(W))
    return CdnDraws(flip, new_label, sign, magnitude)


def _host_sizes(targets):
    return tuple(len(l) for l in targets["labels"])


def _key_width(targets, packed):
    if packed is not None and packed.keypoints is not None:
        return int(packed.keypoints.shape[-1])
    for k in targets["keypoints"]:
        if torch.is_tensor(k) and k.dim() == 2:
            return int(k.shape[-1])
    return 42                                                    # :112: the reference's padding rows are 42 wide


def _pack(targets, device):
    from ..matcher import pack_targets
    if "is_valid" not in targets:                                # pack_targets reads it; this function does not
        targets = dict(targets, is_valid=torch.ones(len(targets["labels"]), dtype=torch.int32))
    return pack_targets(targets, device)


def prepare_for_cdn_composition(dn_args, training, num_queries, num_classes, hidden_dim, label_enc, *, packed=None, key_noise=False,
                                draws=None):
    """``prepare_for_cdn`` (dn_components.py:20-150) in the reference's own structure and torch ops, on the device of
    ``label_enc``'s weight, with torch's generator: the same draws in the same order — the dead key-noise draws of :97-98
    included, so the generator ends in the reference's state.  The route of CPU tensors, other dtypes, autocast, hooks, special
    embeddings and sizes the kernels do not take.  ``key_noise=True`` writes the noised keys back (what :104-105 would have
    done); ``draws`` (a ``CdnDraws``) replaces the generator's draws, which makes this the kernels' oracle.  The zero padding
    has the embedding's dtype (fp32 in the reference, :111-112) and the keys' width (42 there)."""
    if not training:
        return None, None, None, None
    from ..functions.dino_func import inverse_sigmoid
    targets, dn_number, label_noise_ratio, box_noise_scale = dn_args
    device = label_enc.weight.device
    sizes = tuple(packed.sizes) if packed is not None else _host_sizes(targets)
    single_pad, groups = cdn_group_arithmetic(sizes, dn_number)
    B, T, W = len(sizes), sum(sizes), _key_width(targets, packed)
    if packed is not None and T:
        labels, keys = packed.labels.to(device), packed.keypoints.to(device)
    else:
        labels = torch.tensor([int(x) for l in targets["labels"] for x in l], dtype=torch.int64, device=device)
        keys = (torch.cat([torch.as_tensor(k).to(device).reshape(-1, W) for k in targets["keypoints"]]) if B
                else torch.zeros((0, W), device=device))
    batch_idx = torch.cat([torch.full((n,), i, dtype=torch.int64, device=device) for i, n in enumerate(sizes)]) if B \
        else labels.new_zeros(0)
    reps = 2 * groups

    known_labels = labels.repeat(reps, 1).view(-1)                                       # :67-72
    known_bid = batch_idx.repeat(reps, 1).view(-1)
    known_keys = keys.repeat(reps, 1)
    known_labels_expaned = known_labels.clone()
    known_key_expand = known_keys.clone()

    if label_noise_ratio > 0:                                                            # :74-78
        if draws is None:
            p = torch.rand_like(known_labels_expaned.float())
            chosen_indice = torch.nonzero(p < (label_noise_ratio * 0.5)).view(-1)
            new_label = torch.randint_like(chosen_indice, 0, num_classes)
            known_labels_expaned.scatter_(0, chosen_indice, new_label)
        else:
            known_labels_expaned = torch.where(draws.flip, draws.new_label, known_labels_expaned)
    pad_size = 2 * single_pad * groups                                                   # :79-85
    positive_idx = (torch.arange(T, device=device)[None, :] + (torch.arange(groups, device=device) * T * 2)[:, None]).flatten()
    negative_idx = positive_idx + T
    if box_noise_scale > 0 and (draws is None or draws.sign is not None):                # :86-103
        if draws is None:
            rand_sign = torch.randint_like(known_keys, low=0, high=2, dtype=torch.float32) * 2.0 - 1.0
            rand_part = torch.rand_like(known_keys)
        else:
            rand_sign, rand_part = draws.sign, draws.magnitude.clone()
        rand_part[negative_idx] += 1.0
        rand_part *= rand_sign
        known_key_ = known_keys + torch.mul(rand_part, known_key_expand) * box_noise_scale
        known_key_ = known_key_.clamp(min=0.0, max=1.0)
        if key_noise:
            known_key_expand = known_key_

    input_label_embed = label_enc(known_labels_expaned.long())                           # :107-109
    input_key_embed = inverse_sigmoid(known_key_expand)
    input_query_label = torch.zeros((B, pad_size, hidden_dim), dtype=input_label_embed.dtype, device=device)
    input_query_key = torch.zeros((B, pad_size, W), dtype=input_key_embed.dtype, device=device)
    if T:                                                                                # :117-123
        map_known_indice = torch.cat([torch.arange(n, device=device) for n in sizes])
        map_known_indice = torch.cat([map_known_indice + single_pad * i for i in range(reps)]).long()
        input_query_label[(known_bid, map_known_indice)] = input_label_embed
        input_query_key[(known_bid, map_known_indice)] = input_key_embed

    attn_mask = cdn_attention_mask(single_pad, groups, num_queries, device=device)       # :125-137
    return input_query_label, input_query_key, attn_mask, {"pad_size": pad_size, "num_dn_group": groups}


def _check_labels(targets, num_classes, rows):
    if num_classes > rows:
        raise IndexError("prepare_for_cdn: num_classes %d exceeds label_enc's %d rows" % (num_classes, rows))
    for frame in targets["labels"]:
        for x in frame:
            if not 0 <= int(x) < rows:
                raise IndexError("prepare_for_cdn: label %d is outside label_enc's %d rows" % (int(x), rows))


def cdn_fusable(label_enc, hidden_dim, keypoints, width, n_frames, n_targets, single_pad, groups):
    """The kernels apply: a plain fp32 CUDA ``nn.Embedding`` (no max_norm, padding_idx, sparse or frequency-scaled gradient, no
    hook), no autocast, fp32 keypoints on its device, and sizes inside ``msda_cdn_supported``."""
    from .. import _native as MSDA
    from ..functions import cdn_func
    from ..functions.two_stage_func import _has_hooks
    w = getattr(label_enc, "weight", None)
    if not (cdn_func.FUSED and type(label_enc) is nn.Embedding and label_enc.max_norm is None and label_enc.padding_idx is None
            and not label_enc.sparse and not label_enc.scale_grad_by_freq and not torch.is_autocast_enabled()):
        return False
    if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.data_ptr() % 16 == 0 and w.shape[1] == hidden_dim
            and not _has_hooks(label_enc)):
        return False
    if any(not (torch.is_tensor(k) and k.is_cuda and k.dtype == torch.float32 and k.device == w.device) for k in keypoints):
        return False
    pad = 2 * single_pad * groups
    return (MSDA.cdn_supported(hidden_dim, width, w.shape[0], 2 * groups * n_targets) and groups * n_targets < (1 << 30)
            and n_frames * pad * max(hidden_dim, width) < (1 << 31))


def prepare_for_cdn(dn_args, training, num_queries, num_classes, hidden_dim, label_enc, *, packed=None, key_noise=False):
    """Drop-in for models/dino/dn_components.py:20-150 with the reference's signature and return:
    ``(input_query_label [B, pad, hidden_dim], input_query_key [B, pad, W], attn_mask, dn_meta)`` with ``dn_meta`` =
    ``{'pad_size', 'num_dn_group'}`` as Python ints; four ``None`` when not ``training``.  ``dn_args`` = (targets, dn_number,
    label_noise_ratio, box_noise_scale), ``targets`` the reference's dict of per-frame ``labels`` lists and ``keypoints``
    tensors.  Row ``r * single_pad + j`` of frame b is that frame's j-th target in repetition r of ``2 * groups`` (even r
    positive, odd r negative, :82-85); the other rows are zero.  ``attn_mask`` is ``cdn_attention_mask``.

    On fp32 CUDA tensors the two outputs come from ONE launch and ``label_enc.weight`` gets its gradient from ONE more, summed in
    a fixed order (bitwise reproducible); nothing reads the device: the counts come from the host lists (the reference's
    :49-54 and :79 read them back), and the label flips of :74-78 are drawn from the library's counter hash of a seed that is
    one ``random_()`` on a device scalar — reproducible under ``manual_seed``, capturable in a graph, NOT torch's random stream
    (``cdn_draws`` restates them).  A step without any target launches nothing and returns empty ``[B, 0, .]`` tensors.
    ``packed``: the ``PackedTargets`` the criterion already made of the same targets (otherwise ``pack_targets`` is called).

    ``key_noise=False`` is the reference's behaviour: ``box_noise_scale`` is accepted and has NO effect on any output, because
    :104-105, which would write the noise of :94-103 back, are commented out and :109 embeds the un-noised keys.
    ``key_noise=True`` applies that noise: key + (u + [negative row]) * sign * key * box_noise_scale, clamped to [0, 1].

    A label outside ``label_enc``'s rows, or ``num_classes`` beyond them, raises IndexError before anything is launched.
    Everything else the kernels do not take (CPU tensors, other dtypes, autocast, hooks on ``label_enc``, max_norm / padding_idx
    / sparse embeddings, sizes outside ``msda_cdn_supported``, ``MSDA_CDN_FUSED=0``) runs ``prepare_for_cdn_composition``."""
    if not training:
        return None, None, None, None
    targets, dn_number, label_noise_ratio, box_noise_scale = dn_args
    sizes = tuple(packed.sizes) if packed is not None else _host_sizes(targets)
    single_pad, groups = cdn_group_arithmetic(sizes, dn_number)
    B, T, W = len(sizes), sum(sizes), _key_width(targets, packed)
    keypoints = [packed.keypoints] if packed is not None and packed.keypoints is not None else list(targets["keypoints"])
    _check_labels(targets, int(num_classes), label_enc.weight.shape[0])
    if not cdn_fusable(label_enc, hidden_dim, keypoints, W, B, T, single_pad, groups):
        return prepare_for_cdn_composition(dn_args, training, num_queries, num_classes, hidden_dim, label_enc, packed=packed,
                                           key_noise=key_noise)
    from ..functions.cdn_func import cdn_prepare
    weight = label_enc.weight
    pad_size = 2 * single_pad * groups
    if pad_size == 0:
        input_query_label, input_query_key = weight.new_zeros((B, 0, hidden_dim)), weight.new_zeros((B, 0, W))
    else:
        if packed is None:
            packed = _pack(targets, weight.device)
        input_query_label, input_query_key = cdn_prepare(
            weight, packed.labels, packed.offsets, packed.keypoints, single_pad, groups, num_classes, label_noise_ratio,
            box_noise_scale if key_noise else 0.0)[:2]
    attn_mask = cdn_attention_mask(single_pad, groups, num_queries, device=weight.device)
    return input_query_label, input_query_key, attn_mask, {"pad_size": pad_size, "num_dn_group": groups}


def dn_post_process(outputs_class, hand_coord, obj_coord, mano_param, cam_param, obj_param, dn_meta, aux_loss, _set_aux_loss):
    """dn_components.py:153-200: with denoising rows in front (``dn_meta['pad_size'] > 0``) every head output
    [layers, B, pad + queries, .] is split at ``pad_size``; the denoising part goes into
    ``dn_meta['output_known_lbs_bboxes']`` (last layer, plus ``aux_outputs`` from ``_set_aux_loss`` when ``aux_loss``) and the
    matching part is returned.  Slices only: every tensor is a view of its input."""
    if dn_meta and dn_meta["pad_size"] > 0:
        pad = dn_meta["pad_size"]
        singles, pairs = (outputs_class, hand_coord, obj_coord), (mano_param, cam_param, obj_param)
        known = [t[:, :, :pad, :] for t in singles] + [[p[0][:, :, :pad, :], p[1][:, :, :pad, :]] for p in pairs]
        rest = [t[:, :, pad:, :] for t in singles] + [[p[0][:, :, pad:, :], p[1][:, :, pad:, :]] for p in pairs]
        out = {"pred_logits": known[0][-1], "pred_hand_key": known[1][-1], "pred_obj_key": known[2][-1],
               "pred_mano_params": [known[3][0][-1], known[3][1][-1]],
               "pred_cams": [known[4][0][-1], known[4][1][-1]],
               "pred_obj_params": [known[5][0][-1], known[5][1][-1]]}
        if aux_loss:
            out["aux_outputs"] = _set_aux_loss(*known)
        dn_meta["output_known_lbs_bboxes"] = out
        outputs_class, hand_coord, obj_coord, mano_param, cam_param, obj_param = rest
    return outputs_class, hand_coord, obj_coord, mano_param, cam_param, obj_param
