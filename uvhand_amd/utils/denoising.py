"""Pieces of DINO's contrastive-denoising query preparation (models/dino/dn_components.py) that need no random draw."""
import torch


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
