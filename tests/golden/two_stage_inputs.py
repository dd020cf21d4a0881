"""Inputs and per-layer heads of the transformer fixtures (transformer_two_stage.npz / transformer_one_stage.npz), rebuilt
wherever they are needed instead of being stored: gen_golden_r06.py (which ran the reference on them) and
tests/test_transformer*.py (which run the product on them) call the same functions.  Inputs come from numpy's frozen legacy
RandomState stream, weights from torch.manual_seed at construction; `checksums` (stored in the fixtures) guards both.
Test infrastructure, no reference code."""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

# (name, d_model, heads, ffn, enc layers, dec layers, levels (H, W), N, queries, two_stage, weight seed)
CONFIGS = {
    "two_stage": dict(d=256, heads=8, ffn=1024, enc=6, dec=6, shapes=[(28, 28), (14, 14), (7, 7), (4, 4)], N=4, Q=300,
                      two_stage=True, wseed=606),
    "one_stage": dict(d=64, heads=2, ffn=128, enc=2, dec=2, shapes=[(8, 8), (4, 4), (2, 2), (1, 1)], N=2, Q=9,
                      two_stage=False, wseed=607),
}
N_CLASSES = 14
# What the fixtures keep of the large tensors (all rows are covered by fp64 row sums besides):
ROW_STEP = {"hs": 193}    # every 193rd row of hs [layers * N * Q, 256] (193 prime: the kept rows spread over layers / frames)
ROW_STEP_DEFAULT = 61     # every 61st row of the 42- / 14-wide outputs
MATCH_COLS = 4            # the leading columns of init_reference kept whole: they identify each selected query
GRAD_STRIDE = 389         # every 389th element of each input gradient
PGRAD_SAMPLES = 32        # seeded elements of every parameter gradient
CLS_SCALE = 50.0          # widens the class logits so that no selection / refinement decision sits within fp32 reach of a tie


class HeadMLP(nn.Module):
    """The model's 3-layer keypoint head: Linear -> ReLU -> Linear -> ReLU -> Linear."""

    def __init__(self, d_in, d_hidden, d_out, n_layers):
        super().__init__()
        self.n_layers = n_layers
        dims = [d_in] + [d_hidden] * (n_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims, dims[1:] + [d_out]))

    def forward(self, x):
        for i, lin in enumerate(self.layers):
            x = lin(x)
            if i + 1 < self.n_layers:
                x = F.relu(x)
        return x


def attach_heads(transformer, cfg, width):
    """cls_embed / key_embed / obj_key_embed on transformer.decoder, one per prediction (decoder layers + 1 when two-stage),
    each a copy of one head, as the model attaches them; drawn from torch.manual_seed(wseed + 1)."""
    import copy
    torch.manual_seed(cfg["wseed"] + 1)
    d = cfg["d"]
    n_pred = cfg["dec"] + (1 if cfg["two_stage"] else 0)
    cls = nn.Linear(d, N_CLASSES)
    with torch.no_grad():
        cls.bias.fill_(-math.log((1 - 0.01) / 0.01))
        cls.weight.mul_(CLS_SCALE)
    key, obj = HeadMLP(d, d, width, 3), HeadMLP(d, d, width, 3)
    for h in (key, obj):
        nn.init.xavier_uniform_(h.layers[-1].weight.data, gain=1)
        nn.init.constant_(h.layers[-1].bias.data, 0)
    dec = transformer.decoder
    dec.cls_embed = nn.ModuleList(copy.deepcopy(cls) for _ in range(n_pred))
    dec.key_embed = nn.ModuleList(copy.deepcopy(key) for _ in range(n_pred))
    dec.obj_key_embed = nn.ModuleList(copy.deepcopy(obj) for _ in range(n_pred))
    return dec.cls_embed, dec.key_embed, dec.obj_key_embed


def perturb(module, cfg, amount=0.02):
    """Move every parameter off its construction value (seeded): at construction sampling_offsets.weight is zero, so every
    sampling point sits exactly on a pixel centre, where bilinear interpolation has a kink and the location gradient is
    decided by fp32 rounding (tests/conftest.py near_boundary_mask) — a fixture must not sit on it.  Applied after the
    construction checksums are taken."""
    g = torch.Generator().manual_seed(cfg["wseed"] + 2)
    with torch.no_grad():
        for _, p in module.named_parameters():
            p.add_(torch.randn(p.shape, generator=g).to(p.device) * amount)


def inputs(cfg, seed):
    """srcs / pos_embeds [N, d, H, W] per level, masks [N, H, W] (frame 1 padded on the right / bottom, and a ragged
    first row so that the valid extent is not a rectangle), query_embed [Q, 2d] (one-stage), output gradients."""
    rs = np.random.RandomState(seed)
    N, d = cfg["N"], cfg["d"]
    srcs, poss, masks = [], [], []
    for (h, w) in cfg["shapes"]:
        srcs.append(rs.standard_normal((N, d, h, w)).astype(np.float32))
        poss.append(rs.standard_normal((N, d, h, w)).astype(np.float32))
        m = np.zeros((N, h, w), dtype=bool)
        if h > 1:
            m[1, :, w - max(1, w // 5):] = True
            m[1, h - max(1, h // 4):, :] = True
            m[0, 0, w - max(1, w // 7):] = True            # only the first row: the valid width is read off it
        masks.append(m)
    query = rs.standard_normal((cfg["Q"], 2 * d)).astype(np.float32)
    return dict(srcs=srcs, poss=poss, masks=masks, query=query, rs=rs)


def output_grads(cfg, seed, shapes):
    """Seeded gradients for the outputs of the given shapes (explicit, since the coordinate outputs hold +inf)."""
    rs = np.random.RandomState(seed + 1000)
    return [rs.standard_normal(s).astype(np.float32) for s in shapes]


def row_step(label, cfg):
    """Every row of the small one-stage fixture; a subsample of the two-stage one."""
    return ROW_STEP.get(label, ROW_STEP_DEFAULT) if cfg["two_stage"] else 1


def pgrad_index(seed, k, numel):
    """The seeded elements kept of the k-th parameter's gradient (regenerated by the tests, not stored)."""
    rs = np.random.RandomState(seed * 1000 + 2000 + k)
    return rs.randint(0, numel, size=min(PGRAD_SAMPLES, numel)).astype(np.int64)


def checksums(z):
    return np.asarray([float(np.float64(a).sum()) for a in z["srcs"] + z["poss"]] + [float(np.float64(z["query"]).sum())],
                      dtype=np.float64)


def state_checksums(module):
    """(names, fp64 sum, fp64 sum of squares, one element) of every state_dict entry."""
    names, sums = [], []
    for k, v in module.state_dict().items():
        a = v.detach().cpu().double().numpy().ravel()          # numpy's single-threaded pairwise sum: one summation order
        names.append(k)
        sums.append([float(np.sum(a)), float(np.sum(a * a)), float(a[a.size // 2]) if a.size else 0.0])
    return names, np.asarray(sums, dtype=np.float64)
