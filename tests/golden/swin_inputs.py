"""Seeded inputs of the Swin fixtures (gen_golden_r12.py) and of tests/test_swin*.py: two small backbones (window 7 and 12, an
image size that is not a multiple of 4, with a padding mask) and one Swin-L stage-2 BasicLayer on 14 x 14 tokens (the 24 x 24
padded geometry).  Shared by the generator and the tests, so nothing at test time reads the reference."""
import hashlib

import torch

# backbone cases: SwinTransformer(embed_dim, depths, num_heads, window_size, out_indices (1, 2, 3)) under Joiner with
# PositionEmbeddingSine(POS_FEATS, normalize=True); images [B, 3, H, W], image 1 padded on its right and bottom
BACKBONE_CASES = {
    "swin_w7": dict(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, B=2, H=62, W=78, seed=1201),
    "swin_w12": dict(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=12, B=2, H=62, W=78, seed=1202),
}
POS_FEATS = 16
# BasicLayer cases: dim, depth (one W-MSA and one SW-MSA block), heads, window; tokens [B, H * W, dim]
LAYER_CASES = {
    "swin_l_stage2": dict(dim=768, depth=2, num_heads=24, window_size=12, B=1, H=14, W=14, seed=1211),
}
GRAD_FULL = 4096                    # gradients with more elements are kept as sums over dim 0 and dim 1
LAYER_FULL_TOKENS = 16              # the layer case keeps its output and input gradient whole for the first tokens only


def build_backbone(swin_cls, joiner_cls, pos_cls, name):
    c = BACKBONE_CASES[name]
    torch.manual_seed(c["seed"])
    body = swin_cls(embed_dim=c["embed_dim"], depths=list(c["depths"]), num_heads=list(c["num_heads"]),
                    window_size=c["window_size"], drop_path_rate=0.0, out_indices=(1, 2, 3))
    return joiner_cls(body, pos_cls(POS_FEATS, normalize=True)).eval()


def backbone_input(name):
    c = BACKBONE_CASES[name]
    g = torch.Generator().manual_seed(c["seed"] + 1)
    img = torch.randn(c["B"], 3, c["H"], c["W"], generator=g)
    mask = torch.zeros(c["B"], c["H"], c["W"], dtype=torch.bool)
    mask[1, c["H"] - 13:, :] = True
    mask[1, :, c["W"] - 22:] = True
    img[1][:, mask[1]] = 0
    return img, mask


def build_layer(layer_cls, name):
    c = LAYER_CASES[name]
    torch.manual_seed(c["seed"])
    return layer_cls(dim=c["dim"], depth=c["depth"], num_heads=c["num_heads"], window_size=c["window_size"]).eval()


def layer_input(name):
    c = LAYER_CASES[name]
    g = torch.Generator().manual_seed(c["seed"] + 1)
    return torch.randn(c["B"], c["H"] * c["W"], c["dim"], generator=g)


def weighted_sum(outs, seed):
    g = torch.Generator().manual_seed(seed)
    total = 0
    for o in outs:
        total = total + (o * torch.randn(o.shape, generator=g).to(o.device)).sum()
    return total


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def store_grad(z, prefix, g):
    """A parameter gradient: whole when small, else its sums over dim 0 and dim 1 (dim 0 only for vectors)."""
    g = g.detach().cpu()
    if g.numel() <= GRAD_FULL:
        z[prefix + "grad/"] = g.numpy().copy()
    else:
        z[prefix + "gradsum0/"] = g.sum(0).numpy().copy()
        if g.dim() > 1:
            z[prefix + "gradsum1/"] = g.sum(1).numpy().copy()


def store_tokens(z, key, t):
    """A layer case's [1, L, C] tensor: the first LAYER_FULL_TOKENS tokens whole, and its sums over tokens and channels."""
    t = t.detach().cpu()
    z[key + "/head"] = t[:, :LAYER_FULL_TOKENS].numpy().copy()
    z[key + "/sum1"] = t.sum(1).numpy().copy()
    z[key + "/sum2"] = t.sum(2).numpy().copy()
