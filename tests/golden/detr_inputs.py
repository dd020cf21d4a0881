"""Seeded inputs of the DeformableDETR fixtures (gen_golden_r10.py) and of tests/test_detr*.py: a stub transformer that returns
fixed hs / references / encoder outputs, stub backbones, and the cases.  Shared by the generator and the tests, so nothing at
test time reads the reference."""
import hashlib

import torch
from torch import nn

C = 256
# name: (model, two_stage, with_box_refine, dec_layers, frames (B * N), Q, K, R, seed)
CASES = {
    "arctic_refine": ("arctic", True, True, 3, 3, 7, 14, 42, 101),
    "arctic_one_stage": ("arctic", False, False, 2, 2, 9, 14, 42, 102),
    "assembly_2d": ("assembly", True, True, 3, 3, 5, 7, 2, 103),
    "assembly_42d": ("assembly", False, False, 2, 2, 11, 7, 42, 104),
}


class StubDecoder(nn.Module):
    def __init__(self, num_layers):
        super().__init__()
        self.num_layers = num_layers


class StubTransformer(nn.Module):
    """d_model, decoder.num_layers and a forward that returns the case's seeded (hs, init_reference, inter_references,
    enc_outputs_class, enc_outputs_hand_coord_unact, enc_outputs_obj_coord_unact).  hs is a leaf that requires grad."""

    def __init__(self, name):
        super().__init__()
        model, two_stage, _, L, B, Q, K, R, seed = CASES[name]
        self.d_model = C
        self.decoder = StubDecoder(L)
        g = torch.Generator().manual_seed(seed)
        self.hs = (torch.randn(L, B, Q, C, generator=g) * 0.5).requires_grad_(True)
        # references in [-1.2, 1.2]: ARCTIC's refined references lie in [-1, 1], so values below 0 clamp to 0 in
        # inverse_sigmoid; a few land inside (0, eps) and at exactly 0 / 1
        init = torch.rand(B, Q, R, generator=g) * 2.4 - 1.2
        inter = torch.rand(L, B, Q, R, generator=g) * 2.4 - 1.2
        if model == "assembly":
            init = init.abs().clamp(max=1)
        init.view(-1)[:3] = torch.tensor([0.0, 3e-6, 1.0])
        inter.view(-1)[:3] = torch.tensor([7e-6, -0.5, 0.999997])
        self.init_reference, self.inter_references = init, inter
        D = 42 if model == "arctic" else 63
        self.enc = (torch.randn(B, Q, K, generator=g), torch.randn(B, Q, D, generator=g), torch.randn(B, Q, D, generator=g))
        self.calls = []

    def forward(self, srcs, masks, pos, query_embeds):
        self.calls.append((len(srcs), query_embeds.shape))
        return (self.hs, self.init_reference, self.inter_references) + self.enc


class StubPosition(nn.Module):
    """backbone[1]: a position embedding of the source's shape."""

    def forward(self, nested):
        return nested.tensors * 0.5


class StubBackbone(nn.Module):
    """Joiner-like: backbone(samples) -> (features, pos), features NestedTensors; backbone[1] the position embedding."""

    def __init__(self, nested_cls, channels=(8, 16)):
        super().__init__()
        self.strides = [8, 16][:len(channels)]
        self.num_channels = list(channels)
        self.nested_cls = nested_cls
        self.pos = StubPosition()

    def __getitem__(self, i):
        return self.pos

    def forward(self, samples):
        x, m = samples.tensors, samples.mask
        feats, pos = [], []
        for i, ch in enumerate(self.num_channels):
            s = 2 ** (i + 1)
            f = x[:, :1, ::s, ::s].repeat(1, ch, 1, 1)
            mask = m[:, ::s, ::s]
            feats.append(self.nested_cls(f, mask))
            pos.append(torch.zeros(f.shape[0], C, f.shape[2], f.shape[3], device=f.device))
        return feats, pos


class Cfg:
    hand_idx = [0, 1]


def build(name, model_cls, nested_cls, seed=0):
    """The case's model from `model_cls` (the reference's DeformableDETR or a drop-in), built under `seed`."""
    model, two_stage, refine, L, B, Q, K, R, _ = CASES[name]
    torch.manual_seed(seed)
    tr = StubTransformer(name)
    if model == "arctic":
        return model_cls([None, StubPosition()], tr, K, Q, 2, aux_loss=True, with_box_refine=refine, two_stage=two_stage,
                         cfg=Cfg())
    return model_cls(StubBackbone(nested_cls), tr, K, Q, 2, aux_loss=True, with_box_refine=refine, two_stage=two_stage,
                     cfg=Cfg())


def samples(name, nested_cls):
    model, _, _, L, B, Q, K, R, seed = CASES[name]
    g = torch.Generator().manual_seed(seed + 1)
    if model == "arctic":                                   # local_fm: per level [B, N, C, W, H]
        return [torch.randn(1, B, C, 4, 4, generator=g), torch.randn(1, B, C, 2, 2, generator=g)]
    x = torch.randn(B, 3, 16, 16, generator=g)
    return nested_cls(x, torch.zeros(B, 16, 16, dtype=torch.bool))


def perturb(model, seed):
    """Seeded values for every head parameter (the init zeroes AssemblyHands' last keypoint layers, which would hide every
    gradient below them)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(model.named_parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)


def flatten_outputs(out, prefix=""):
    """[(path, tensor)] of the output dict in a fixed order."""
    items = []
    if isinstance(out, dict):
        for k in sorted(out):
            items += flatten_outputs(out[k], prefix + "/" + k)
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            items += flatten_outputs(v, "%s/%d" % (prefix, i))
    else:
        items.append((prefix, out))
    return items


def weighted_sum(out, seed):
    """A seeded weighted sum of every output that depends on the heads."""
    g = torch.Generator().manual_seed(seed)
    total = 0
    for path, t in flatten_outputs(out):
        if "interm_outputs" in path or "enc_outputs" in path or not t.requires_grad:
            continue
        w = torch.randn(t.shape, generator=g).to(t.device, t.dtype)
        total = total + (t * w).sum()
    return total


def digest(t):
    """sha256 of a tensor's bytes (bit identity of a constructed state_dict without storing it)."""
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
