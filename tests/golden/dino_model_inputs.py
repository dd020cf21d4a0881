"""Configuration, stub backbone, seeded parameters and inputs of the DINO model fixture (dino_model.npz), rebuilt wherever they
are needed instead of being stored: gen_dino_model.py (which ran the reference's DINO class on them) and tests/test_dino_model*.py
(which run the product on them) call the same functions.  Test infrastructure, no reference code."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from dino_inputs import ACT_BAR, GRAD_BAR, PGRAD_SAMPLES, _err, hold, set_parameters, ulp  # noqa: F401

# The fixture's size: 2 frames of 24 x 20 images (frame 1 padded on the right and at the bottom), a two-level stub backbone
# (6 x 5 and 3 x 3) plus one extra level (2 x 2): S = 43 rows; 10 queries, 14 classes, 2 decoder layers.  The hidden size is
# the transformer's only one: its decoder feeds a 2 x 128-wide sine table to ref_point_head, an MLP of d_model inputs.
CFG = dict(N=2, d=256, heads=8, ffn=32, enc_layers=1, dec_layers=2, image=(24, 20), valid=[(24, 20), (20, 15)], channels=(6, 10),
           levels=3, queries=10, K=14, points=2, dn_number=2, targets=[[1, 12], [13]])
# The smallest model the HIP routes take (head_dim 32): one backbone level (8 x 6) plus one extra level (4 x 3): S = 60.
GPU_CFG = dict(N=2, d=256, heads=8, ffn=64, enc_layers=1, dec_layers=2, image=(32, 24), valid=[(32, 24), (28, 19)], channels=(8,),
               levels=2, queries=20, K=14, points=4, dn_number=3, targets=[[1, 12, 3], [13, 2]], seed=7005)
# (seed 7005: the 21 largest row maxima of each frame lie at least 7e-3 apart and every class argmax leads by 7e-2, so fp32 and
# fp64 select the same rows and the same hands; frame 1's padded rows, which share one set of logits, are not among them)
# eval without targets; a training step with targets (label noise 0, dropout 0: nothing random); the same with the encoder's
# keypoint heads as copies of their own (two_stage_bbox_embed_share=False)
CASES = {"eval": dict(seed=6101, train=False, bbox_share=True),
         "train": dict(seed=6102, train=True, bbox_share=True),
         "train_own_enc_heads": dict(seed=6103, train=True, bbox_share=False)}


def _seed(case, cfg):
    return cfg.get("seed", CASES[case]["seed"])


INIT_SEED = 79                # torch.manual_seed before a bare construction (the seeded-initialisation sums)


class NestedTensor:
    """A batch of images and its padding mask (True on padded pixels)."""

    def __init__(self, tensors, mask):
        self.tensors = tensors
        self.mask = mask

    def decompose(self):
        return self.tensors, self.mask


class _Body(nn.Module):
    def __init__(self, channels):
        super().__init__()
        convs, c_in = [], 3
        for i, c in enumerate(channels):
            convs.append(nn.Conv2d(c_in, c, kernel_size=4, stride=4) if i == 0 else nn.Conv2d(c_in, c, kernel_size=3, stride=2, padding=1))
            c_in = c
        self.convs = nn.ModuleList(convs)


class _Position(nn.Module):
    """A parameter-free positional encoding read off the mask: sines of the normalised row and cosines of the normalised column
    of each valid pixel, one frequency per channel."""

    def __init__(self, d):
        super().__init__()
        self.d = d

    def forward(self, nt):
        keep = (~nt.mask).to(torch.float32)
        y = keep.cumsum(1) / keep.sum(1, keepdim=True).clamp_min(1.0).amax(2, keepdim=True)
        x = keep.cumsum(2) / keep.sum(2, keepdim=True).clamp_min(1.0).amax(1, keepdim=True)
        k = torch.arange(1, self.d // 2 + 1, dtype=torch.float32, device=keep.device)[None, :, None, None]
        return torch.cat([torch.sin(y[:, None] * k), torch.cos(x[:, None] * k)], 1)


class StubBackbone(nn.Sequential):
    """What the model asks of a backbone: ``backbone(samples) -> (features, positions)``, ``backbone[1]`` the positional
    encoding of a NestedTensor, ``num_channels`` and ``strides``.  A strided convolution and a tanh per level."""

    def __init__(self, channels, d):
        super().__init__(_Body(channels), _Position(d))
        self.num_channels = list(channels)
        self.strides = [4 * 2 ** i for i in range(len(channels))]

    def forward(self, samples):
        x, feats, pos = samples.tensors, [], []
        for conv in self[0].convs:
            x = torch.tanh(conv(x))
            mask = F.interpolate(samples.mask[None].float(), size=x.shape[-2:]).to(torch.bool)[0]
            feats.append(NestedTensor(x, mask))
            pos.append(self[1](feats[-1]).to(x.dtype))
        return feats, pos


def construct(model_cls, transformer_cls, case, cfg=CFG, **over):
    """The bare model of a case: the package's transformer, the stub backbone, the reference's arguments of build_dino."""
    tr = transformer_cls(d_model=cfg["d"], nhead=cfg["heads"], num_queries=cfg["queries"], num_encoder_layers=cfg["enc_layers"],
                         num_decoder_layers=cfg["dec_layers"], dim_feedforward=cfg["ffn"], dropout=0.0, activation="relu",
                         return_intermediate_dec=True, query_dim=4, modulate_hw_attn=True, deformable_encoder=True,
                         deformable_decoder=True, num_feature_levels=cfg["levels"], enc_n_points=cfg["points"],
                         dec_n_points=cfg["points"], learnable_tgt_init=True, two_stage_type="standard", decoder_sa_type="sa",
                         module_seq=["sa", "ca", "ffn"], embed_init_tgt=True)
    kw = dict(num_classes=cfg["K"], num_queries=cfg["queries"], aux_loss=True, iter_update=True, query_dim=4,
              num_feature_levels=cfg["levels"], nheads=cfg["heads"], two_stage_type="standard",
              two_stage_bbox_embed_share=CASES[case]["bbox_share"], two_stage_class_embed_share=True, decoder_sa_type="sa",
              dn_number=cfg["dn_number"], dn_box_noise_scale=0.4, dn_label_noise_ratio=0.0, dn_labelbook_size=cfg["K"])
    kw.update(over)
    return model_cls(StubBackbone(cfg["channels"], cfg["d"]), tr, **kw)


def build(model_cls, transformer_cls, case, cfg=CFG, **over):
    """The model under test (or the reference's), every parameter set from the case's seed by name — so nothing here depends on
    how a constructor consumes the RNG.  The GroupNorm scales are moved to around 1, the class heads widened."""
    model = construct(model_cls, transformer_cls, case, cfg, **over)
    set_parameters(model, _seed(case, cfg))
    with torch.no_grad():
        for proj in model.input_proj:
            proj[1].weight.add_(1.0)
        for head in {id(m): m for m in list(model.class_embed) + [model.transformer.enc_out_class_embed]}.values():
            head.weight.mul_(6.0)                                 # no selection or argmax within fp32 reach of a tie
    return model.train(CASES[case]["train"])


def images(case, cfg=CFG):
    rs = np.random.RandomState(_seed(case, cfg) + 1)
    N, (H, W) = cfg["N"], cfg["image"]
    img = rs.standard_normal((N, 3, H, W)).astype(np.float32)
    mask = np.zeros((N, H, W), dtype=bool)
    for n, (vh, vw) in enumerate(cfg["valid"]):
        mask[n, vh:, :] = True
        mask[n, :, vw:] = True
        img[n][:, mask[n]] = 0.0
    return img, mask


def targets(case, cfg=CFG, device="cpu", dtype=torch.float32):
    """The reference's target dict (per-frame label lists, keypoints [T_k, 42] in (0.05, 0.95)), None for the eval case."""
    if not CASES[case]["train"]:
        return None
    rs = np.random.RandomState(_seed(case, cfg) + 4)
    kps = [torch.from_numpy(rs.uniform(0.05, 0.95, (len(l), 42)).astype(np.float32)).to(device).to(dtype) for l in cfg["targets"]]
    return {"labels": [list(l) for l in cfg["targets"]], "keypoints": kps,
            "is_valid": torch.ones(len(cfg["targets"]), dtype=torch.int32)}


def flat_outputs(out):
    """[(name, tensor)] of every tensor of the output dict, in the dict's own order; dn_meta's denoising part included."""
    flat = []

    def walk(prefix, v):
        if torch.is_tensor(v):
            flat.append((prefix, v))
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(prefix + "." + k if prefix else k, x)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk("%s.%d" % (prefix, i), x)

    walk("", out)
    return flat


def key_order(out):
    """The dict's keys, nested ones too, in order (integers and None leaves included as names only)."""
    names = []

    def walk(prefix, v):
        names.append(prefix)
        if isinstance(v, dict):
            for k, x in v.items():
                walk(prefix + "." + k if prefix else k, x)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk("%s.%d" % (prefix, i), x)

    walk("", out)
    return names[1:]


def output_weight(case, j, shape):
    rs = np.random.RandomState(CASES[case]["seed"] * 10 + 2 + j)
    return rs.standard_normal(tuple(shape)).astype(np.float32)


def pgrad_index(case, k, numel):
    rs = np.random.RandomState(CASES[case]["seed"] * 100 + 3 + k)
    return rs.randint(0, numel, size=min(PGRAD_SAMPLES, numel)).astype(np.int64)


def prepare(case, device="cpu", dtype=torch.float32, cfg=CFG):
    img, mask = images(case, cfg)
    samples = NestedTensor(torch.from_numpy(img).to(device).to(dtype).requires_grad_(True), torch.from_numpy(mask).to(device))
    return dict(samples=samples, targets=targets(case, cfg, device, dtype), weights={}, device=device, dtype=dtype, case=case)


def step(model, prep, backward=True, **forward_kw):
    """One forward (+ backward of the seeded weighted sum over every output that carries a gradient) on prepared tensors:
    (the output dict, [(name, tensor)], the projected levels the transformer received)."""
    seen = []

    def keep(mod, args):
        seen.extend(args[0])
        for s in args[0]:
            if s.requires_grad:
                s.retain_grad()

    h = model.transformer.register_forward_pre_hook(keep)
    try:
        out = model(prep["samples"], prep["targets"], **forward_kw)
    finally:
        h.remove()
    flat = flat_outputs(out)
    if backward:
        loss = None
        for j, (name, o) in enumerate(flat):
            if not o.requires_grad:
                continue
            if name not in prep["weights"]:                      # made once per prepared step: a replayed step copies nothing
                prep["weights"][name] = torch.from_numpy(output_weight(prep["case"], j, o.shape)).to(prep["device"]).to(prep["dtype"])
            term = (o * prep["weights"][name]).sum()
            loss = term if loss is None else loss + term
        loss.backward()
    return out, flat, seen


def compare(model, case, z, device="cpu", cfg=CFG):
    """Run `model` on the case and compare with the fixture: [(what, error, bar)], errors relative to each tensor's max."""
    prep = prepare(case, device, cfg=cfg)
    out, flat, srcs = step(model, prep)
    report = []
    want = [str(k) for k in z[case + "/output_names"]]
    assert [k for k, _ in flat] == want, ([k for k, _ in flat], want)
    for j, (name, o) in enumerate(flat):
        report.append((name, _err(o.detach().cpu().numpy(), z["%s/out%d" % (case, j)]), ACT_BAR))
    report.append(("grad_image", _err(prep["samples"].tensors.grad.cpu().numpy(), z[case + "/grad_image"]), GRAD_BAR))
    for lvl, s in enumerate(srcs):
        report.append(("grad_src%d" % lvl, _err(s.grad.cpu().numpy(), z["%s/grad_src%d" % (case, lvl)]), GRAD_BAR))
    params = sorted(model.named_parameters(), key=lambda kv: kv[0])
    assert [k for k, _ in params] == [str(k) for k in z[case + "/param_names"]]
    for j, (k, p) in enumerate(params):
        ref_none = bool(z[case + "/pgrad_none"][j])
        if (p.grad is None) != ref_none:
            report.append(("pgrad None-ness " + k, float("inf"), GRAD_BAR))
            continue
        if ref_none:
            continue
        flat_g = p.grad.detach().flatten().double().cpu().numpy()
        idx = pgrad_index(case, j, flat_g.size)
        ref = z[case + "/pgrad_val"][j, :idx.size].astype(np.float64)
        total = float(z[case + "/pgrad_abssum"][j])
        report.append(("pgrad " + k, _err(flat_g[idx], ref, scale=total / flat_g.size), GRAD_BAR))
        report.append(("pgrad sum " + k, _err([flat_g.sum()], [float(z[case + "/pgrad_sum"][j])], scale=total), GRAD_BAR))
    return report
