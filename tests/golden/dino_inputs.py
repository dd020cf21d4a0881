"""Configuration, seeded parameters and inputs of the DINO decoder fixture (dino_decoder.npz), rebuilt wherever they are needed
instead of being stored: gen_dino_decoder.py (which ran the reference's TransformerDecoder on them) and tests/test_dino_decoder*.py
(which run the product on them) call the same functions.  Test infrastructure, no reference code."""
import numpy as np
import torch
from torch import nn

# N frames, L = 8 denoising rows (cdn_attention_mask(2, 2, 7)) + 7 matching queries, 2 levels whose padding makes every valid
# ratio differ from 1, K classes; two cases: 42-wide points (the live model) and 2-wide points (heads of the same width)
CFG = dict(N=2, d=256, heads=8, ffn=64, layers=2, shapes=[(6, 5), (3, 3)], valid=[[(5, 4), (2, 2)], [(4, 3), (2, 1)]],
           single_pad=2, dn_number=2, queries=7, K=14, points=4)
CASES = {"w42": dict(width=42, seed=4301), "w2": dict(width=2, seed=4302)}
CLS_SCALE = 6.0               # widens the class logits: no argmax within fp32 reach of a tie (MIN_MARGIN, checked by the generator)
MIN_MARGIN = 1e-3
PGRAD_SAMPLES = 64            # seeded elements kept of every parameter gradient
ACT_BAR, GRAD_BAR = 2e-4, 5e-4                # the bars of assembly_inputs.compare for module fixtures, relative to each tensor's max


def seq_len():
    return 2 * CFG["single_pad"] * CFG["dn_number"] + CFG["queries"]


class HeadMLP(nn.Module):
    """The model's 3-layer keypoint head: Linear -> ReLU -> Linear -> ReLU -> Linear (keys ``layers.{0,1,2}``)."""

    def __init__(self, d_in, d_hidden, d_out):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(d_in, d_hidden), nn.Linear(d_hidden, d_hidden), nn.Linear(d_hidden, d_out)])

    def forward(self, x):
        x = torch.relu(self.layers[0](x))
        x = torch.relu(self.layers[1](x))
        return self.layers[2](x)


def build(layer_cls, decoder_cls, case):
    """The decoder under test (or the reference's), its heads attached as dino.py attaches them, every parameter set from the
    case's seed by name — so nothing depends on how a constructor consumes the RNG."""
    c = CFG
    layer = layer_cls(d_model=c["d"], d_ffn=c["ffn"], dropout=0.0, activation="relu", n_levels=len(c["shapes"]), n_heads=c["heads"],
                      n_points=c["points"], decoder_sa_type="sa", module_seq=["sa", "ca", "ffn"])
    dec = decoder_cls(layer, c["layers"], nn.LayerNorm(c["d"]), return_intermediate=True, d_model=c["d"], query_dim=4,
                      num_feature_levels=len(c["shapes"]), deformable_decoder=True, rm_dec_query_scale=True)
    w = CASES[case]["width"]
    dec.class_embed = nn.ModuleList(nn.Linear(c["d"], c["K"]) for _ in range(c["layers"]))
    dec.key_embed = nn.ModuleList(HeadMLP(c["d"], c["d"], w) for _ in range(c["layers"]))
    dec.obj_key_embed = nn.ModuleList(HeadMLP(c["d"], c["d"], w) for _ in range(c["layers"]))
    set_parameters(dec, CASES[case]["seed"])
    return dec.eval()


def set_parameters(module, seed):
    """Every parameter from one seeded stream, in sorted name order: weights N(0, 1 / fan_in), LayerNorm scales 1 + 0.1 N,
    biases 0.1 N; the class weights widened by CLS_SCALE and the heads' last layers kept non-zero."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters(), key=lambda kv: kv[0]):
            r = torch.randn(p.shape, generator=g, dtype=torch.float32)
            if p.dim() >= 2:
                r = r / float(p.shape[-1]) ** 0.5
                if name.startswith("class_embed"):
                    r = r * CLS_SCALE
            elif "norm" in name and name.endswith("weight"):
                r = 1.0 + 0.1 * r
            else:
                r = 0.1 * r
            p.copy_(r)


def inputs(case):
    """tgt [L, N, d], memory / pos [S, N, d], refpoints_unsigmoid [L, N, width], the padding mask [N, S] and what goes with it."""
    c, w, seed = CFG, CASES[case]["width"], CASES[case]["seed"]
    rs = np.random.RandomState(seed + 1)
    L, N, d = seq_len(), c["N"], c["d"]
    S = sum(h * w_ for h, w_ in c["shapes"])
    masks = []
    for lvl, (H, W) in enumerate(c["shapes"]):
        m = np.ones((N, H, W), dtype=bool)
        for n in range(N):
            vh, vw = c["valid"][n][lvl]
            m[n, :vh, :vw] = False
        masks.append(m)
    return dict(tgt=rs.standard_normal((L, N, d)).astype(np.float32),
                memory=rs.standard_normal((S, N, d)).astype(np.float32),
                pos=rs.standard_normal((S, N, d)).astype(np.float32),
                refpoints=rs.standard_normal((L, N, w)).astype(np.float32),
                masks=masks,
                padding=np.concatenate([m.reshape(N, -1) for m in masks], 1),
                valid_ratios=np.stack([np.stack([(~m[:, 0, :]).sum(1) / m.shape[2], (~m[:, :, 0]).sum(1) / m.shape[1]], -1)
                                       for m in masks], 1).astype(np.float32),
                spatial_shapes=np.asarray(c["shapes"], dtype=np.int64),
                level_start_index=np.asarray([0] + list(np.cumsum([h * w_ for h, w_ in c["shapes"]])[:-1]), dtype=np.int64))


def output_weights(case, shapes):
    """The seeded weighting of every returned tensor (the loss is the sum of the weighted outputs)."""
    rs = np.random.RandomState(CASES[case]["seed"] + 2)
    return [rs.standard_normal(s).astype(np.float32) for s in shapes]


def pgrad_index(case, k, numel):
    rs = np.random.RandomState(CASES[case]["seed"] * 100 + 3 + k)
    return rs.randint(0, numel, size=min(PGRAD_SAMPLES, numel)).astype(np.int64)


def prepare(case, device="cpu", dtype=torch.float32, mask=True, ref_grad=True):
    """Everything one step reads, on `device`: the three leaves, the decoder's keyword arguments and the output weights.
    ref_grad=False: refpoints_unsigmoid arrives detached, as DINO's two-stage selection hands it over (with a gradient the
    first layer's points require grad, which selects the compositions there)."""
    from uvhand_amd.utils.denoising import cdn_attention_mask
    x = inputs(case)
    t = lambda a: torch.from_numpy(a).to(device)
    leaves = {k: t(x[k]).to(dtype).requires_grad_(True) for k in ("tgt", "memory", "refpoints")}
    leaves["refpoints"].requires_grad_(ref_grad)
    tgt_mask = cdn_attention_mask(CFG["single_pad"], CFG["dn_number"], CFG["queries"], device=device) if mask else None
    kwargs = dict(tgt_mask=tgt_mask, memory_key_padding_mask=t(x["padding"]), pos=t(x["pos"]).to(dtype),
                  level_start_index=t(x["level_start_index"]), spatial_shapes=t(x["spatial_shapes"]),
                  valid_ratios=t(x["valid_ratios"]).to(dtype))
    N, L, n = CFG["N"], seq_len(), CFG["layers"]
    shapes = [(N, L, CFG["d"])] * n + [(N, L, CASES[case]["width"])] * (n + 1)
    weights = [t(w_).to(dtype) for w_ in output_weights(case, shapes)]
    return dict(leaves=leaves, kwargs=kwargs, weights=weights)


def step(dec, prep):
    """One forward + backward on prepared tensors (no host <-> device traffic of its own): the outputs [hs..., refs...]."""
    lv = prep["leaves"]
    hs, refs = dec(lv["tgt"], lv["memory"], refpoints_unsigmoid=lv["refpoints"], **prep["kwargs"])
    outs = list(hs) + list(refs)
    loss = (outs[0] * prep["weights"][0]).sum()
    for o, w_ in zip(outs[1:], prep["weights"][1:]):
        loss = loss + (o * w_).sum()
    loss.backward()
    return outs


def run(dec, case, device="cpu", dtype=torch.float32, mask=True, ref_grad=True):
    """One forward + backward of `dec` on the case's inputs: (outputs [hs..., refs...], leaves {tgt, memory, refpoints})."""
    prep = prepare(case, device, dtype, mask, ref_grad)
    return step(dec, prep), prep["leaves"]


def ulp(x):
    import math
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 0.0


def hold(what, ours, t32, r64, ratios=None):
    """The project's accuracy rule: the largest error of `ours` against the fp64 evaluation is at most 4 times that of the torch
    fp32 composition, which counts as at least one fp32 ulp of the tensor's largest value.  Prints the figures, returns the ratio."""
    r64 = r64.double()
    e_ours = float((ours.double() - r64).abs().max()) if r64.numel() else 0.0
    e_torch = float((t32.double() - r64).abs().max()) if r64.numel() else 0.0
    top = float(r64.abs().max()) if r64.numel() else 0.0
    yard = max(e_torch, ulp(top))
    ratio = e_ours / yard if yard else (float("inf") if e_ours else 0.0)
    if ratios is not None:
        ratios[what] = max(ratios.get(what, 0.0), ratio)
    print("%-44s ours %.3e torch %.3e yardstick %.3e ratio %.2f" % (what, e_ours, e_torch, yard, ratio))
    assert e_ours <= 4.0 * yard, (what, e_ours, e_torch, yard)
    return ratio


def labels():
    n = CFG["layers"]
    return ["hs%d" % i for i in range(n)] + ["ref%d" % i for i in range(n + 1)]


def _err(got, ref, scale=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), scale or 0.0, 1e-30))


def compare(dec, case, z, device="cpu"):
    """Run `dec` on the case and compare with the fixture: [(what, error, bar)], errors relative to each tensor's max."""
    outs, leaves = run(dec, case, device)
    report = []
    for lab, o in zip(labels(), outs):
        report.append((lab, _err(o.detach().cpu().numpy(), z["%s/%s" % (case, lab)]), ACT_BAR))
    for k, leaf in leaves.items():
        report.append(("grad_" + k, _err(leaf.grad.cpu().numpy(), z["%s/grad_%s" % (case, k)]), GRAD_BAR))
    params = sorted(dec.named_parameters(), key=lambda kv: kv[0])
    assert [k for k, _ in params] == [str(k) for k in z[case + "/param_names"]]
    for j, (k, p) in enumerate(params):
        ref_none = bool(z[case + "/pgrad_none"][j])
        if (p.grad is None) != ref_none:
            report.append(("pgrad None-ness " + k, float("inf"), GRAD_BAR))
            continue
        if ref_none:
            continue
        flat = p.grad.detach().flatten().double().cpu().numpy()
        idx = pgrad_index(case, j, flat.size)
        ref = z[case + "/pgrad_val"][j, :idx.size].astype(np.float64)
        total = float(z[case + "/pgrad_abssum"][j])
        report.append(("pgrad " + k, _err(flat[idx], ref, scale=total / flat.size), GRAD_BAR))
        report.append(("pgrad sum " + k, _err([flat.sum()], [float(z[case + "/pgrad_sum"][j])], scale=total), GRAD_BAR))
    return report

