"""Configuration, seeded parameters and inputs of the DINO DeformableTransformer fixture (dino_transformer.npz), rebuilt wherever
they are needed instead of being stored: gen_dino_transformer.py (which ran the reference's DeformableTransformer on them) and
tests/test_dino_transformer*.py (which run the product on them) call the same functions.  Test infrastructure, no reference code."""
import numpy as np
import torch
from torch import nn

from dino_inputs import ACT_BAR, GRAD_BAR, MIN_MARGIN, PGRAD_SAMPLES, _err, hold, set_parameters, ulp  # noqa: F401

# N frames over a three-level pyramid (S = 43); frame 1 has a padded right / bottom border; Q queries out of K classes
CFG = dict(N=2, d=256, heads=8, ffn=64, enc_layers=2, dec_layers=2, shapes=[(6, 5), (3, 3), (2, 2)],
           valid=[[(6, 5), (3, 3), (2, 2)], [(5, 4), (3, 2), (2, 1)]], queries=7, K=14, points=4,
           dn_single_pad=1, dn_number=3)
# (i) the learned tgt, no denoising inputs; (ii) the selected rows as tgt and the learned proposal offsets; (iii) = (i) with
# six denoising rows under cdn_attention_mask(1, 3, 7)
CASES = {"embed": dict(seed=5104, embed_init_tgt=True, learn_wh=False, dn=False),
         "rows_wh": dict(seed=5108, embed_init_tgt=False, learn_wh=True, dn=False),
         "embed_dn": dict(seed=5104, embed_init_tgt=True, learn_wh=False, dn=True)}
INIT_SEED = 77                # torch.manual_seed before a bare construction (the seeded-initialisation sums)
# a second pyramid beyond the 8192 rows the older selection kernel sorts: S = 8193 + 64, N = 1, Q = 900, 1 + 1 layers
BIG = dict(N=1, d=256, heads=8, ffn=64, enc_layers=1, dec_layers=1, shapes=[(99, 83), (8, 5)], queries=900, K=14, points=4,
           seed=5201)
assert sum(h * w for h, w in BIG["shapes"]) == 8193 + 64


def n_rows(cfg=CFG):
    return sum(h * w for h, w in cfg["shapes"])


def dn_rows():
    return 2 * CFG["dn_single_pad"] * CFG["dn_number"]


def construct(transformer_cls, case, cfg=CFG, **over):
    """The bare transformer of a case, as ``build_deformable_transformer`` would make it at this size."""
    c = CASES[case] if case is not None else dict(embed_init_tgt=True, learn_wh=False)
    kw = dict(d_model=cfg["d"], nhead=cfg["heads"], num_queries=cfg["queries"], num_encoder_layers=cfg["enc_layers"],
              num_decoder_layers=cfg["dec_layers"], dim_feedforward=cfg["ffn"], dropout=0.0, activation="relu",
              return_intermediate_dec=True, query_dim=4, modulate_hw_attn=True, deformable_encoder=True, deformable_decoder=True,
              num_feature_levels=len(cfg["shapes"]), enc_n_points=cfg["points"], dec_n_points=cfg["points"],
              learnable_tgt_init=True, two_stage_type="standard", two_stage_learn_wh=c["learn_wh"], decoder_sa_type="sa",
              module_seq=["sa", "ca", "ffn"], embed_init_tgt=c["embed_init_tgt"])
    kw.update(over)
    return transformer_cls(**kw)


def build(transformer_cls, mlp_cls, case, cfg=CFG, seed=None):
    """The transformer under test (or the reference's) with its heads attached as dino.py:200-220 attaches them, every
    parameter set from the case's seed by name — so nothing here depends on how a constructor consumes the RNG."""
    tr = construct(transformer_cls, case, cfg)
    d, K, n = cfg["d"], cfg["K"], cfg["dec_layers"]
    tr.decoder.class_embed = nn.ModuleList(nn.Linear(d, K) for _ in range(n))
    tr.decoder.key_embed = nn.ModuleList(mlp_cls(d, d, 42, 3) for _ in range(n))
    tr.decoder.obj_key_embed = nn.ModuleList(mlp_cls(d, d, 42, 3) for _ in range(n))
    tr.enc_out_class_embed = nn.Linear(d, K)
    tr.enc_out_key_embed = mlp_cls(d, d, 42, 3)
    tr.enc_out_obj_key_embed = mlp_cls(d, d, 42, 3)
    seed = CASES[case]["seed"] if seed is None else seed
    set_parameters(tr, seed)
    with torch.no_grad():
        # the encoder's class head decides the selection: widened like the decoder's, so that no order or argmax sits within
        # fp32 reach of a tie (checked by the generator); the learned offsets start where _reset_parameters puts them
        tr.enc_out_class_embed.weight.mul_(6.0)
        for head in tr.decoder.class_embed:
            head.weight.mul_(6.0)
        if getattr(tr, "two_stage_wh_embedding", None) is not None:
            tr.two_stage_wh_embedding.weight.mul_(0.3).add_(-2.9444)
    return tr.eval()


def inputs(case, cfg=CFG):
    seed = (CASES[case]["seed"] if case is not None else cfg["seed"]) + 1
    rs = np.random.RandomState(seed)
    N, d = cfg["N"], cfg["d"]
    srcs, poss, masks = [], [], []
    for lvl, (H, W) in enumerate(cfg["shapes"]):
        srcs.append(rs.standard_normal((N, d, H, W)).astype(np.float32))
        poss.append(rs.standard_normal((N, d, H, W)).astype(np.float32))
        m = np.zeros((N, H, W), dtype=bool)
        if "valid" in cfg:
            for n in range(N):
                vh, vw = cfg["valid"][n][lvl]
                m[n, vh:, :] = True
                m[n, :, vw:] = True
        masks.append(m)
    out = dict(srcs=srcs, poss=poss, masks=masks)
    if case is not None and CASES[case]["dn"]:
        out["dn_ref"] = rs.standard_normal((N, dn_rows(), 42)).astype(np.float32)
        out["dn_tgt"] = rs.standard_normal((N, dn_rows(), d)).astype(np.float32)
    return out


def output_shapes(case, cfg=CFG):
    N, d, Q = cfg["N"], cfg["d"], cfg["queries"]
    L = Q + (dn_rows() if case is not None and CASES[case]["dn"] else 0)
    n = cfg["dec_layers"]
    return [(N, L, d)] * n + [(N, L, 42)] * (n + 1) + [(1, N, Q, d), (1, N, Q, 42), (1, N, Q, 42), (N, Q, 42)]


def labels(cfg=CFG):
    n = cfg["dec_layers"]
    return (["hs%d" % i for i in range(n)] + ["ref%d" % i for i in range(n + 1)]
            + ["hs_enc", "ref_enc_obj", "ref_enc_hand", "init_box_proposal_unsig"])


def output_weights(case, cfg=CFG):
    seed = (CASES[case]["seed"] if case is not None else cfg["seed"]) + 2
    rs = np.random.RandomState(seed)
    return [rs.standard_normal(s).astype(np.float32) for s in output_shapes(case, cfg)]


def pgrad_index(case, k, numel):
    rs = np.random.RandomState(CASES[case]["seed"] * 100 + 3 + k)
    return rs.randint(0, numel, size=min(PGRAD_SAMPLES, numel)).astype(np.int64)


def prepare(case, device="cpu", dtype=torch.float32, cfg=CFG):
    """Everything one step reads, on `device`: the leaves (srcs), the forward's arguments and the output weights."""
    from uvhand_amd.utils.denoising import cdn_attention_mask
    x = inputs(case, cfg)
    t = lambda a: torch.from_numpy(a).to(device)
    srcs = [t(a).to(dtype).requires_grad_(True) for a in x["srcs"]]
    poss = [t(a).to(dtype) for a in x["poss"]]
    masks = [t(a) for a in x["masks"]]
    dn_ref = dn_tgt = attn_mask = None
    if "dn_ref" in x:
        dn_ref, dn_tgt = t(x["dn_ref"]).to(dtype), t(x["dn_tgt"]).to(dtype)
        attn_mask = cdn_attention_mask(CFG["dn_single_pad"], CFG["dn_number"], CFG["queries"], device=device)
    weights = [t(w).to(dtype) for w in output_weights(case, cfg)]
    return dict(srcs=srcs, poss=poss, masks=masks, dn_ref=dn_ref, dn_tgt=dn_tgt, attn_mask=attn_mask, weights=weights)


def flat_outputs(ret):
    hs, references, hs_enc, ref_enc, init_box = ret
    return list(hs) + list(references) + [hs_enc, ref_enc[0], ref_enc[1], init_box]


def step(tr, prep, backward=True):
    """One forward (+ backward of the seeded weighted sum) on prepared tensors, without host <-> device traffic of its own:
    the nine flat outputs.  The sum runs over the outputs that carry gradient."""
    ret = tr(prep["srcs"], prep["masks"], prep["dn_ref"], prep["poss"], prep["dn_tgt"], prep["attn_mask"])
    outs = flat_outputs(ret)
    if backward:
        loss = None
        for o, w in zip(outs, prep["weights"]):
            if o.requires_grad:
                term = (o * w).sum()
                loss = term if loss is None else loss + term
        loss.backward()
    return outs


def compare(tr, case, z, device="cpu"):
    """Run `tr` on the case and compare with the fixture: [(what, error, bar)], errors relative to each tensor's max; the
    selected rows must be the fixture's exactly."""
    prep = prepare(case, device)
    outs = step(tr, prep)
    report = [("topk", 0.0 if np.array_equal(tr.last_topk_proposals.cpu().numpy(), z[case + "/topk"]) else float("inf"), 0.0)]
    for lab, o in zip(labels(), outs):
        report.append((lab, _err(o.detach().cpu().numpy(), z["%s/%s" % (case, lab)]), ACT_BAR))
    for lvl, s in enumerate(prep["srcs"]):
        report.append(("grad_src%d" % lvl, _err(s.grad.cpu().numpy(), z["%s/grad_src%d" % (case, lvl)]), GRAD_BAR))
    params = sorted(tr.named_parameters(), key=lambda kv: kv[0])
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


def numpy_select_rule(cls, Q, hand=(12, 13)):
    """The selection rule restated in numpy: per row the first maximum, NaN winning (the first NaN's class is the argmax); per
    frame a stable sort of the rows by descending maximum, NaN above every number, so ties keep the lower row first and -0
    equals +0 (the comparison is numeric).  Returns (topk [N, Q] int64, code [N, Q] uint8)."""
    cls = np.asarray(cls, dtype=np.float32)
    N, S, K = cls.shape
    topk = np.zeros((N, Q), dtype=np.int64)
    code = np.zeros((N, Q), dtype=np.uint8)
    for n in range(N):
        isnan = np.isnan(cls[n])
        nan_row = isnan.any(1)
        safe = np.where(isnan, -np.inf, cls[n])
        arg = np.where(nan_row, isnan.argmax(1), safe.argmax(1))
        val = np.where(nan_row, np.inf, safe.max(1)).astype(np.float64)
        order = np.lexsort((np.arange(S), -val, ~nan_row))          # the last key is the first criterion; lexsort is stable
        topk[n] = order[:Q]
        a = arg[topk[n]]
        is_hand = (a == hand[0]) | (a == hand[1])
        code[n] = np.where(is_hand, 2, np.where(a != 0, 1, 0))
    return topk, code
