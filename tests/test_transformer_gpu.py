"""DeformableTransformer (uvhand_amd.modules) on the GPU against the reference's (tests/golden/transformer_*.npz, made by
gen_golden_r06.py), with the fused two-stage path on (the default).  Bars as in test_stack_gpu.py: activations within 2e-4
of each tensor's max, gradients within 5e-4; the selected refpoints (init_reference) exact or within 1e-5.  What the fixtures keep of each tensor
(rows, strided samples, fp64 row sums of every row) is set in tests/golden/two_stage_inputs.py.  inter_references is held to 1e-4: it
is the refinement sigmoid(logit(ref) + key_embed(hs)) of every decoder layer, so it carries the hidden state's fp32 reordering
error through the keypoint MLP (measured 1.6e-5 of max on the MI355X), not just a selection.

Gradients: 5e-4 everywhere in the one-stage fixture and on the decoder side of the two-stage one (decoder layers, pos_trans
and its norm, the per-layer heads: measured <= 2.6e-4).  On the encoder side of the two-stage fixture (6 encoder layers at
d_model 256: encoder parameters, level_embed, the input gradients, enc_output and the heads on the encoder output,
``*_embed.6``) the bar is 3e-2, measured on the MI355X: 1.9e-2 of max on key_embed[6].layers.0.weight and 1.1e-2 on the
finest level's pos gradient, 4e-3 on encoder parameters.  Both come from discrete flips that fp32 reordering decides, not from
the two-stage code (whose gradients test_two_stage_gpu.py checks against fp64 at 5e-6): ReLU flips in the 4180-row
encoder-output heads (one flipped row moves a weight gradient by ~1/sqrt(rows) of its scale) and sampling points within
rounding of a bilinear kink, whose location gradient jumps, through six encoder layers.  The queries are matched to the fixture's by
their refpoints first: the selection's order inside the top 300 follows logit gaps far below fp32 reach (the generator keeps
every discrete decision — the top-300 boundary, the class argmaxes — >= 1e-3 away, not the order among the selected), and
the decoder is equivariant under a permutation of the queries, so the outputs and the output gradients are permuted to the
fixture's order."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import two_stage_inputs as TI  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ACT, GRAD, ENC_GRAD, REFP, INTER = 2e-4, 5e-4, 3e-2, 1e-5, 1e-4
ENC_SIDE = re.compile(r"^(encoder\.|level_embed|enc_output|decoder\.(cls_embed|key_embed|obj_key_embed)\.6\.)")
LABELS = ["hs", "init_reference", "inter_references", "enc_class", "enc_hand", "enc_obj"]


def _build(name):
    from uvhand_amd.modules import DeformableTransformer
    cfg = TI.CONFIGS[name]
    torch.manual_seed(cfg["wseed"])
    tr = DeformableTransformer(d_model=cfg["d"], nhead=cfg["heads"], num_encoder_layers=cfg["enc"], num_decoder_layers=cfg["dec"],
                               dim_feedforward=cfg["ffn"], dropout=0.0, return_intermediate_dec=True,
                               num_feature_levels=len(cfg["shapes"]), two_stage=cfg["two_stage"], two_stage_num_proposals=cfg["Q"],
                               two_stage_learn_xy=True)
    TI.attach_heads(tr, cfg, 42 if cfg["two_stage"] else 2)
    return tr.to(DEV), cfg


def _inputs(cfg, z):
    seed = int(z["seed"])
    x = TI.inputs(cfg, seed)
    assert np.array_equal(TI.checksums(x), z["input_checksums"])
    srcs = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in x["srcs"]]
    poss = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in x["poss"]]
    masks = [torch.from_numpy(m).to(DEV) for m in x["masks"]]
    query = None if cfg["two_stage"] else torch.from_numpy(x["query"]).to(DEV).requires_grad_(True)
    return seed, srcs, poss, masks, query


_REPORT = []


def _close(got, ref, bar, what, scale=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf), what + ": +inf placement"
    if (~inf).any():
        scale = max(np.abs(ref[~inf]).max(), scale or 0.0, 1e-30)
        err = np.abs(got[~inf] - ref[~inf]).max() / scale
        _REPORT.append((what, err, bar))                       # every comparison is reported, then asserted together
        print("%-40s %.3e (bar %.0e)" % (what, err, bar))


def _perm(init_ref, fixture_ref):
    """perm[n, q] = the fixture's query matching the product's query q of frame n (nearest refpoint row, within 1e-5)."""
    N, Q, _ = init_ref.shape
    perm = torch.empty(N, Q, dtype=torch.long)
    for n in range(N):
        d = torch.cdist(init_ref[n].double(), fixture_ref[n].double(), p=float("inf"))
        dist, idx = d.min(1)
        assert dist.max() <= REFP, "selected refpoints differ from the reference's: %.3e" % dist.max()
        assert torch.unique(idx).numel() == Q
        perm[n] = idx
    return perm


def _reorder(t, index, qdim):
    """out[..., n, j, ...] = t[..., n, index[n, j], ...] for the frame / query dimensions (qdim - 1, qdim)."""
    tt = t.movedim((qdim - 1, qdim), (0, 1))
    out = tt[torch.arange(index.shape[0], device=index.device)[:, None], index]
    return out.movedim((0, 1), (qdim - 1, qdim))


@pytest.mark.parametrize("name", ["two_stage", "one_stage"])
def test_fixture_through_product(name):
    z = np.load(os.path.join(HERE, "golden", "transformer_%s.npz" % name))
    tr, cfg = _build(name)
    names, sums = TI.state_checksums(tr)
    assert np.array_equal(sums, z["state_checksums"])
    TI.perturb(tr, cfg)
    seed, srcs, poss, masks, query = _inputs(cfg, z)
    outs = [o for o in tr(srcs, masks, poss, query) if o is not None]
    grads = [torch.from_numpy(g).to(DEV) for g in TI.output_grads(cfg, seed, [tuple(o.shape) for o in outs])]
    if cfg["two_stage"]:
        match = torch.from_numpy(z["init_reference_match"])                # the leading columns of every selected refpoint
        perm = _perm(outs[1].detach().cpu()[..., :match.shape[-1]], match).to(DEV)
        inv = torch.argsort(perm, dim=1)                       # product query of each fixture query
        to_fixture = lambda t, qdim: _reorder(t, inv, qdim)    # noqa: E731
        from_fixture = lambda t, qdim: _reorder(t, perm, qdim)  # noqa: E731

        cmp_outs = [to_fixture(outs[0].detach(), 2), to_fixture(outs[1].detach(), 1), to_fixture(outs[2].detach(), 2)] + \
            [o.detach() for o in outs[3:]]
        grads = [from_fixture(grads[0], 2), grads[1], grads[2]] + grads[3:]
        _close(cmp_outs[1].cpu()[..., :match.shape[-1]], match, REFP, "init_reference matched columns")
    else:
        cmp_outs = [o.detach() for o in outs]
    for lab, o in zip(LABELS, cmp_outs):
        rows = o.reshape(-1, o.shape[-1]).cpu()
        bar = {"init_reference": REFP, "inter_references": INTER}.get(lab, ACT)
        _close(rows[::TI.row_step(lab, cfg)].numpy(), z[lab + "_rows"], bar, lab)
        # a LayerNorm output's row sums cancel to ~0: their scale is the elements' times sqrt(width), not their own maximum
        fin = np.isfinite(z[lab + "_rows"])
        elem = np.abs(z[lab + "_rows"][fin]).max() if fin.any() else 0.0
        _close(rows.double().sum(-1).numpy(), z[lab + "_rowsum"], bar, lab + " row sums", scale=elem * o.shape[-1] ** 0.5)
    pairs = [(o, g) for o, g in zip(outs, grads) if o.requires_grad]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    in_bar = ENC_GRAD if cfg["two_stage"] else GRAD
    for i, (s, p) in enumerate(zip(srcs, poss)):
        _close(s.grad.double().sum(1).cpu(), z["grad_src%d_rowsum" % i], in_bar, "grad_src%d" % i)
        _close(p.grad.double().sum(1).cpu(), z["grad_pos%d_rowsum" % i], in_bar, "grad_pos%d" % i)
        _close(s.grad.flatten()[::TI.GRAD_STRIDE].cpu(), z["grad_src%d_sample" % i], in_bar, "grad_src%d sample" % i)
        _close(p.grad.flatten()[::TI.GRAD_STRIDE].cpu(), z["grad_pos%d_sample" % i], in_bar, "grad_pos%d sample" % i)
    if query is not None:
        _close(query.grad.cpu(), z["grad_query"], GRAD, "grad_query")
    params = list(tr.named_parameters())
    assert [k for k, _ in params] == [str(k) for k in z["param_names"]]
    for j, (k, p) in enumerate(params):
        ref_none = bool(z["pgrad_none"][j])
        assert (p.grad is None) == ref_none, k
        if ref_none:
            continue
        flat = p.grad.flatten()
        idx = TI.pgrad_index(seed, j, flat.numel())
        vals = flat[torch.from_numpy(idx).to(DEV)].double().cpu().numpy()
        ref = z["pgrad_val"][j, :idx.size].astype(np.float64)
        total = float(z["pgrad_abssum"][j])
        scale = max(np.abs(ref).max(), total / flat.numel(), 1e-30)
        bar = ENC_GRAD if (cfg["two_stage"] and ENC_SIDE.match(k)) else GRAD
        _close(vals, ref, bar, "pgrad " + k, scale=scale)
        _close([float(flat.double().sum())], [float(z["pgrad_sum"][j])], bar, "pgrad sum " + k, scale=total)
    bad = [r for r in _REPORT if not r[1] <= r[2]]
    _REPORT.clear()
    assert not bad, "beyond the bars: " + "; ".join("%s %.3e > %.0e" % r for r in bad[:12])
    if cfg["two_stage"]:
        g = tr.two_stage_learn_xy.weight.grad
        assert g is not None and torch.count_nonzero(g) == 0


def test_two_stage_bf16_autocast_runs_finite():
    tr, cfg = _build("two_stage")
    z = np.load(os.path.join(HERE, "golden", "transformer_two_stage.npz"))
    TI.perturb(tr, cfg)
    seed, srcs, poss, masks, _ = _inputs(cfg, z)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        hs, init_ref, inter, cls, hand, obj = tr(srcs, masks, poss)
    assert torch.isfinite(hs).all() and torch.isfinite(init_ref).all()
    loss = hs.float().sum() + cls.float().sum()
    loss.backward()
    for s in srcs:
        assert torch.isfinite(s.grad).all()
