"""Configurations and per-layer heads of the AssemblyHands transformer fixtures (assembly_one_stage.npz /
assembly_two_stage.npz), rebuilt wherever they are needed instead of being stored: gen_golden_r07.py (which ran the
reference on them) and tests/test_assembly*.py (which run the product on them) call the same functions.  Inputs, the
seeded parameter perturbation, output gradients and checksums are two_stage_inputs.py's.  Test infrastructure, no
reference code."""
import copy
import math

import numpy as np
import torch
from torch import nn

import two_stage_inputs as TI

# one_stage: the path AssemblyHands training runs (one-stage, with_box_refine, 3 classes, 300 queries, 2-d initial refpoints);
# two_stage: the H2O label layout the file's two-stage selection indexes (11 classes, the 3 queries the selection implies)
CONFIGS = {
    "one_stage": dict(d=256, heads=8, ffn=1024, enc=6, dec=6, shapes=[(28, 28), (14, 14), (7, 7), (4, 4)], N=4, Q=300,
                      two_stage=False, classes=3, wseed=707, subsample=True),
    "two_stage": dict(d=64, heads=2, ffn=128, enc=2, dec=2, shapes=[(28, 28), (14, 14), (7, 7), (4, 4)], N=4, Q=3,
                      two_stage=True, classes=11, wseed=708, subsample=False),
}
KP_WIDTH = 63                 # 21 (x, y, z) keypoints per head output (models/assembly_detr.py:101-102)
ROW_STEP = {"hs": 193}        # as two_stage_inputs.ROW_STEP, for the subsampled (large) fixture
ROW_STEP_DEFAULT = 61


def attach_heads(transformer, cfg):
    """cls_embed Linear(d, classes) and the 3-layer 63-output keypoint_embed / obj_keypoint_embed MLPs, cloned per prediction
    (decoder layers + 1 when two-stage) and attached as with_box_refine attaches them (models/assembly_detr.py:100-118):
    the class bias at the 0.01 prior, the MLPs' last layers zeroed; drawn from torch.manual_seed(wseed + 1).  The class
    weights are widened by two_stage_inputs.CLS_SCALE so that no decision sits within fp32 reach of a tie."""
    torch.manual_seed(cfg["wseed"] + 1)
    d = cfg["d"]
    n_pred = cfg["dec"] + (1 if cfg["two_stage"] else 0)
    cls = nn.Linear(d, cfg["classes"])
    with torch.no_grad():
        cls.bias.fill_(-math.log((1 - 0.01) / 0.01))
        cls.weight.mul_(TI.CLS_SCALE)
    key, obj = TI.HeadMLP(d, d, KP_WIDTH, 3), TI.HeadMLP(d, d, KP_WIDTH, 3)
    for h in (key, obj):
        nn.init.constant_(h.layers[-1].weight.data, 0)
        nn.init.constant_(h.layers[-1].bias.data, 0)
    dec = transformer.decoder
    dec.cls_embed = nn.ModuleList(copy.deepcopy(cls) for _ in range(n_pred))
    dec.keypoint_embed = nn.ModuleList(copy.deepcopy(key) for _ in range(n_pred))
    dec.obj_keypoint_embed = nn.ModuleList(copy.deepcopy(obj) for _ in range(n_pred))
    return dec.cls_embed, dec.keypoint_embed, dec.obj_keypoint_embed


def build_kwargs(cfg):
    return dict(d_model=cfg["d"], nhead=cfg["heads"], num_encoder_layers=cfg["enc"], num_decoder_layers=cfg["dec"],
                dim_feedforward=cfg["ffn"], dropout=0.0, return_intermediate_dec=True, num_feature_levels=len(cfg["shapes"]),
                two_stage=cfg["two_stage"], two_stage_num_proposals=cfg["Q"], cfg=None)


def row_step(label, cfg):
    return ROW_STEP.get(label, ROW_STEP_DEFAULT) if cfg["subsample"] else 1


def selection_margins(cls):
    """The discrete decisions of the two-stage selection (models/assembly_transformer.py:202-210) per frame: the gap between
    each class column's maximum and its next distinct value (rows zeroed by the proposals give bitwise-equal logits, whose
    ties the first-index rule settles exactly), and |score - best| of every comparison of the object loop."""
    cls = cls.detach().double()
    gaps = []
    for n in range(cls.shape[0]):
        best = 0.0
        for k in range(1, 11):
            col = torch.unique(cls[n, :, k])
            if col.numel() > 1:
                top = torch.topk(col, 2)[0]
                gaps.append(float(top[0] - top[1]))
            if k <= 8:
                score = float(cls[n, :, k].max())
                gaps.append(abs(score - best))
                if best < score:
                    best = score
    return np.asarray(gaps, dtype=np.float64)


LABELS = ["hs", "init_reference", "inter_references", "enc_class", "enc_hand", "enc_obj"]


def _close(report, got, ref, bar, what, scale=None):
    """Append (what, max error / scale, bar); +inf must sit where the fixture has it."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    inf = np.isinf(ref)
    if not np.array_equal(np.isinf(got), inf):
        report.append((what + " (+inf placement)", float("inf"), bar))
        return
    if (~inf).any():
        scale = max(np.abs(ref[~inf]).max(), scale or 0.0, 1e-30)
        report.append((what, float(np.abs(got[~inf] - ref[~inf]).max() / scale), bar))


def compare(tr, cfg, z, device, act=2e-4, grad=5e-4, backward=True):
    """Run the (constructed, not yet perturbed) product transformer on the fixture's inputs on `device` and compare with the
    fixture: every output's kept rows and fp64 row sums (bar `act`, relative to each tensor's max), then — with backward —
    the input and parameter gradients (bar `grad`).  Returns [(what, error, bar)]."""
    report = []
    names, sums = TI.state_checksums(tr)
    assert np.array_equal(sums, z["state_checksums"]), "seeded construction differs from the reference's"
    TI.perturb(tr, cfg)
    seed = int(z["seed"])
    x = TI.inputs(cfg, seed)
    assert np.array_equal(TI.checksums(x), z["input_checksums"])
    srcs = [torch.from_numpy(a).to(device).requires_grad_(backward) for a in x["srcs"]]
    poss = [torch.from_numpy(a).to(device).requires_grad_(backward) for a in x["poss"]]
    masks = [torch.from_numpy(m).to(device) for m in x["masks"]]
    query = torch.from_numpy(x["query"]).to(device).requires_grad_(backward)
    with torch.set_grad_enabled(backward):
        outs = [o for o in tr(srcs, masks, poss, query) if o is not None]
    for lab, o in zip(LABELS, outs):
        rows = o.detach().reshape(-1, o.shape[-1]).cpu()
        _close(report, rows[::row_step(lab, cfg)].numpy(), z[lab + "_rows"], act, lab)
        fin = np.isfinite(z[lab + "_rows"])
        elem = np.abs(z[lab + "_rows"][fin]).max() if fin.any() else 0.0
        _close(report, rows.double().sum(-1).numpy(), z[lab + "_rowsum"], act, lab + " row sums", scale=elem * o.shape[-1] ** 0.5)
    if not backward:
        return report
    grads = [torch.from_numpy(g).to(device) for g in TI.output_grads(cfg, seed, [tuple(o.shape) for o in outs])]
    pairs = [(o, g) for o, g in zip(outs, grads) if o.requires_grad]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    for i, (s, p) in enumerate(zip(srcs, poss)):
        _close(report, s.grad.double().sum(1).cpu(), z["grad_src%d_rowsum" % i], grad, "grad_src%d" % i)
        _close(report, p.grad.double().sum(1).cpu(), z["grad_pos%d_rowsum" % i], grad, "grad_pos%d" % i)
        _close(report, s.grad.flatten()[::TI.GRAD_STRIDE].cpu(), z["grad_src%d_sample" % i], grad, "grad_src%d sample" % i)
        _close(report, p.grad.flatten()[::TI.GRAD_STRIDE].cpu(), z["grad_pos%d_sample" % i], grad, "grad_pos%d sample" % i)
    _close(report, query.grad.double().sum(1).cpu(), z["grad_query_rowsum"], grad, "grad_query")
    _close(report, query.grad.flatten()[::TI.GRAD_STRIDE].cpu(), z["grad_query_sample"], grad, "grad_query sample")
    params = list(tr.named_parameters())
    assert [k for k, _ in params] == [str(k) for k in z["param_names"]]
    for j, (k, p) in enumerate(params):
        ref_none = bool(z["pgrad_none"][j])
        if (p.grad is None) != ref_none:
            report.append(("pgrad None-ness " + k, float("inf"), grad))
            continue
        if ref_none:
            continue
        flat = p.grad.flatten()
        idx = TI.pgrad_index(seed, j, flat.numel())
        vals = flat[torch.from_numpy(idx).to(flat.device)].double().cpu().numpy()
        ref = z["pgrad_val"][j, :idx.size].astype(np.float64)
        total = float(z["pgrad_abssum"][j])
        scale = max(np.abs(ref).max(), total / flat.numel(), 1e-30)
        _close(report, vals, ref, grad, "pgrad " + k, scale=scale)
        _close(report, [float(flat.double().sum())], [float(z["pgrad_sum"][j])], grad, "pgrad sum " + k, scale=total)
    return report
