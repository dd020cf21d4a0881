"""The DINO model class (uvhand_amd.modules.DINO) on the GPU, at the smallest size the HIP routes take
(tests/golden/dino_model_inputs.GPU_CFG: hidden 256, 8 heads, 2 levels, 20 queries, 2 frames, 5 targets): every output and
gradient of a training step held to the project's accuracy rule against the same model with MSDA_HEADS_FUSED=0, with an fp64
copy as the yardstick; the step under torch.cuda.set_sync_debug_mode("error") with the targets given as PackedTargets; the
output dict through SetDinoCriterion and the package's AdamW."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_model_inputs as MI  # noqa: E402

pytestmark = pytest.mark.gpu

CASE, CFG = "train", MI.GPU_CFG
RATIOS = {}


def _dev():
    return torch.device("cuda:0")


def _build():
    from uvhand_amd.modules import DINO, DinoDeformableTransformer
    return MI.build(DINO, DinoDeformableTransformer, CASE, CFG).to(_dev())


def _results(model, prep, flat, srcs):
    params = sorted(model.named_parameters())
    names = ([k for k, _ in flat] + ["grad_image"] + ["grad_src%d" % i for i in range(len(srcs))] + ["pgrad " + k for k, _ in params])
    return names, [o.detach() for _, o in flat] + [prep["samples"].tensors.grad] + [s.grad for s in srcs] + [p.grad for _, p in params]


def _heads_launches(monkeypatch):
    from uvhand_amd import _native as MSDA
    calls = []
    real_f, real_r = MSDA.heads_forward, MSDA.heads_ref_backward
    monkeypatch.setattr(MSDA, "heads_forward", lambda *a, **k: (calls.append("forward"), real_f(*a, **k))[1])
    monkeypatch.setattr(MSDA, "heads_ref_backward", lambda *a, **k: (calls.append("ref_backward"), real_r(*a, **k))[1])
    return calls


def test_training_step_holds_the_ratio_rule(monkeypatch):
    """ours: the model as shipped (the heads node with its reference gradient).  The yardstick: the same model with
    MSDA_HEADS_FUSED=0 (the reference's per-layer composition after the transformer) in fp32 on the GPU.  Both against that
    composition on an fp64 copy."""
    calls = _heads_launches(monkeypatch)
    model = _build()
    prep = MI.prepare(CASE, _dev(), cfg=CFG)
    out, flat, srcs = MI.step(model, prep)
    names, ours = _results(model, prep, flat, srcs)
    assert calls == ["forward", "ref_backward"], "the heads node did not serve the step: %s" % calls
    assert out["dn_meta"]["pad_size"] == 2 * 3 * 2 * CFG["dn_number"] and "output_known_lbs_bboxes" in out["dn_meta"]
    topk = model.transformer.last_topk_proposals.clone()
    monkeypatch.setenv("MSDA_HEADS_FUSED", "0")
    got = []
    for dt in (torch.float32, torch.float64):
        m2 = copy.deepcopy(model).to(dt)
        m2.zero_grad(set_to_none=True)
        p2 = MI.prepare(CASE, _dev(), dt, cfg=CFG)
        _, f2, s2 = MI.step(m2, p2)
        n2, r2 = _results(m2, p2, f2, s2)
        assert n2 == names and torch.equal(m2.transformer.last_topk_proposals, topk), dt
        got.append(r2)
    assert len(calls) == 2, "the yardstick ran on the heads node"
    for name, a, b, c in zip(names, ours, got[0], got[1]):
        assert (a is None) == (b is None) == (c is None), name
        if a is not None:
            MI.hold(name, a, b, c, RATIOS)


def test_training_step_with_packed_targets_makes_no_host_sync():
    from uvhand_amd.matcher import pack_targets
    model = _build()
    prep = MI.prepare(CASE, _dev(), cfg=CFG)
    packed = pack_targets(prep["targets"], _dev())
    MI.step(model, prep, packed=packed)                 # the first call: level tensors, output weights, allocations
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, flat, _ = MI.step(model, prep, packed=packed)      # forward + backward: nothing may synchronise
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(o).all()) for _, o in flat)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in model.named_parameters())


def test_output_feeds_the_dino_criterion():
    from types import SimpleNamespace
    from uvhand_amd import criterion as C
    from uvhand_amd import matcher as M
    from uvhand_amd.optim import AdamW
    model = _build()
    opt = AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    before = model.key_embed[0].layers[0].weight.detach().clone()
    prep = MI.prepare(CASE, _dev(), cfg=CFG)
    out, _, _ = MI.step(model, prep, backward=False)
    n_aux = CFG["dec_layers"] - 1
    terms = ("loss_ce", "loss_hand_keypoint", "loss_obj_keypoint")
    weight = {k + s: 1.0 for k in terms for s in [""] + ["_%d" % i for i in range(n_aux)] + ["_interm", "_dn"]}
    crit = C.SetDinoCriterion(CFG["K"], M.DinoHungarianMatcher(2.0, 5.0, 2.0, 0.25), weight, 0.25,
                              ["labels", "boxes", "cardinality"], None, None, small_loss=lambda *a: {}).train()
    losses = crit(out, prep["targets"], SimpleNamespace(device="cuda", img_res=224), {})
    assert all(k in losses for k in weight), sorted(set(weight) - set(losses))
    total = sum(losses[k] * w for k, w in weight.items())
    assert all(bool(torch.isfinite(v)) for v in losses.values()), {k: float(v) for k, v in losses.items()}
    total.backward()
    grads = [p.grad for _, p in model.named_parameters() if p.grad is not None]
    assert len(grads) > 50 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert model.key_embed[0].layers[0].weight.grad.abs().sum() > 0
    opt.step()                                          # the package's AdamW closes the step: nothing here is the reference's
    after = model.key_embed[0].layers[0].weight.detach()
    assert bool(torch.isfinite(after).all()) and not torch.equal(after, before)


def test_zz_print_ratios():
    for k in sorted(RATIOS):
        print("worst ratio %-72s %.2f" % (k, RATIOS[k]))
