"""The DINO model class (uvhand_amd.modules.DINO) and functions.heads_func.dino_heads on the CPU: the seeded construction, the
output dict and every tensor and gradient of the fixture that the reference's own class produced
(tests/golden/gen_dino_model.py), and the heads' composition against a per-layer loop and torch.autograd.gradcheck."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_model_inputs as MI  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "dino_model.npz"))


@pytest.fixture(autouse=True)
def _cpu_sampling(monkeypatch):
    """The library's sampling op refuses CPU tensors: the oracle's pure-PyTorch core serves it here, as in the generator."""
    import uvhand_amd.modules.ms_deform_attn as msda_mod
    from oracle.torch_fallback import msda_torch_fallback

    class _CpuCore:
        @staticmethod
        def apply(value, shapes, lsi, loc, attn, im2col_step):
            return msda_torch_fallback(value, shapes, loc, attn)

    monkeypatch.setattr(msda_mod, "MSDeformAttnFunction", _CpuCore)


def _classes():
    from uvhand_amd.modules import DINO, DinoDeformableTransformer
    return DINO, DinoDeformableTransformer


@pytest.mark.parametrize("case", list(MI.CASES))
def test_seeded_construction_is_the_references(case, fixture):
    torch.manual_seed(MI.INIT_SEED)
    bare = MI.construct(*_classes(), case)
    sd = bare.state_dict()
    assert list(sd.keys()) == [str(k) for k in fixture[case + "/state_keys"]]
    sums = np.asarray([float(v.double().sum()) for v in sd.values()], dtype=np.float64)
    assert np.array_equal(sums, fixture[case + "/init_sums"])


def test_heads_are_shared_as_the_reference_shares_them():
    m = MI.construct(*_classes(), "train")
    tr = m.transformer
    assert all(x is m.class_embed[0] for x in m.class_embed) and tr.decoder.class_embed is m.class_embed
    assert tr.decoder.key_embed is m.key_embed and tr.decoder.obj_key_embed is m.obj_key_embed
    assert tr.enc_out_class_embed is m.class_embed[0] and tr.enc_out_key_embed is m.key_embed[0]
    assert tr.enc_out_obj_key_embed is m.obj_key_embed[0]
    assert m.label_embedding is None and all(layer.label_embedding is None for layer in tr.decoder.layers)
    own = MI.construct(*_classes(), "train_own_enc_heads")
    assert own.transformer.enc_out_key_embed is not own.key_embed[0] and own.transformer.enc_out_class_embed is own.class_embed[0]
    split = MI.construct(*_classes(), "train", dec_pred_bbox_embed_share=False, two_stage_bbox_embed_share=False,
                         two_stage_class_embed_share=False)
    assert split.key_embed[0] is not split.key_embed[1] and split.transformer.enc_out_class_embed is not split.class_embed[0]
    with pytest.raises(Exception, match="Not implemented."):
        MI.construct(*_classes(), "train", dec_pred_class_embed_share=False)
    with pytest.raises(AssertionError):
        MI.construct(*_classes(), "train", dec_pred_bbox_embed_share=False)      # two_stage_bbox_embed_share needs both shared
    with pytest.raises(AssertionError):
        MI.construct(*_classes(), "train", iter_update=False)


@pytest.mark.parametrize("case", list(MI.CASES))
def test_model_reproduces_the_fixture(case, fixture):
    model = MI.build(*_classes(), case)
    prep = MI.prepare(case)
    out, _, _ = MI.step(model, prep, backward=False)
    assert MI.key_order(out) == [str(k) for k in fixture[case + "/key_order"]]
    assert list(out.keys())[:6] == ["pred_logits", "pred_hand_key", "pred_obj_key", "pred_mano_params", "pred_cams",
                                    "pred_obj_params"]
    assert list(out.keys())[6:] == ["aux_outputs", "interm_outputs", "dn_meta"]
    report = MI.compare(MI.build(*_classes(), case), case, fixture)
    for r in report:
        print("%-72s %.3e (bar %.0e)" % r)
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, "beyond the bars: " + "; ".join("%s %.3e > %.0e" % r for r in bad[:12])


def test_interm_hand_key_is_the_first_of_ref_enc():
    """dino.py:376-378 unpack ref_enc as (obj, hand) and emit the first as pred_hand_key."""
    model = MI.build(*_classes(), "eval")
    seen = {}
    real = model.heads
    model.heads = lambda hs, reference, hs_enc, ref_enc, dn_meta: (seen.update(ref=ref_enc), real(hs, reference, hs_enc, ref_enc, dn_meta))[1]
    out, _, _ = MI.step(model, MI.prepare("eval"), backward=False)
    assert torch.equal(out["interm_outputs"]["pred_hand_key"], seen["ref"][0][-1])
    assert torch.equal(out["interm_outputs"]["pred_obj_key"], seen["ref"][1][-1])


def test_enc_outputs_branch_fails_as_the_references():
    model = MI.build(*_classes(), "eval")
    hs = [torch.zeros(2, 3, 256) for _ in range(2)]
    ref = [torch.full((2, 3, 42), 0.5) for _ in range(3)]
    with pytest.raises(AttributeError, match="enc_bbox_embed"):
        model.heads(hs, ref, torch.zeros(2, 2, 3, 256), [torch.zeros(2, 2, 3, 42)] * 2, None)


# ---- dino_heads on the CPU ----------------------------------------------------------------------------------------------------
def _heads(C, K, L, shared_mods, dtype, seed=0):
    from uvhand_amd.modules.detr import MLP
    torch.manual_seed(seed)
    n = 1 if shared_mods else L
    cls = [nn.Linear(C, K) for _ in range(n)]
    key = [MLP(C, C, 42, 3) for _ in range(n)]
    obj = [MLP(C, C, 42, 3) for _ in range(n)]
    shared = [nn.Linear(C, w) for w in (48, 10, 3, 3, 3, 1)]
    for m in cls + key + obj + shared:
        m.to(dtype)
    rep = lambda ms: nn.ModuleList([ms[0]] * L if shared_mods else ms)
    return rep(cls), rep(key), rep(obj), shared


def _inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


@pytest.mark.parametrize("shared_mods", [True, False])
@pytest.mark.parametrize("stacked", [False, True])
def test_dino_heads_equals_the_per_layer_loop(shared_mods, stacked):
    from uvhand_amd.functions.heads_func import dino_heads
    L, N, Q, C, K = 3, 2, 5, 16, 14
    cls, key, obj, shared = _heads(C, K, L, shared_mods, torch.float32)
    g = torch.Generator().manual_seed(1)
    hs = [torch.randn(N, Q, C, generator=g, requires_grad=True) for _ in range(L)]
    refs = [(torch.rand(N, Q, 42, generator=g) * 2 - 1).requires_grad_(l > 0) for l in range(L)]
    logits, (hand, objk), sh = dino_heads(torch.stack(hs) if stacked else hs, refs, cls, key, obj, shared)
    for l in range(L):
        assert torch.equal(logits[l], cls[l](hs[l]))
        assert torch.equal(hand[l], (key[l](hs[l]) + _inverse_sigmoid(refs[l])).sigmoid() * 2 - 1)
        assert torch.equal(objk[l], (obj[l](hs[l]) + _inverse_sigmoid(refs[l])).sigmoid() * 2 - 1)
        for o, lin in zip(sh, shared):
            assert torch.equal(o[l], lin(hs[l]))
    assert logits.shape == (L, N, Q, K) and hand.shape == (L, N, Q, 42) and [o.shape[-1] for o in sh] == [48, 10, 3, 3, 3, 1]
    w = torch.randn(L, N, Q, 42, generator=g)
    ((hand + 2 * objk) * w).sum().backward()
    assert refs[0].grad is None and all(r.grad is not None and r.grad.abs().sum() > 0 for r in refs[1:])
    # outside [0, 1] the reference's clamp stops the gradient
    for r in refs[1:]:
        out = (r.detach() < 0) | (r.detach() > 1)
        assert out.any() and torch.equal(r.grad[out], torch.zeros_like(r.grad[out]))


def test_dino_heads_keeps_autocasts_dtypes():
    """DINO's logits stay what autocast makes them (dino.py:341), unlike ARCTIC's .to(float32)."""
    from uvhand_amd.functions.heads_func import dino_heads
    L, N, Q, C, K = 2, 1, 3, 16, 14
    cls, key, obj, shared = _heads(C, K, L, True, torch.float32)
    hs = [torch.randn(N, Q, C) for _ in range(L)]
    refs = [torch.rand(N, Q, 42) for _ in range(L)]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        logits, (hand, _), sh = dino_heads(hs, refs, cls, key, obj, shared)
    assert logits.dtype == torch.bfloat16 and sh[0].dtype == torch.bfloat16 and hand.dtype == torch.float32


def test_dino_heads_reference_gradient_passes_gradcheck():
    from uvhand_amd.functions.heads_func import dino_heads
    L, N, Q, C, K = 2, 1, 2, 8, 3
    cls, key, obj, shared = _heads(C, K, L, False, torch.float64)
    g = torch.Generator().manual_seed(2)
    hs = [torch.randn(N, Q, C, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(L)]
    # away from the clamp boundaries 0, eps, 1 - eps, 1: inside (0.05, 0.95), or outside [0, 1] by at least 0.05
    inner = torch.rand(L, N, Q, 42, generator=g, dtype=torch.float64) * 0.9 + 0.05
    outer = torch.where(torch.rand(L, N, Q, 42, generator=g) < 0.5, -0.05 - inner, 1.05 + inner)
    pts = torch.where(torch.rand(L, N, Q, 42, generator=g) < 0.3, outer, inner)
    refs = [pts[l].clone().requires_grad_(True) for l in range(L)]

    def fn(*leaves):
        logits, (hand, objk), sh = dino_heads(list(leaves[:L]), list(leaves[L:]), cls, key, obj, shared)
        return (logits, hand, objk) + tuple(sh)

    assert torch.autograd.gradcheck(fn, tuple(hs) + tuple(refs), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_build_dino_model_takes_build_dinos_arguments():
    from types import SimpleNamespace
    from uvhand_amd.modules import DINO, build_dino_model
    args = SimpleNamespace(
        num_classes=14, num_queries=10, random_refpoints_xy=False, fix_refpoints_hw=-1, num_feature_levels=3, nheads=8,
        two_stage_type="standard", two_stage_bbox_embed_share=False, two_stage_class_embed_share=False, decoder_sa_type="sa",
        num_patterns=0, use_dn=True, dn_number=5, dn_box_noise_scale=0.4, dn_label_noise_ratio=0.5,
        hidden_dim=256, dropout=0.0, dim_feedforward=32, enc_layers=1, unic_layers=0, dec_layers=2, pre_norm=False, query_dim=4,
        transformer_activation="relu", num_select=10, enc_n_points=2, dec_n_points=2, use_deformable_box_attn=False,
        box_attn_type="roi_align", learnable_tgt_init=True, decoder_query_perturber=None, add_channel_attention=False,
        add_pos_value=False, random_refpoints_xy_=False, two_stage_pat_embed=0, two_stage_add_query_num=0,
        two_stage_learn_wh=False, two_stage_default_hw=0.05, two_stage_keep_all_tokens=False, dec_layer_number=None,
        rm_self_attn_layers=None, key_aware_type=None, layer_share_type=None, rm_detach=None, decoder_layer_noise=False,
        dln_xy_noise=0.2, dln_hw_noise=0.2, decoder_module_seq=["sa", "ca", "ffn"], embed_init_tgt=True,
        use_detached_boxes_dec_out=False, use_checkpoint=False, use_transformer_ckpt=False, num_queries_=10)
    model = build_dino_model(args, MI.StubBackbone((6, 10), 256))
    assert isinstance(model, DINO) and model.dn_number == 5 and model.dn_labelbook_size == 14 and model.aux_loss
    assert model.transformer.enc_out_key_embed is not model.key_embed[0]
    args.use_dn = False
    assert build_dino_model(args, MI.StubBackbone((6, 10), 256)).dn_number == 0
