"""The DINO DeformableTransformer (uvhand_amd.modules.DinoDeformableTransformer and its encoder) against the reference's
(tests/golden/dino_transformer.npz, made by gen_dino_transformer.py): both forms of the two-stage block on the CPU, end to end,
outputs and gradients, with the sampling on the oracle's pure-PyTorch core; the checkpoint keys and the seeded initialisation;
the constructor refusals; the selection rule of ``dino_select_composition`` against a numpy restatement.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_transformer_inputs as TI  # noqa: E402

from uvhand_amd.functions import dino_func as DF  # noqa: E402
from uvhand_amd.modules import DinoDeformableTransformer as Transformer  # noqa: E402
from uvhand_amd.modules import DinoDeformableTransformerEncoderLayer as EncoderLayer  # noqa: E402
from uvhand_amd.modules import DinoTransformerEncoder as Encoder  # noqa: E402
from uvhand_amd.modules import build_dino_deformable_transformer  # noqa: E402
from uvhand_amd.modules.detr import MLP  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "dino_transformer.npz"))


class _CpuCore:
    """MSDeformAttnFunction's interface on the oracle's pure-PyTorch core (CPU only; test infrastructure)."""

    @staticmethod
    def apply(value, shapes, lsi, loc, attn, im2col_step):
        from oracle.torch_fallback import msda_torch_fallback
        return msda_torch_fallback(value, shapes, loc, attn)


@pytest.fixture
def cpu_core(monkeypatch):
    import uvhand_amd.modules.ms_deform_attn as msda_mod
    monkeypatch.setattr(msda_mod, "MSDeformAttnFunction", _CpuCore)


numpy_rule = TI.numpy_select_rule


def test_exports():
    import uvhand_amd.modules as m
    for name in ("DinoDeformableTransformer", "DinoTransformerEncoder", "DinoDeformableTransformerEncoderLayer",
                 "build_dino_deformable_transformer"):
        assert name in m.__all__ and hasattr(m, name)
    assert Transformer is not m.DeformableTransformer and Encoder is not m.DeformableTransformerEncoder
    assert callable(DF.select_queries_dino) and callable(DF.dino_select_composition)


@pytest.mark.parametrize("case", list(TI.CASES))
def test_state_dict_keys_and_seeded_initialisation(case, fixture):
    torch.manual_seed(TI.INIT_SEED)
    tr = TI.construct(Transformer, case)
    sd = tr.state_dict()
    assert list(sd.keys()) == [str(k) for k in fixture[case + "/state_keys"]]
    sums = np.asarray([float(v.double().sum()) for v in sd.values()])
    assert np.array_equal(sums, fixture[case + "/init_sums"]), "the seeded construction consumes the RNG differently"
    assert tr.enc_out_class_embed is None and tr.enc_out_bbox_embed is None
    assert (tr.tgt_embed is not None) == TI.CASES[case]["embed_init_tgt"]
    assert (tr.two_stage_wh_embedding is not None) == TI.CASES[case]["learn_wh"]


@pytest.mark.parametrize("case", list(TI.CASES))
def test_fixture_condition(case, fixture):
    assert float(fixture[case + "/row_margin"]) >= TI.MIN_MARGIN
    assert float(fixture[case + "/class_margin"]) >= TI.MIN_MARGIN
    assert (fixture[case + "/dec_margin"] >= TI.MIN_MARGIN).all()
    assert set(fixture[case + "/codes"].flatten().tolist()) == {0, 1, 2}
    assert float(fixture[case + "/proposals_err"]) == 0.0
    dead = np.concatenate([m.reshape(m.shape[0], -1) for m in TI.inputs(case)["masks"]], 1)
    assert dead[1].any() and not dead[0].any(), "one frame has a padded right / bottom border"
    assert not np.take_along_axis(dead, fixture[case + "/topk"], 1).any()


def _check(report):
    for r in report:
        print("%-64s %.3e (bar %.0e)" % r)
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, "beyond the bars: " + "; ".join("%s %.3e > %.0e" % r for r in bad[:12])


@pytest.mark.parametrize("case", list(TI.CASES))
def test_reference_structure_on_cpu_reproduces_fixture(case, fixture, cpu_core):
    tr = TI.build(Transformer, MLP, case)
    prep = TI.prepare(case)
    assert not tr.heads_after_selection(torch.zeros(2, 43, 14), torch.zeros(2, 43, 256), torch.zeros(2, 43, 42))
    _check(TI.compare(tr, case, fixture))
    ret = tr(prep["srcs"], prep["masks"], prep["dn_ref"], prep["poss"], prep["dn_tgt"], prep["attn_mask"])
    assert ret[3][0].requires_grad is False and ret[3][1].requires_grad is False and ret[4].requires_grad is False
    assert ret[2].requires_grad


@pytest.mark.parametrize("case", list(TI.CASES))
def test_heads_after_selection_on_cpu_reproduces_fixture(case, fixture, cpu_core):
    tr = TI.build(Transformer, MLP, case)
    tr.two_stage_route = "selected"                     # dino_select_composition on CPU tensors, the heads on the Q rows
    _check(TI.compare(tr, case, fixture))
    assert np.array_equal(tr.last_topk_proposals.numpy(), fixture[case + "/topk"])


def test_hooked_or_foreign_heads_keep_the_reference_structure():
    from uvhand_amd.modules.dino_deformable_transformer import _plain_head
    lin, mlp = nn.Linear(8, 4), MLP(8, 8, 4, 3)
    assert _plain_head(lin) and _plain_head(mlp)
    h = mlp.layers[1].register_forward_hook(lambda *a: None)
    assert not _plain_head(mlp)
    h.remove()
    assert _plain_head(mlp)
    assert not _plain_head(nn.Sequential(nn.Linear(8, 4)))
    h = lin.register_forward_pre_hook(lambda *a: None)
    assert not _plain_head(lin)
    h.remove()


def test_constructor_refusals():
    for option in ("use_deformable_box_attn", "add_channel_attention", "two_stage_keep_all_tokens"):
        with pytest.raises(NotImplementedError, match=option):
            TI.construct(Transformer, "embed", **{option: True})
    with pytest.raises(AssertionError):
        TI.construct(Transformer, "embed", learnable_tgt_init=False)
    with pytest.raises(AssertionError):
        TI.construct(Transformer, "embed", layer_share_type="both")
    with pytest.raises(NotImplementedError):
        TI.construct(Transformer, "embed", decoder_sa_type="ca_label")
    with pytest.raises(NotImplementedError):
        TI.construct(Transformer, "embed", deformable_encoder=False, num_feature_levels=1)
    with pytest.raises(NotImplementedError):
        EncoderLayer(use_deformable_box_attn=True)
    with pytest.raises(NotImplementedError):
        Encoder(EncoderLayer(d_ffn=64), 1, deformable_encoder=False)


def test_two_stage_no_constructs_and_raises_in_forward():
    tr = TI.construct(Transformer, "embed", two_stage_type="no")
    keys = {k.split(".")[0] for k in tr.state_dict()}
    assert "refpoint_embed" in keys and "tgt_embed" in keys and "enc_output" not in keys
    assert tuple(tr.refpoint_embed.weight.shape) == (TI.CFG["queries"], 4)
    prep = TI.prepare("embed")
    with pytest.raises(NotImplementedError, match="unknown two_stage_type no"):
        tr(prep["srcs"], prep["masks"], None, prep["poss"], None)


def test_builder_reads_the_reference_arguments():
    from types import SimpleNamespace
    args = SimpleNamespace(decoder_layer_noise=False, hidden_dim=256, dropout=0.0, nheads=8, num_queries=7, dim_feedforward=64,
                           enc_layers=1, unic_layers=0, dec_layers=1, pre_norm=False, query_dim=4, transformer_activation="relu",
                           num_patterns=0, num_feature_levels=3, enc_n_points=4, dec_n_points=4, use_deformable_box_attn=False,
                           box_attn_type="roi_align", add_channel_attention=False, add_pos_value=False, random_refpoints_xy=False,
                           two_stage_type="standard", two_stage_pat_embed=0, two_stage_add_query_num=0,
                           two_stage_keep_all_tokens=False, dec_layer_number=None, decoder_sa_type="sa",
                           decoder_module_seq=["sa", "ca", "ffn"], embed_init_tgt=True)
    tr = build_dino_deformable_transformer(args)
    assert isinstance(tr, Transformer) and tr.two_stage_learn_wh and tr.two_stage_wh_embedding is not None
    assert tr.decoder.return_intermediate and tr.num_queries == 7


def test_get_valid_ratio():
    tr = TI.construct(Transformer, "embed")
    m = torch.zeros(2, 6, 5, dtype=torch.bool)
    m[1, 4:, :] = True
    m[1, :, 3:] = True
    assert torch.equal(tr.get_valid_ratio(m), torch.tensor([[1.0, 1.0], [3 / 5, 4 / 6]]))


# ---- the selection rule ---------------------------------------------------------------------------------------------------
def _rule_case(cls, Q):
    cls = torch.as_tensor(cls, dtype=torch.float32)
    N, S, _ = cls.shape
    mem = torch.arange(N * S * 4, dtype=torch.float32).view(N, S, 4)
    prop = torch.arange(N * S * 42, dtype=torch.float32).view(N, S, 42) * 0.5
    topk, tgt, prop_sel, code = DF.select_queries_dino(cls, mem, prop, Q)
    want_topk, want_code = numpy_rule(cls.numpy(), Q)
    assert np.array_equal(topk.numpy(), want_topk), (topk, want_topk)
    assert np.array_equal(code.numpy(), want_code)
    assert torch.equal(tgt, torch.gather(mem, 1, topk[..., None].expand(-1, -1, 4)))
    assert torch.equal(prop_sel, torch.gather(prop, 1, topk[..., None].expand(-1, -1, 42)))
    return topk


def test_composition_rule_ties():
    topk = _rule_case(np.full((2, 40, 14), 0.25, dtype=np.float32), 9)
    assert topk.tolist() == [list(range(9))] * 2


def test_composition_rule_nan_inf_zero():
    rs = np.random.RandomState(11)
    cls = rs.standard_normal((2, 50, 14)).astype(np.float32)
    cls[0, 7, 3] = np.nan                       # a NaN row ranks first; its argmax is the NaN's class
    cls[0, 30, 13] = np.nan
    cls[0, 30, 2] = np.nan
    cls[0, 9, 12] = np.inf
    cls[0, 4, 5] = np.inf                       # two +inf rows: the lower row first
    cls[1, 20] = -np.inf                        # a row of -inf sorts last
    cls[1, 5:12] = -1.0
    cls[1, 5, 0] = 0.0
    cls[1, 6, 1] = -0.0                         # -0 equals +0: rows 5 and 6 tie, the lower row first
    cls[1, :, :] = np.minimum(cls[1], 0.0)
    topk = _rule_case(cls, 12)
    assert topk[0, :4].tolist() == [7, 30, 4, 9]
    first_zero = [r for r in topk[1].tolist() if r in (5, 6)]
    assert first_zero == [5, 6]
    topk = _rule_case(cls, 50)
    assert topk[1, -1].item() == 20


def test_composition_raises_torchs_error_for_k_beyond_rows():
    with pytest.raises(RuntimeError, match="out of range"):
        DF.select_queries_dino(torch.zeros(1, 5, 3), torch.zeros(1, 5, 4), torch.zeros(1, 5, 42), 6)


def test_select_gradient_routing_on_cpu():
    g = torch.Generator().manual_seed(2)
    cls = torch.randn(2, 30, 14, generator=g).requires_grad_(True)
    mem = torch.randn(2, 30, 8, generator=g).requires_grad_(True)
    prop = torch.randn(2, 30, 42, generator=g).requires_grad_(True)
    topk, tgt, prop_sel, code = DF.select_queries_dino(cls, mem, prop, 5)
    assert tgt.requires_grad and not prop_sel.requires_grad and not code.requires_grad
    w = torch.randn(2, 5, 8, generator=g)
    (tgt * w).sum().backward()
    want = torch.zeros(2, 30, 8).scatter_(1, topk[..., None].expand(-1, -1, 8), w)
    assert torch.equal(mem.grad, want) and cls.grad is None and prop.grad is None
