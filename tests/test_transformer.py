"""DeformableTransformer (uvhand_amd.modules): construction against the reference's (tests/golden/transformer_*.npz, made by
gen_golden_r06.py) and the two-stage pieces' composition route on the CPU.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import two_stage_inputs as TI  # noqa: E402

from uvhand_amd.functions import two_stage_func as TS  # noqa: E402


def _fixture(name):
    return np.load(os.path.join(HERE, "golden", "transformer_%s.npz" % name))


def _build(name):
    from uvhand_amd.modules import DeformableTransformer
    cfg = TI.CONFIGS[name]
    torch.manual_seed(cfg["wseed"])
    tr = DeformableTransformer(d_model=cfg["d"], nhead=cfg["heads"], num_encoder_layers=cfg["enc"], num_decoder_layers=cfg["dec"],
                               dim_feedforward=cfg["ffn"], dropout=0.0, return_intermediate_dec=True,
                               num_feature_levels=len(cfg["shapes"]), two_stage=cfg["two_stage"], two_stage_num_proposals=cfg["Q"],
                               two_stage_learn_xy=True)
    TI.attach_heads(tr, cfg, 42 if cfg["two_stage"] else 2)
    return tr


def test_module_imports_and_constructs():
    from uvhand_amd.modules import DeformableTransformer
    import uvhand_amd.modules as m
    assert "DeformableTransformer" in m.__all__
    tr = DeformableTransformer(two_stage=True)
    names = [n for n, _ in tr.named_children()]
    assert names == ["encoder", "decoder", "enc_output", "enc_output_norm", "pos_trans", "pos_trans_norm", "two_stage_learn_xy"]
    assert isinstance(tr.pos_trans, nn.Sequential) and tr.state_dict()["pos_trans.0.weight"].shape == (1024, 5376)
    one = DeformableTransformer()
    assert [n for n, _ in one.named_children()] == ["encoder", "decoder", "reference_points"]
    assert one.two_stage_learn_xy is None
    assert torch.equal(tr.two_stage_learn_xy.weight, torch.full((1, 40), math.log(0.05 / 0.95)))


@pytest.mark.parametrize("name", ["two_stage", "one_stage"])
def test_state_dict_keys_and_shapes(name):
    z = _fixture(name)
    sd = _build(name).state_dict()
    assert list(sd.keys()) == [str(k) for k in z["state_names"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in z["state_shapes"]]


@pytest.mark.parametrize("name", ["two_stage", "one_stage"])
def test_seeded_construction_matches_reference(name):
    z = _fixture(name)
    names, sums = TI.state_checksums(_build(name))
    assert names == [str(k) for k in z["state_names"]]
    bad = [n for n, a, b in zip(names, sums, z["state_checksums"]) if not np.array_equal(a, b)]
    assert not bad, "state_dict differs from the reference's construction: %s" % bad[:5]


def _two_stage_cpu_inputs(seed=0, N=2, shapes=((6, 5), (3, 3), (2, 1))):
    g = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in shapes)
    memory = torch.randn(N, S, 16, generator=g, requires_grad=True)
    masks = []
    for (h, w) in shapes:
        m = torch.zeros(N, h, w, dtype=torch.bool)
        m[1, :, w - max(1, w // 3):] = True
        m[0, 0, w - 1:] = True if w > 1 else False
        masks.append(m.flatten(1))
    return memory, torch.cat(masks, 1), list(shapes)


def test_proposals_composition_on_cpu():
    memory, mask, hw = _two_stage_cpu_inputs()
    xy = torch.full((40,), math.log(0.05 / 0.95), requires_grad=True)
    out_mem, props = TS.encoder_output_proposals(memory, mask, hw, xy)
    ref_mem, ref_props = TS.proposals_composition(memory, mask, hw, xy)
    assert torch.equal(out_mem, ref_mem) and torch.equal(props, ref_props)
    assert torch.isinf(props[mask]).all()
    assert (out_mem[mask] == 0).all()
    # the learned offsets reach the graph only through sliced-away columns: their gradient is zeros, not None
    (out_mem.sum() + props[..., 0:2].masked_fill(torch.isinf(props[..., 0:2]), 0).sum()).backward()
    assert xy.grad is not None and torch.count_nonzero(xy.grad) == 0


def test_selection_and_pos_trans_composition_on_cpu():
    g = torch.Generator().manual_seed(3)
    N, S, K, Q = 2, 40, 14, 7
    cls = torch.randn(N, S, K, generator=g)
    hand, obj, prop = (torch.randn(N, S, 42, generator=g) for _ in range(3))
    ref, refp, idx = TS.select_queries(cls, hand, obj, prop, Q, return_indices=True)
    assert torch.equal(idx, torch.topk(cls.max(-1)[0], Q, dim=1)[1])
    assert torch.equal(refp, ref.sigmoid() * 2 - 1)
    with pytest.raises(RuntimeError):
        TS.select_queries(cls, hand, obj, prop, S + 1)
    pe = TS.proposal_pos_embed(ref)
    assert pe.shape == (N, Q, 5376)
    u = ref.sigmoid()[..., :, None] * (2 * math.pi) / TS.pe_dim_t("cpu")
    assert torch.allclose(pe.view(N, Q, 42, 64, 2)[..., 0], u[..., 0::2].sin(), atol=1e-6)
    torch.manual_seed(0)
    pos_trans = nn.Sequential(nn.Linear(5376, 1024), nn.ReLU(), nn.Linear(1024, 1024), nn.ReLU(), nn.Linear(1024, 512), nn.ReLU())
    norm = nn.LayerNorm(512)
    out = TS.pos_trans_embed(pos_trans, norm, ref)
    assert torch.equal(out, norm(pos_trans(pe)))


def test_knob_off_routes_composition(monkeypatch):
    monkeypatch.setattr(TS, "FUSED", False)
    assert not TS._plain_cuda_f32(torch.zeros(1))
    pos_trans = nn.Sequential(nn.Linear(5376, 8), nn.ReLU(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 8), nn.ReLU())
    assert not TS.pos_trans_fusable(pos_trans, torch.zeros(1, 42))
    memory, mask, hw = _two_stage_cpu_inputs(1)
    out_mem, props = TS.encoder_output_proposals(memory, mask, hw, None)
    ref_mem, ref_props = TS.proposals_composition(memory, mask, hw, None)
    assert torch.equal(props, ref_props) and torch.equal(out_mem, ref_mem)
