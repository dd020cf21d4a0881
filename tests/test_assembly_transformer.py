"""The AssemblyHands DeformableTransformer (uvhand_amd.modules.AssemblyDeformableTransformer): construction against the
reference's (tests/golden/assembly_*.npz, made by gen_golden_r07.py) and the composition route on the CPU, end to end,
with the sampling itself on the oracle's pure-PyTorch core (the library's op refuses CPU tensors, as the reference's
does).  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import assembly_inputs as AI  # noqa: E402
import two_stage_inputs as TI  # noqa: E402

from uvhand_amd.functions import assembly_func as AF  # noqa: E402


def _fixture(name):
    return np.load(os.path.join(HERE, "golden", "assembly_%s.npz" % name))


def _build(name):
    from uvhand_amd.modules import AssemblyDeformableTransformer
    cfg = AI.CONFIGS[name]
    torch.manual_seed(cfg["wseed"])
    tr = AssemblyDeformableTransformer(**AI.build_kwargs(cfg))
    AI.attach_heads(tr, cfg)
    return tr, cfg


def test_imports_and_exports():
    import uvhand_amd.modules as m
    from uvhand_amd.modules import (AssemblyDeformableTransformer, AssemblyDeformableTransformerDecoder, DeformableTransformer,
                                    DeformableTransformerDecoder)
    for name in ("AssemblyDeformableTransformer", "AssemblyDeformableTransformerDecoder", "MSDeformAttn",
                 "DeformableTransformerEncoderLayer", "DeformableTransformerDecoderLayer", "DeformableTransformerEncoder",
                 "DeformableTransformerDecoder", "DeformableTransformer"):
        assert name in m.__all__, name
    assert AssemblyDeformableTransformer is not DeformableTransformer
    assert AssemblyDeformableTransformerDecoder is not DeformableTransformerDecoder
    assert DeformableTransformer.__module__.endswith("deformable_transformer")


def test_named_children_in_order():
    from uvhand_amd.modules import AssemblyDeformableTransformer
    two = AssemblyDeformableTransformer(two_stage=True, cfg="c")
    assert [n for n, _ in two.named_children()] == ["encoder", "decoder", "enc_output", "enc_output_norm", "pos_trans",
                                                    "pos_trans_norm"]
    assert type(two.pos_trans) is nn.Linear and two.pos_trans.weight.shape == (512, 512)
    assert two.cfg == "c" and two.decoder.cfg == "c" and not hasattr(two, "two_stage_learn_xy")
    one = AssemblyDeformableTransformer()
    assert [n for n, _ in one.named_children()] == ["encoder", "decoder", "reference_points"]
    assert one.cfg is None
    dec = one.decoder
    assert [n for n, _ in dec.named_children()] == ["layers"]
    assert dec.cls_embed is None and dec.keypoint_embed is None and dec.obj_keypoint_embed is None
    AI.attach_heads(one, dict(AI.CONFIGS["one_stage"], d=256))
    assert [n for n, _ in dec.named_children()] == ["layers", "cls_embed", "keypoint_embed", "obj_keypoint_embed"]


@pytest.mark.parametrize("name", ["one_stage", "two_stage"])
def test_state_dict_keys_and_shapes(name):
    z = _fixture(name)
    sd = _build(name)[0].state_dict()
    assert list(sd.keys()) == [str(k) for k in z["state_names"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in z["state_shapes"]]


@pytest.mark.parametrize("name", ["one_stage", "two_stage"])
def test_seeded_construction_matches_reference(name):
    z = _fixture(name)
    names, sums = TI.state_checksums(_build(name)[0])
    assert names == [str(k) for k in z["state_names"]]
    bad = [n for n, a, b in zip(names, sums, z["state_checksums"]) if not np.array_equal(a, b)]
    assert not bad, "state_dict differs from the reference's construction: %s" % bad[:5]


class _CpuCore:
    """MSDeformAttnFunction's interface on the oracle's pure-PyTorch core (CPU only; test infrastructure)."""

    @staticmethod
    def apply(value, shapes, lsi, loc, attn, im2col_step):
        from oracle.torch_fallback import msda_torch_fallback
        return msda_torch_fallback(value, shapes, loc, attn)


@pytest.mark.parametrize("name", ["one_stage", "two_stage"])
def test_composition_route_on_cpu_reproduces_fixture(name, monkeypatch):
    import uvhand_amd.modules.ms_deform_attn as msda_mod
    monkeypatch.setattr(msda_mod, "MSDeformAttnFunction", _CpuCore)
    tr, cfg = _build(name)
    report = AI.compare(tr, cfg, _fixture(name), torch.device("cpu"), backward=(name == "two_stage"))
    for r in report:
        print("%-48s %.3e (bar %.0e)" % r)
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, "beyond the bars: " + "; ".join("%s %.3e > %.0e" % r for r in bad[:12])


def _refine_inputs(width, seed=0, N=2, Q=40, K=3):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(N, Q, width, generator=g) * 1.4 - 0.2
    return r, torch.randn(N, Q, K, generator=g), torch.randn(N, Q, 63, generator=g)


@pytest.mark.parametrize("width", [2, 42])
def test_refine_composition_is_the_reference_formula(width):
    r, cls, tmp = _refine_inputs(width)
    out = AF.refine(r, cls, tmp)                          # CPU tensors: the composition
    assert out.shape == (2, 40, 42) and not out.requires_grad
    hand = cls.argmax(-1) != 0
    assert hand.any() and (~hand).any()
    if width == 2:
        base = AF.inverse_sigmoid(r).repeat(1, 1, 21)
    else:
        mean = torch.stack([r[..., 0::2].mean(-1), r[..., 1::2].mean(-1)], -1)
        base = AF.inverse_sigmoid((mean + 0.5) / 2).repeat(1, 1, 21)
    delta = tmp.view(2, 40, 21, 3)[..., :2].reshape(2, 40, 42)
    exp = torch.where(hand[..., None], base + delta, base).sigmoid() * 2 - 0.5
    assert torch.allclose(out, exp, atol=1e-6, rtol=0)


def test_selection_composition_follows_the_loop():
    g = torch.Generator().manual_seed(4)
    N, S, K = 3, 16, 11
    cls = torch.randn(N, S, K, generator=g)
    cls[2] = -cls[2].abs() - 0.1                           # an all-negative frame: the object stays at row 0
    hand, obj = torch.randn(N, S, 63, generator=g), torch.randn(N, S, 63, generator=g)
    refp, idx = AF.select_queries(cls, hand, obj, return_indices=True)
    assert refp.shape == (N, 3, 2) and idx.shape == (N, 3)
    assert torch.equal(idx[:, 0], cls[..., 9].argmax(1)) and torch.equal(idx[:, 1], cls[..., 10].argmax(1))
    assert idx[2, 2] == 0
    for n in range(2):
        best, pick = 0.0, 0
        for k in range(1, 9):
            s, i = cls[n, :, k].max(0)
            if best < s:
                best, pick = s, int(i)
        assert idx[n, 2] == pick
    rows = torch.stack([hand[torch.arange(N), idx[:, 0]], hand[torch.arange(N), idx[:, 1]], obj[torch.arange(N), idx[:, 2]]], 1)
    assert torch.allclose(refp, torch.stack([rows[..., 0::3].sigmoid().mean(-1), rows[..., 1::3].sigmoid().mean(-1)], -1))
    with pytest.raises(IndexError):
        AF.select_queries(cls[..., :10], hand, obj)


def test_proposals_composition_on_cpu():
    g = torch.Generator().manual_seed(2)
    N, H, W, C = 2, 4, 5, 8
    memory = torch.randn(N, H * W, C, generator=g, requires_grad=True)
    mask = torch.zeros(N, H, W, dtype=torch.bool)
    mask[1, :, 3:] = True
    mask[1, 3:, :] = True
    mem_out, props = AF.encoder_output_proposals(memory, mask.flatten(1), [(H, W)])
    assert props.shape == (N, H * W, 2)
    dead = torch.isinf(props).all(-1)
    assert dead[mask.flatten(1)].all() and (mem_out[dead] == 0).all()
    assert torch.equal(mem_out[~dead], memory[~dead])
    # frame 0: valid 4 x 5 -> centres (w + 0.5) / 5, (h + 0.5) / 4, all inside (0.01, 0.99)
    p = torch.tensor([[(w + 0.5) / W, (h + 0.5) / H] for h in range(H) for w in range(W)])
    assert torch.allclose(props[0], torch.log(p / (1 - p)))


def test_knob_off_routes_composition(monkeypatch):
    monkeypatch.setattr(AF, "FUSED", False)
    assert not AF._plain_cuda_f32(torch.zeros(1))
    r, cls, tmp = _refine_inputs(2)
    assert not AF.refine_fusable(r, cls, tmp)
    assert torch.equal(AF.refine(r, cls, tmp), AF.refine_composition(r, cls, tmp))
