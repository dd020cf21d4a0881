"""The DINO decoder (uvhand_amd.modules.DinoTransformerDecoder / DinoDeformableTransformerDecoderLayer) against the reference's
(tests/golden/dino_decoder.npz, made by gen_dino_decoder.py): the composition route on the CPU, end to end, outputs and
gradients, with the sampling itself on the oracle's pure-PyTorch core (the library's op refuses CPU tensors); the checkpoint
keys; the constructor refusals.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_inputs as DI  # noqa: E402

from uvhand_amd.functions import dino_func as DF  # noqa: E402
from uvhand_amd.modules import DinoDeformableTransformerDecoderLayer as Layer  # noqa: E402
from uvhand_amd.modules import DinoTransformerDecoder as Decoder  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "dino_decoder.npz"))


class _CpuCore:
    """MSDeformAttnFunction's interface on the oracle's pure-PyTorch core (CPU only; test infrastructure)."""

    @staticmethod
    def apply(value, shapes, lsi, loc, attn, im2col_step):
        from oracle.torch_fallback import msda_torch_fallback
        return msda_torch_fallback(value, shapes, loc, attn)


def test_exports():
    import uvhand_amd.modules as m
    assert "DinoTransformerDecoder" in m.__all__ and "DinoDeformableTransformerDecoderLayer" in m.__all__
    assert Decoder is not m.DeformableTransformerDecoder and Layer is not m.DeformableTransformerDecoderLayer


@pytest.mark.parametrize("case", list(DI.CASES))
def test_composition_route_on_cpu_reproduces_fixture(case, fixture, monkeypatch):
    import uvhand_amd.modules.ms_deform_attn as msda_mod
    monkeypatch.setattr(msda_mod, "MSDeformAttnFunction", _CpuCore)
    dec = DI.build(Layer, Decoder, case)
    report = DI.compare(dec, case, fixture)
    for r in report:
        print("%-56s %.3e (bar %.0e)" % r)
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, "beyond the bars: " + "; ".join("%s %.3e > %.0e" % r for r in bad[:12])


@pytest.mark.parametrize("case", list(DI.CASES))
def test_fixture_condition(case, fixture):
    assert (fixture[case + "/margin"] >= DI.MIN_MARGIN).all()


@pytest.mark.parametrize("case", list(DI.CASES))
def test_state_dict_keys(case, fixture):
    dec = DI.build(Layer, Decoder, case)
    assert list(dec.state_dict().keys()) == [str(k) for k in fixture[case + "/state_keys"]]


def test_heads_start_unattached():
    dec = Decoder(Layer(d_ffn=64, decoder_sa_type="sa"), 1, nn.LayerNorm(256), return_intermediate=True, deformable_decoder=True,
                  rm_dec_query_scale=True)
    for name in ("class_embed", "key_embed", "obj_key_embed", "bbox_embed", "rm_detach"):
        assert getattr(dec, name) is None, name
    assert {k.split(".")[0] for k in dec.state_dict()} == {"layers", "norm", "ref_point_head"}
    assert [k for k in dec.state_dict() if k.startswith("ref_point_head")] == [
        "ref_point_head.layers.0.weight", "ref_point_head.layers.0.bias", "ref_point_head.layers.1.weight",
        "ref_point_head.layers.1.bias"]


def test_constructor_refusals():
    with pytest.raises(NotImplementedError):
        Layer(decoder_sa_type="ca_label")
    with pytest.raises(NotImplementedError):
        Layer(decoder_sa_type="ca_content")
    with pytest.raises(NotImplementedError):
        Layer(decoder_sa_type="sa", use_deformable_box_attn=True)
    with pytest.raises(AssertionError):
        Layer(decoder_sa_type="sa", module_seq=["sa", "ca"])
    layer = Layer(d_ffn=64, decoder_sa_type="sa")
    norm = nn.LayerNorm(256)
    with pytest.raises(NotImplementedError):
        Decoder(layer, 1, norm, return_intermediate=True, deformable_decoder=False, rm_dec_query_scale=True)
    with pytest.raises(NotImplementedError):
        Decoder(layer, 1, norm, return_intermediate=True, deformable_decoder=True, rm_dec_query_scale=False)
    with pytest.raises(AssertionError):
        Decoder(layer, 1, norm, return_intermediate=True, query_dim=3, deformable_decoder=True, rm_dec_query_scale=True)
    with pytest.raises(AssertionError):
        Decoder(layer, 1, norm, return_intermediate=False, deformable_decoder=True, rm_dec_query_scale=True)


def test_dec_layer_number_raises_as_the_reference(monkeypatch):
    import uvhand_amd.modules.ms_deform_attn as msda_mod
    monkeypatch.setattr(msda_mod, "MSDeformAttnFunction", _CpuCore)
    dec = DI.build(Layer, Decoder, "w42")
    dec.dec_layer_number = [15, 15]
    with pytest.raises(Exception, match="Not implemented"):
        DI.run(dec, "w42")


def test_module_seq_and_rm_self_attn(monkeypatch):
    """Any permutation of the three blocks runs, and a layer without its self-attention modules skips that block."""
    import uvhand_amd.modules.ms_deform_attn as msda_mod
    monkeypatch.setattr(msda_mod, "MSDeformAttnFunction", _CpuCore)
    dec = DI.build(Layer, Decoder, "w42")
    for layer in dec.layers:
        layer.module_seq = ["ca", "ffn", "sa"]
        layer.key_aware_type = "mean"
    outs, _ = DI.run(dec, "w42")
    assert all(torch.isfinite(o).all() for o in outs)
    dec.layers[0].rm_self_attn_modules()
    assert dec.layers[0].self_attn is None and dec.layers[0].norm2 is None
    outs, _ = DI.run(dec, "w42")
    assert all(torch.isfinite(o).all() for o in outs)


def test_sine_embed_composition_layout():
    """y first, sin / cos interleaved, torch's table: against a direct fp64 statement."""
    g = torch.Generator().manual_seed(3)
    pos = torch.rand(5, 3, 42, generator=g) * 2 - 1
    valid = torch.rand(3, 2, generator=g) * 0.5 + 0.5
    pe = DF.sine_embed_for_position(pos, valid)                         # CPU tensors: the composition
    assert pe.shape == (5, 3, 256)
    p64 = pos.double() * valid.double().repeat(1, 21)[None]
    ex, ey = p64[..., 0::2].mean(-1) * 2 * np.pi, p64[..., 1::2].mean(-1) * 2 * np.pi
    i = torch.arange(64, dtype=torch.float64)
    d = 10000.0 ** (2 * i / 128)
    ref = torch.cat([torch.stack([(e[..., None] / d).sin(), (e[..., None] / d).cos()], -1).flatten(-2) for e in (ey, ex)], -1)
    assert float((pe.double() - ref).abs().max()) < 1e-5


def test_refine_composition_rule_and_gradient_routing():
    g = torch.Generator().manual_seed(5)
    ref = torch.rand(6, 2, 42, generator=g) * 2 - 1
    cls = torch.randn(6, 2, 14, generator=g)
    cls[0, 0, 0] = 50.0                                                  # class 0: stays
    cls[1, 0, 12] = 50.0                                                 # hand
    cls[2, 0, 5] = 50.0                                                  # object
    dk = torch.randn(6, 2, 42, generator=g).requires_grad_(True)
    do = torch.randn(6, 2, 42, generator=g).requires_grad_(True)
    out = DF.refine(ref, cls, dk, do)
    out.sum().backward()
    c = cls.argmax(-1)
    hand = (c == 12) | (c == 13)
    obj = ~hand & (c != 0)
    assert (dk.grad[~hand] == 0).all() and (do.grad[~obj] == 0).all()
    assert (dk.grad[hand] != 0).any() and (do.grad[obj] != 0).any()
    stay = ~hand & ~obj
    u = DF.inverse_sigmoid(ref)
    assert torch.equal(out[stay], u[stay].sigmoid() * 2 - 1)
    gu = (1 - out.detach() ** 2) / 2                                     # the kernel's backward formula
    assert torch.allclose(dk.grad[hand], gu[hand], rtol=1e-5, atol=1e-7)


def test_knob_values(monkeypatch):
    assert DF.QUERY_POS_ROUTE in ("table", "fused")
    monkeypatch.setattr(DF, "FUSED", False)
    assert not DF._plain_cuda_f32(torch.zeros(1))
