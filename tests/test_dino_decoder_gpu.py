"""The DINO decoder (uvhand_amd.modules.DinoTransformerDecoder) on the GPU at the fixture's shape (tests/golden/dino_inputs.py):
the fused route held to the project's accuracy rule against an fp64 copy of the module, the step under
torch.cuda.set_sync_debug_mode("error") — where the composition route, with the reference's boolean-mask adds, raises —, the
step captured in one graph, and the masked self-attention core reached from the layer."""
import copy
import gc
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_inputs as DI  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = {}


def _dev():
    return torch.device("cuda:0")


def _build(case):
    from uvhand_amd.modules import DinoDeformableTransformerDecoderLayer, DinoTransformerDecoder
    return DI.build(DinoDeformableTransformerDecoderLayer, DinoTransformerDecoder, case).to(_dev())


def _plain_torch(monkeypatch):
    """The module on its composition route (MSDA_DINO_FUSED=0): the reference's own query positions and refinement in torch
    ops.  In fp64 every other piece of the layer falls back to its torch module as well; in fp32 they stay what the package
    ships, so the yardstick's error and the fused route's differ by the pieces under test alone.  (A first form of this test also
    replaced the fp32 yardstick's attention, LayerNorm and FFN nodes by the plain modules.  The 42-wide case passed; in the
    2-wide case one tensor missed the bar — the two-element bias gradient of key_embed.0.layers.2, a cancelling sum over 30 rows:
    7.07e-8 against a yardstick of 1.49e-8, one fp32 ulp of its largest value — through rounding differences of nodes that
    were there before, not of the kernels this file is about.)"""
    from uvhand_amd.functions import dino_func as DF
    monkeypatch.setattr(DF, "FUSED", False)


@pytest.mark.parametrize("ref_grad", [True, False])
@pytest.mark.parametrize("case", list(DI.CASES))
def test_fused_route_holds_the_ratio_rule(case, ref_grad, monkeypatch):
    """ref_grad=False: every layer on the kernels; True (the fixture's form): the first layer's points require grad."""
    dec = _build(case)
    outs, leaves = DI.run(dec, case, _dev(), ref_grad=ref_grad)
    ours = [o.detach() for o in outs] + [leaves[k].grad for k in leaves] + [p.grad for _, p in sorted(dec.named_parameters())]
    names = DI.labels() + ["grad_" + k for k in leaves] + ["pgrad " + k for k, _ in sorted(dec.named_parameters())]
    _plain_torch(monkeypatch)
    got = []
    for dt in (torch.float32, torch.float64):
        d2 = copy.deepcopy(dec).to(dt)
        d2.zero_grad(set_to_none=True)
        o2, l2 = DI.run(d2, case, _dev(), dt, ref_grad=ref_grad)
        got.append([o.detach() for o in o2] + [l2[k].grad for k in l2] + [p.grad for _, p in sorted(d2.named_parameters())])
    for name, a, b, c in zip(names, ours, got[0], got[1]):
        assert (a is None) == (c is None), name
        if a is not None:
            DI.hold("%s%s %s" % (case, "" if ref_grad else " detached", name), a, b, c, RATIOS)


def test_step_makes_no_host_sync_and_the_composition_does(monkeypatch):
    from uvhand_amd.functions import dino_func as DF
    dec = _build("w42")
    prep = DI.prepare("w42", _dev(), ref_grad=False)
    DI.step(dec, prep)                                   # warm-up: MSDeformAttn verifies the pyramid's shapes once per tensor
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = DI.step(dec, prep)                        # forward + backward: nothing may synchronise
        monkeypatch.setattr(DF, "FUSED", False)
        with pytest.raises(RuntimeError):
            DI.step(dec, prep)                           # the reference's boolean-mask adds: a nonzero each
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(o).all() for o in outs)


def test_step_replays_from_one_graph(monkeypatch):
    """Forward plus backward captured once and replayed on new inputs equals the eager result bit for bit (the fixture has
    dropout 0; the sampling's backward takes its deterministic kernels so that two runs can be compared at all)."""
    monkeypatch.setenv("MSDA_DETERMINISTIC", "1")
    dec = _build("w42")
    prep = DI.prepare("w42", _dev(), ref_grad=False)
    params = [p for _, p in sorted(dec.named_parameters())]
    grad_leaves = [prep["leaves"][k] for k in ("tgt", "memory")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            DI.step(dec, prep)
    torch.cuda.current_stream().wait_stream(side)
    dec.zero_grad(set_to_none=True)
    for v in prep["leaves"].values():
        v.grad = None
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = DI.step(dec, prep)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for k in ("tgt", "memory"):
            v = prep["leaves"][k]
            v.copy_(torch.randn(v.shape, generator=g).to(_dev()))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.detach().clone() for o in outs] + [v.grad.clone() for v in grad_leaves] + [p.grad.clone() for p in params if p.grad is not None]
    dec.zero_grad(set_to_none=True)
    for v in prep["leaves"].values():
        v.grad = None
    eager = DI.step(dec, prep)
    eager = [o.detach() for o in eager] + [v.grad for v in grad_leaves] + [p.grad for p in params if p.grad is not None]
    assert len(replayed) == len(eager) and len(eager) > 50           # (the class heads get no gradient: argmax)
    for i, (a, b) in enumerate(zip(replayed, eager)):
        assert torch.equal(a, b), i


def test_masked_layer_reaches_the_long_attention_core(monkeypatch):
    from uvhand_amd import _native as MSDA
    calls = []
    real = MSDA.attn32x_forward
    monkeypatch.setattr(MSDA, "attn32x_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    dec = _build("w42")
    DI.run(dec, "w42", _dev())
    assert len(calls) == DI.CFG["layers"]
    calls.clear()
    DI.run(dec, "w42", _dev(), mask=False)                # without a mask the short core serves L = 15
    assert not calls


def test_zz_print_ratios():
    for k in sorted(RATIOS):
        print("worst ratio %-60s %.2f" % (k, RATIOS[k]))
