"""The DINO DeformableTransformer (uvhand_amd.modules.DinoDeformableTransformer) on the GPU at the fixture's shape
(tests/golden/dino_transformer_inputs.py): the fused drop-in against the fixture and held to the project's accuracy rule against
an fp64 copy of the module; a pyramid beyond the 8192 rows the older selection kernel sorts; the step under
torch.cuda.set_sync_debug_mode("error") — where the reference's structure, with its boolean-mask assignments, raises —; the
step captured in one graph; the MSDA_DINO_FUSED knob."""
import copy
import gc
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_transformer_inputs as TI  # noqa: E402

pytestmark = pytest.mark.gpu

RATIOS = {}


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "dino_transformer.npz"))


def _build(case, cfg=TI.CFG, seed=None):
    from uvhand_amd.modules import DinoDeformableTransformer
    from uvhand_amd.modules.detr import MLP
    return TI.build(DinoDeformableTransformer, MLP, case, cfg, seed).to(_dev())


def _spy(monkeypatch):
    from uvhand_amd import _native as MSDA
    calls = []
    real = MSDA.dino_select_forward
    monkeypatch.setattr(MSDA, "dino_select_forward", lambda *a, **k: (calls.append(a[0].shape[1]), real(*a, **k))[1])
    return calls


def _results(tr, prep, outs, cfg=TI.CFG):
    params = sorted(tr.named_parameters())
    names = TI.labels(cfg) + ["grad_src%d" % i for i in range(len(prep["srcs"]))] + ["pgrad " + k for k, _ in params]
    return names, [o.detach() for o in outs] + [s.grad for s in prep["srcs"]] + [p.grad for _, p in params]


@pytest.mark.parametrize("case", list(TI.CASES))
def test_fused_drop_in_reproduces_the_fixture(case, fixture, monkeypatch):
    calls = _spy(monkeypatch)
    tr = _build(case)
    report = TI.compare(tr, case, fixture, _dev())
    assert calls == [TI.n_rows()], "the selection kernels did not serve the call"
    assert np.array_equal(tr.last_topk_proposals.cpu().numpy(), fixture[case + "/topk"])
    for r in report:
        print("%-64s %.3e (bar %.0e)" % r)
    bad = [r for r in report if not r[1] <= r[2]]
    assert not bad, "beyond the bars: " + "; ".join("%s %.3e > %.0e" % r for r in bad[:12])


@pytest.mark.parametrize("case", list(TI.CASES))
def test_fused_drop_in_holds_the_ratio_rule(case, monkeypatch):
    """ours: the drop-in as shipped.  The yardstick: the reference's structure (MSDA_DINO_FUSED=0: heads on every row, gathers,
    mask assignments, and the decoder's compositions) in fp32 on the GPU.  Both against the same structure in fp64."""
    from uvhand_amd.functions import dino_func as DF
    tr = _build(case)
    prep = TI.prepare(case, _dev())
    names, ours = _results(tr, prep, TI.step(tr, prep))
    topk = tr.last_topk_proposals.clone()
    monkeypatch.setattr(DF, "FUSED", False)
    got = []
    for dt in (torch.float32, torch.float64):
        t2 = copy.deepcopy(tr).to(dt)
        t2.zero_grad(set_to_none=True)
        p2 = TI.prepare(case, _dev(), dt)
        got.append(_results(t2, p2, TI.step(t2, p2))[1])
        assert torch.equal(t2.last_topk_proposals, topk), dt
    for name, a, b, c in zip(names, ours, got[0], got[1]):
        assert (a is None) == (c is None) == (b is None), name
        if a is not None:
            TI.hold("%s %s" % (case, name), a, b, c, RATIOS)


def test_pyramid_beyond_the_older_kernels_limit(monkeypatch):
    """S = 8193 + 64 rows per frame, Q = 900: the kernels serve the whole class where msda_two_stage_select_f32 cannot.  The
    selected rows are the rule's on the very logits the kernels read.  At this size the pyramid's outermost rows lie outside
    (0.01, 0.99): they are zeroed, share one set of logits and carry +inf proposals, so the reference's ``torch.topk`` promises no
    order among them; the yardstick is therefore ``dino_select_composition`` (a stable sort: the same rule) with the heads after
    the selection, on the same module — the same rows exactly, the rest within the module fixtures' bars (MSDA_DINO_FUSED=0 also
    moves the decoder's query positions and refinement to their torch compositions)."""
    from uvhand_amd.functions import dino_func as DF
    calls = _spy(monkeypatch)
    logits = []
    real = DF.select_queries_dino
    monkeypatch.setattr(DF, "select_queries_dino", lambda c, *a, **k: (logits.append(c.detach().clone()), real(c, *a, **k))[1])
    cfg = TI.BIG
    tr = _build(None, cfg, cfg["seed"])
    prep = TI.prepare(None, _dev(), cfg=cfg)
    names, ours = _results(tr, prep, TI.step(tr, prep), cfg)
    assert calls == [8193 + 64]
    topk = tr.last_topk_proposals.clone()
    want = TI.numpy_select_rule(logits[0].cpu().numpy(), 900)[0]
    assert np.array_equal(topk.cpu().numpy(), want)
    tr.zero_grad(set_to_none=True)
    for s in prep["srcs"]:
        s.grad = None
    monkeypatch.setattr(DF, "FUSED", False)
    tr.two_stage_route = "selected"
    _, ref = _results(tr, prep, TI.step(tr, prep), cfg)
    assert len(calls) == 1, "the yardstick ran on the kernels"
    assert torch.equal(tr.last_topk_proposals, topk)
    for name in ("hs_enc", "init_box_proposal_unsig"):
        assert torch.equal(ours[names.index(name)], ref[names.index(name)]), name
    for name, a, b in zip(names, ours, ref):
        assert (a is None) == (b is None), name
        if a is None:
            continue
        bar = TI.ACT_BAR if name in TI.labels(cfg) else TI.GRAD_BAR
        finite = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), finite), name
        err = float((a[finite] - b[finite]).abs().max() / b[finite].abs().max().clamp_min(1e-30)) if finite.any() else 0.0
        print("%-48s %.3e (bar %.0e)" % (name, err, bar))
        assert err <= bar, (name, err)


def test_step_makes_no_host_sync_and_the_reference_structure_does():
    tr = _build("embed_dn")
    prep = TI.prepare("embed_dn", _dev())
    TI.step(tr, prep)                                   # warm-up: the level tensors, MSDeformAttn's check of them, allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = TI.step(tr, prep)                        # forward + backward: nothing may synchronise
        tr.two_stage_route = "reference"
        with pytest.raises(RuntimeError):
            TI.step(tr, prep)                           # the reference's boolean-mask assignments: a nonzero each
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(o).all() for o in outs)


def test_step_replays_from_one_graph(monkeypatch):
    """Forward plus backward captured once and replayed on new srcs equals the eager result bit for bit (the fixture has dropout
    0; the sampling's backward takes its deterministic kernels so that two runs can be compared at all)."""
    monkeypatch.setenv("MSDA_DETERMINISTIC", "1")
    tr = _build("embed_dn")
    prep = TI.prepare("embed_dn", _dev())
    params = [p for _, p in sorted(tr.named_parameters())]

    def clear():
        tr.zero_grad(set_to_none=True)
        for s in prep["srcs"]:
            s.grad = None

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            TI.step(tr, prep)
    torch.cuda.current_stream().wait_stream(side)
    clear()
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = TI.step(tr, prep)
    g = torch.Generator().manual_seed(78)
    with torch.no_grad():
        for s in prep["srcs"]:
            s.copy_(torch.randn(s.shape, generator=g).to(_dev()))
    graph.replay()
    torch.cuda.synchronize()
    replayed = ([o.detach().clone() for o in outs] + [s.grad.clone() for s in prep["srcs"]]
                + [p.grad.clone() for p in params if p.grad is not None] + [tr.last_topk_proposals.clone()])
    clear()
    eager = TI.step(tr, prep)
    eager = ([o.detach() for o in eager] + [s.grad for s in prep["srcs"]] + [p.grad for p in params if p.grad is not None]
             + [tr.last_topk_proposals])
    assert len(replayed) == len(eager) and len(eager) > 60
    for i, (a, b) in enumerate(zip(replayed, eager)):
        assert torch.equal(a, b), i


def test_knob_selects_the_reference_structure(monkeypatch):
    from uvhand_amd.functions import dino_func as DF
    calls = _spy(monkeypatch)
    tr = _build("embed")
    prep = TI.prepare("embed", _dev())
    TI.step(tr, prep, backward=False)
    assert len(calls) == 1
    monkeypatch.setattr(DF, "FUSED", False)
    ran = []
    monkeypatch.setattr(tr, "_select_reference", lambda *a: (ran.append(1), type(tr)._select_reference(tr, *a))[1])
    TI.step(tr, prep, backward=False)
    assert len(calls) == 1 and ran == [1]


def test_hooked_head_selects_the_reference_structure(monkeypatch):
    calls = _spy(monkeypatch)
    tr = _build("embed")
    prep = TI.prepare("embed", _dev())
    seen = []
    h = tr.enc_out_key_embed.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].shape[1]))
    TI.step(tr, prep, backward=False)
    h.remove()
    assert not calls and seen == [TI.n_rows()], "a hook on a head must see every encoder row, as in the reference"


def test_zz_print_ratios():
    for k in sorted(RATIOS):
        print("worst ratio %-60s %.2f" % (k, RATIOS[k]))
