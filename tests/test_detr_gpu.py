"""The DETR prediction heads on the GPU (csrc/msda_heads.hip through functions/heads_func.py and modules/detr.py): fixtures
of the reference's DeformableDETR (gen_golden_r10.py), the torch restatement, launch counts, no host sync, bitwise
reproducibility, graph capture, the composition's routes, and whole models over the package's transformer."""
import copy
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import detr_inputs as DI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions.heads_func import ARCTIC, ASSEMBLY, detr_heads, detr_heads_reference  # noqa: E402
from uvhand_amd.modules import ArcticDeformableDETR, AssemblyDeformableDETR  # noqa: E402
from uvhand_amd.modules.detr import MLP, NestedTensor  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ACT, GRAD = 2e-5, 1e-4           # fp32 MFMA against the CPU: as tests/test_linear_gpu.py


def _cls(name):
    return ArcticDeformableDETR if DI.CASES[name][0] == "arctic" else AssemblyDeformableDETR


def _gpu_model(name, seed):
    model = DI.build(name, _cls(name), NestedTensor)
    DI.perturb(model, seed)
    tr = model.transformer
    model.to(DEV)
    tr.hs = tr.hs.detach().to(DEV).requires_grad_(True)
    tr.init_reference = tr.init_reference.to(DEV)
    tr.inter_references = tr.inter_references.to(DEV)
    tr.enc = tuple(t.to(DEV) for t in tr.enc)
    return model


def _samples(name):
    s = DI.samples(name, NestedTensor)
    return [t.to(DEV) for t in s] if isinstance(s, list) else NestedTensor(s.tensors.to(DEV), s.mask.to(DEV))


@pytest.mark.parametrize("name", list(DI.CASES))
def test_fixture_outputs_and_gradients(name):
    z = load_golden("detr_" + name)
    seed = DI.CASES[name][-1]
    model = _gpu_model(name, seed)
    model.train()
    out = model(_samples(name))
    for path, t in DI.flatten_outputs(out):
        assert rel_err(t.detach().cpu().numpy(), z["out" + path]) < ACT, path
    DI.weighted_sum(out, seed + 7).backward()
    assert rel_err(model.transformer.hs.grad.cpu().numpy(), z["grad/hs"]) < GRAD
    for k, p in model.named_parameters():
        if "grad/" + k in z:
            assert rel_err(p.grad.cpu().numpy(), z["grad/" + k]) < GRAD, k
        elif "gradsum0/" + k in z:
            assert rel_err(p.grad.sum(0).cpu().numpy(), z["gradsum0/" + k]) < GRAD, k
            assert rel_err(p.grad.sum(1).cpu().numpy(), z["gradsum1/" + k]) < GRAD, k
        else:
            assert p.grad is None, k


def _heads(kind, L, B, Q, refine, R=42, K=14, seed=0):
    """Module lists as the models hold them and seeded inputs, on the GPU."""
    torch.manual_seed(seed)
    C = 256
    n = L if refine else 1
    cls = [torch.nn.Linear(C, K) for _ in range(n)]
    cls = torch.nn.ModuleList(cls if refine else cls * L).to(DEV)
    heads = []
    for _ in range(2 if kind == ARCTIC else 1):
        m = [MLP(C, C, 42 if kind == ARCTIC else 63, 3) for _ in range(n)]
        heads.append(torch.nn.ModuleList(m if refine else m * L).to(DEV))
    shared = [torch.nn.Linear(C, w).to(DEV) for w in _native.HEADS_SHARED_WIDTHS] if kind == ARCTIC else None
    hs = (torch.randn(L, B, Q, C, device=DEV) * 0.5).requires_grad_(True)
    init = torch.rand(B, Q, R, device=DEV) * 2.4 - 1.2
    inter = torch.rand(L, B, Q, R, device=DEV) * 2.4 - 1.2
    return hs, init, inter, cls, heads, shared


def _run(kind, hs, init, inter, cls, heads, shared, fn=detr_heads, seed=3):
    logits, keys, outs = fn(kind, hs, init, inter, cls, heads, shared)
    flat = [logits] + keys + outs
    g = torch.Generator(device=DEV).manual_seed(seed)
    loss = sum((t * torch.randn(t.shape, device=DEV, generator=g)).sum() for t in flat)
    params = [p for m in [cls] + heads + (shared or []) for p in m.parameters()]
    grads = torch.autograd.grad(loss, [hs] + params)
    return [t.detach() for t in flat], list(grads)


CONFIGS = [(ARCTIC, True, 42), (ASSEMBLY, True, 2), (ASSEMBLY, False, 42), (ASSEMBLY, True, 42)]


@pytest.mark.parametrize("kind,refine,R", CONFIGS)
def test_matches_restatement(kind, refine, R):
    args = _heads(kind, 6, 3, 37, refine, R=R)                         # B * Q = 111: edge tiles
    a_out, a_grad = _run(kind, *args)
    b_out, b_grad = _run(kind, *args, fn=detr_heads_reference)
    for x, y in zip(a_out, b_out):
        assert rel_err(x.cpu().numpy(), y.cpu().numpy()) < ACT
    for x, y in zip(a_grad, b_grad):
        assert rel_err(x.cpu().numpy(), y.cpu().numpy()) < GRAD


@pytest.mark.parametrize("L", [1, 6])
@pytest.mark.parametrize("kind", [ARCTIC, ASSEMBLY])
def test_launch_counts(kind, L):
    hs, init, inter, cls, heads, shared = _heads(kind, L, 2, 50, True, R=42)
    torch.cuda.synchronize()
    n0 = _native.launch_count()
    logits, keys, outs = detr_heads(kind, hs, init, inter, cls, heads, shared)
    n1 = _native.launch_count()
    loss = sum(t.sum() for t in [logits] + keys + outs)
    loss.backward()
    n2 = _native.launch_count()
    assert n1 - n0 == 3 and n2 - n1 == 5


def test_no_host_sync():
    args = _heads(ARCTIC, 6, 2, 40, True)
    _run(ARCTIC, *args)                                                 # warm up allocator and code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        hs, init, inter, cls, heads, shared = args
        logits, keys, outs = detr_heads(ARCTIC, hs, init, inter, cls, heads, shared)
        sum(t.sum() for t in [logits] + keys + outs).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.parametrize("kind", [ARCTIC, ASSEMBLY])
def test_bitwise_reproducible(kind):
    args = _heads(kind, 6, 2, 45, True)
    a_out, a_grad = _run(kind, *args)
    b_out, b_grad = _run(kind, *args)
    assert all(torch.equal(x, y) for x, y in zip(a_out + a_grad, b_out + b_grad))


def test_graph_capture_matches_eager():
    hs, init, inter, cls, heads, shared = _heads(ARCTIC, 6, 2, 33, True)
    params = [p for m in [cls] + heads + shared for p in m.parameters()]
    weights = [torch.randn(s, device=DEV) for s in [(6, 2, 33, 14), (6, 2, 33, 42), (6, 2, 33, 42)]]

    def step():
        logits, keys, outs = detr_heads(ARCTIC, hs, init, inter, cls, heads, shared)
        loss = sum((t * w).sum() for t, w in zip([logits] + keys, weights)) + sum(o.sum() for o in outs)
        return [logits] + keys + list(torch.autograd.grad(loss, [hs] + params))

    eager = [t.detach().clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, static))


def _composition_launches(kind, args, monkeypatch=None, autocast=False):
    n0 = _native.launch_count()
    if autocast:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = detr_heads(kind, *args)
    else:
        out = detr_heads(kind, *args)
    return out, _native.launch_count() - n0


def test_composition_routes(monkeypatch):
    hs, init, inter, cls, heads, shared = _heads(ARCTIC, 3, 2, 20, True)
    args = (hs, init, inter, cls, heads, shared)
    ref_out, ref_grad = _run(ARCTIC, *args, fn=detr_heads_reference)
    monkeypatch.setenv("MSDA_HEADS_FUSED", "0")
    out, n = _composition_launches(ARCTIC, args)
    assert n == 0
    got_out, got_grad = _run(ARCTIC, *args)
    assert all(torch.equal(x, y) for x, y in zip(ref_out + ref_grad, got_out + got_grad))
    monkeypatch.setenv("MSDA_HEADS_FUSED", "1")
    # references that require grad take the composition (and get their gradient)
    init_g = init.clone().requires_grad_(True)
    out, n = _composition_launches(ARCTIC, (hs, init_g, inter, cls, heads, shared))
    assert n == 0
    out[1][0].sum().backward()
    assert init_g.grad is not None
    # bf16 autocast: the reference under --amp (logits in fp32, the shared Linears bf16)
    (logits, keys, outs), n = _composition_launches(ARCTIC, args, autocast=True)
    assert n == 0 and logits.dtype == torch.float32 and outs[0].dtype == torch.bfloat16
    with torch.autocast("cuda", dtype=torch.bfloat16):
        r_logits, r_keys, _ = detr_heads_reference(ARCTIC, *args)
    assert torch.equal(logits, r_logits) and keys[0].dtype == r_keys[0].dtype and torch.equal(keys[0], r_keys[0])


def _package_model(kind):
    from uvhand_amd.modules import AssemblyDeformableTransformer, DeformableTransformer
    torch.manual_seed(0)
    Q = 20 if kind == ARCTIC else 3            # AssemblyHands' two-stage selection keeps (left, right, object)
    if kind == ARCTIC:
        tr = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=2, dim_feedforward=512,
                                   dropout=0.0, return_intermediate_dec=True, num_feature_levels=2, two_stage=True,
                                   two_stage_num_proposals=Q)
        model = ArcticDeformableDETR([None, DI.StubPosition()], tr, 14, Q, 2, with_box_refine=True, two_stage=True)
        g = torch.Generator().manual_seed(9)
        samples = [torch.randn(1, 2, 256, 8, 8, generator=g).to(DEV), torch.randn(1, 2, 256, 4, 4, generator=g).to(DEV)]
    else:
        tr = AssemblyDeformableTransformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=2,
                                           dim_feedforward=512, dropout=0.0, return_intermediate_dec=True,
                                           num_feature_levels=2, two_stage=True, two_stage_num_proposals=Q)
        model = AssemblyDeformableDETR(DI.StubBackbone(NestedTensor), tr, 14, Q, 2, with_box_refine=True, two_stage=True,
                                       cfg=DI.Cfg())
        g = torch.Generator().manual_seed(9)
        samples = NestedTensor(torch.randn(2, 3, 32, 32, generator=g).to(DEV), torch.zeros(2, 32, 32, dtype=torch.bool,
                                                                                             device=DEV))
    return model.to(DEV).eval(), samples


@pytest.mark.parametrize("kind", [ARCTIC, ASSEMBLY])
def test_whole_model_matches_composition(kind, monkeypatch):
    model, samples = _package_model(kind)
    twin = copy.deepcopy(model)
    results = []
    for m, fused in ((model, "1"), (twin, "0")):
        monkeypatch.setenv("MSDA_HEADS_FUSED", fused)
        out = m(samples)
        flat = DI.flatten_outputs(out)
        DI.weighted_sum(out, 11).backward()
        results.append(([t.detach().cpu().numpy() for _, t in flat],
                        {k: p.grad.cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}))
    (a_out, a_grad), (b_out, b_grad) = results
    for x, y in zip(a_out, b_out):
        assert rel_err(x, y) < 1e-4
    assert set(a_grad) == set(b_grad)
    for k in a_grad:
        assert rel_err(a_grad[k], b_grad[k]) < 1e-3, k
    assert np.isfinite(np.concatenate([v.ravel() for v in a_grad.values()])).all()
