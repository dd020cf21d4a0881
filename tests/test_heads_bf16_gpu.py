"""The bf16-autocast form of the DETR prediction heads (csrc/msda_heads_bf16.hip, reached with MSDA_HEADS_BF16=1 under bf16
autocast): routes and dtypes, accuracy against an fp64 evaluation of the same heads, the forward's rounding points, bitwise
reproducibility, graph capture, and whole models.

Accuracy rule (the package's rule for a fused form against torch's own route, tests/test_optim_gpu.py): for every output and
every gradient the node's maximum absolute error against fp64 is at most 4 times the autocast composition's own error
against fp64 on the same inputs, where the composition's error counts as at least one bf16 ulp of the tensor's largest
magnitude (an exact composition result must not make the bound zero).  Each test prints the ratios it measured; on an
MI355X they were 0.09 to 1.00 for the outputs and 0.00 to 1.85 for the gradients over the cases below."""
import copy
import math
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import detr_inputs as DI  # noqa: E402
from uvhand_amd import _native  # noqa: E402
from uvhand_amd.functions import heads_func  # noqa: E402
from uvhand_amd.functions.heads_func import ARCTIC, ASSEMBLY, detr_heads, detr_heads_reference  # noqa: E402
from uvhand_amd.modules import ArcticDeformableDETR  # noqa: E402
from uvhand_amd.modules.detr import MLP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
FACTOR = 4.0


def _amp():
    return torch.autocast("cuda", dtype=BF)


def _heads(kind, L, B, Q, C, K, refine, n_mlp, R=42, seed=0):
    """Module lists as the models hold them (refine: one module per level, else one module repeated) and seeded inputs whose
    references include exactly 0 and 1 (inverse_sigmoid's clamps) and, for AssemblyHands' later levels, the values that
    (r + 0.5) / 2 maps onto them."""
    torch.manual_seed(seed)
    n = L if refine else 1
    cls = [torch.nn.Linear(C, K) for _ in range(n)]
    cls = torch.nn.ModuleList(cls if refine else cls * L).to(DEV)
    heads = []
    for _ in range(n_mlp):
        m = [MLP(C, C, 42 if kind == ARCTIC else 63, 3) for _ in range(n)]
        heads.append(torch.nn.ModuleList(m if refine else m * L).to(DEV))
    shared = [torch.nn.Linear(C, w).to(DEV) for w in _native.HEADS_SHARED_WIDTHS] if kind == ARCTIC else None
    hs = (torch.randn(L, B, Q, C, device=DEV) * 0.5).requires_grad_(True)
    init = torch.rand(B, Q, R, device=DEV) * 2.4 - 1.2
    inter = torch.rand(L, B, Q, R, device=DEV) * 2.4 - 1.2
    init[0, 0, 0], init[0, 0, 1], init[0, 1, 0], init[0, 1, 1] = 0.0, 1.0, 1.0, 0.0
    inter[:, 0, 0, 0], inter[:, 0, 0, 1], inter[:, 0, 1, 0], inter[:, 0, 1, 1] = 0.0, 1.0, -0.5, 1.5
    return hs, init, inter, cls, heads, shared


def _params(cls, heads, shared):
    seen, out = set(), []
    for m in [cls] + heads + (shared or []):
        for p in m.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                out.append(p)
    return out


def _run(kind, hs, init, inter, cls, heads, shared, fn=detr_heads, seed=3, amp=True):
    """Outputs and gradients (hs, then every parameter) for seeded output gradients that bf16 holds exactly."""
    if amp:
        with _amp():
            logits, keys, outs = fn(kind, hs, init, inter, cls, heads, shared)
    else:
        logits, keys, outs = fn(kind, hs, init, inter, cls, heads, shared)
    flat = [logits] + keys + outs
    g = torch.Generator(device=DEV).manual_seed(seed)
    loss = 0
    for t in flat:
        w = torch.randn(t.shape, device=DEV, generator=g).to(BF)
        loss = loss + (t * w.to(t.dtype)).sum()
    grads = torch.autograd.grad(loss, [hs] + _params(cls, heads, shared))
    return [t.detach() for t in flat], list(grads)


def _fp64(kind, hs, init, inter, cls, heads, shared):
    """The same heads evaluated in fp64 with no rounding."""
    cls64 = copy.deepcopy(cls).double()
    heads64 = [copy.deepcopy(h).double() for h in heads]
    if heads and heads[0][0] is heads[0][-1]:                           # deepcopy keeps the sharing inside one ModuleList
        assert heads64[0][0] is heads64[0][-1]
    shared64 = [copy.deepcopy(m).double() for m in shared] if shared is not None else None
    hs64 = hs.detach().double().requires_grad_(True)
    return _run(kind, hs64, init.double(), inter.double(), cls64, heads64, shared64, fn=detr_heads_reference, amp=False)


def _bf16_ulp(x):
    m = float(x.abs().max())
    return 2.0 ** (math.floor(math.log2(m)) - 7) if m > 0 else 2.0 ** -133


def _check_against_fp64(names, node, comp, ref):
    """The accuracy rule of the module docstring; returns the ratios node error / max(composition error, ulp)."""
    ratios = []
    for name, a, b, r in zip(names, node, comp, ref):
        assert a.shape == r.shape and a.dtype == b.dtype, name
        assert torch.isfinite(a.float()).all(), name
        e_node = float((a.double() - r).abs().max())
        e_comp = max(float((b.double() - r).abs().max()), _bf16_ulp(r))
        ratios.append((name, e_node / e_comp))
    print("node error / composition error against fp64: " + ", ".join("%s %.3f" % x for x in ratios))
    worst = max(ratios, key=lambda x: x[1])
    assert worst[1] <= FACTOR, "%s: %.3f times the composition's error" % worst
    return ratios


def _names(kind, n_mlp, n_param):
    outs = ["logits"] + ["kp%d" % i for i in range(n_mlp)] + (["shared%d" % i for i in range(6)] if kind == ARCTIC else [])
    return outs, ["grad_hs"] + ["grad_p%d" % i for i in range(n_param)]


# (kind, L, B, Q, C, K, per-level modules, n_mlp, R): M = B * Q in {40, 70, 128} (below a 64-row tile, a tile and a tail,
# exact tiles), C = 256, the smallest width the kernels take (8) and 40 (a full reduction stage and a partial one), and
# M * L = 2100 rows with shared modules: two weight-gradient chunks, the second a tail.
CASES = [
    (ARCTIC, 3, 2, 35, 256, 14, True, 2, 42),
    (ARCTIC, 1, 2, 20, 256, 4, False, 2, 42),
    (ARCTIC, 3, 2, 64, 8, 14, True, 2, 42),
    (ARCTIC, 3, 2, 35, 40, 4, False, 2, 42),
    (ARCTIC, 3, 2, 20, 256, 14, True, 0, 42),
    (ARCTIC, 1, 2, 64, 40, 14, True, 0, 42),
    (ARCTIC, 3, 2, 350, 40, 14, False, 2, 42),
    (ASSEMBLY, 3, 2, 35, 256, 14, True, 1, 2),
    (ASSEMBLY, 1, 2, 20, 256, 4, False, 1, 42),
    (ASSEMBLY, 3, 2, 64, 8, 14, True, 1, 42),
    (ASSEMBLY, 3, 2, 35, 40, 4, False, 1, 2),
    (ASSEMBLY, 1, 2, 64, 256, 14, True, 1, 2),
    (ASSEMBLY, 3, 2, 350, 40, 14, False, 1, 42),
]


def _id(case):
    return "%s-L%d-M%d-C%d-K%d-%s-mlp%d-R%d" % (case[0], case[1], case[2] * case[3], case[4], case[5],
                                                  "perlevel" if case[6] else "shared", case[7], case[8])


@pytest.fixture
def knob(monkeypatch):
    monkeypatch.setenv("MSDA_HEADS_BF16", "1")
    return monkeypatch


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_route_dtypes_and_accuracy_against_fp64(case, knob):
    """With the knob on under bf16 autocast the node runs (1..3 launches forward, 1..5 backward), returns the composition's
    dtypes, and meets the accuracy rule for every output and gradient."""
    kind, L, B, Q, C, K, refine, n_mlp, R = case
    args = _heads(kind, L, B, Q, C, K, refine, n_mlp, R)
    hs, init, inter, cls, heads, shared = args
    torch.cuda.synchronize()
    n0 = _native.launch_count()
    with _amp():
        logits, keys, outs = detr_heads(kind, *args)
    n1 = _native.launch_count()
    sum(t.float().sum() for t in [logits] + keys + outs).backward()
    n2 = _native.launch_count()
    assert 1 <= n1 - n0 <= 3 and 1 <= n2 - n1 <= 5, (n1 - n0, n2 - n1)
    hs.grad = None
    for p in _params(cls, heads, shared):
        p.grad = None

    node_out, node_grad = _run(kind, *args)
    knob.setenv("MSDA_HEADS_BF16", "0")
    n3 = _native.launch_count()
    comp_out, comp_grad = _run(kind, *args)
    assert _native.launch_count() == n3                                 # knob off: the composition, no library launch
    assert [t.dtype for t in node_out] == [t.dtype for t in comp_out]
    assert [t.shape for t in node_out] == [t.shape for t in comp_out]
    assert all(g.dtype == torch.float32 for g in node_grad)
    ref_out, ref_grad = _fp64(kind, *args)
    out_names, grad_names = _names(kind, n_mlp, len(node_grad) - 1)
    _check_against_fp64(out_names, node_out, comp_out, ref_out)
    _check_against_fp64(grad_names, node_grad, comp_grad, ref_grad)


def test_launch_budget_at_six_levels(knob):
    """All three depths forward and all five passes backward: exactly the fp32 form's budget."""
    for kind, n_mlp in ((ARCTIC, 2), (ASSEMBLY, 1)):
        args = _heads(kind, 6, 2, 50, 256, 14, True, n_mlp, 42)
        n0 = _native.launch_count()
        with _amp():
            logits, keys, outs = detr_heads(kind, *args)
        n1 = _native.launch_count()
        sum(t.float().sum() for t in [logits] + keys + outs).backward()
        assert (n1 - n0, _native.launch_count() - n1) == (3, 5)


def _launches(kind, args, dtype=BF):
    n0 = _native.launch_count()
    with torch.autocast("cuda", dtype=dtype):
        out = detr_heads(kind, *args)
    return out, _native.launch_count() - n0


@pytest.mark.parametrize("kind,n_mlp", [(ARCTIC, 2), (ASSEMBLY, 1)])
def test_composition_keeps_its_routes(kind, n_mlp, monkeypatch):
    hs, init, inter, cls, heads, shared = _heads(kind, 3, 2, 20, 256, 14, True, n_mlp, 42)
    args = (hs, init, inter, cls, heads, shared)
    monkeypatch.delenv("MSDA_HEADS_BF16", raising=False)
    (logits, keys, outs), n = _launches(kind, args)                     # knob unset under autocast
    assert n == 0
    with _amp():
        r_logits, r_keys, r_outs = detr_heads_reference(kind, *args)
    assert all(torch.equal(a, b) for a, b in zip([logits] + keys + outs, [r_logits] + r_keys + r_outs))
    monkeypatch.setenv("MSDA_HEADS_BF16", "1")
    assert _launches(kind, args)[1] > 0                                  # the knob alone switches the route
    assert _launches(kind, args, dtype=torch.float16)[1] == 0           # fp16 autocast
    assert _launches(kind, (hs.detach().to(BF), init, inter, cls, heads, shared))[1] == 0          # bf16 hs
    init_g = init.clone().requires_grad_(True)
    out, n = _launches(kind, (hs, init_g, inter, cls, heads, shared))   # a reference that requires grad
    assert n == 0
    out[1][0].float().sum().backward()
    assert init_g.grad is not None
    narrow = _heads(kind, 3, 2, 20, 36, 14, True, n_mlp, 42)            # C = 36: the fp32 kernels take it, these do not
    assert _native.heads_supported(36) and not _native.heads_bf16_supported(36)
    assert _launches(kind, narrow)[1] == 0
    # the knob on without autocast: the fp32 node as before
    n0 = _native.launch_count()
    logits32, _, _ = detr_heads(kind, *args)
    assert _native.launch_count() - n0 == 3 and logits32.dtype == torch.float32


def _direct_forward(kind, args):
    """The C entry's own results (hidden and sig included) for the operands detr_heads would pass."""
    hs, init, inter, cls, heads, shared = args
    with _amp():
        meta, params = heads_func._fused_plan(kind, hs, init, inter, cls, list(heads), shared)
    k, flags, n_cls, n_mlp, n_sh, bf16 = meta
    assert bf16
    L, B, Q, C = hs.shape
    groups = heads_func._split([p.detach() for p in params], n_cls, n_mlp, n_sh)
    return _native.heads_forward_bf16(k, hs.detach().view(L, B * Q, C), init.contiguous(),
                                      inter[:L - 1].contiguous() if L > 1 else None, *groups, flags)


def test_rounding_points_arctic(knob):
    """Logits are bf16 values held in fp32; keypoints are the fp32 epilogue of the saved fp32 sigmoid."""
    args = _heads(ARCTIC, 3, 2, 35, 256, 14, True, 2, 42)
    with _amp():
        logits, keys, outs = detr_heads(ARCTIC, *args)
    assert logits.dtype == torch.float32 and torch.equal(logits, logits.to(BF).float())
    d_logits, d_kp, d_sh, hidden, sig = _direct_forward(ARCTIC, args)
    assert torch.equal(d_logits.view_as(logits), logits)
    assert hidden.dtype == BF and sig.dtype == torch.float32 and (hidden >= 0).all()
    for h in range(2):
        assert torch.equal(d_kp[h], sig[h] * 2 - 1)
    assert all(o.dtype == BF for o in outs) and all(k.dtype == torch.float32 for k in keys)


@pytest.mark.parametrize("R", [2, 42])
def test_rounding_points_assembly(R, knob):
    """Keypoints lie on the grid of bf16 `sigmoid * 2 - 0.5`: recomputed in torch's bf16 arithmetic from the node's saved
    fp32 sigmoid they are equal bit for bit."""
    args = _heads(ASSEMBLY, 3, 2, 35, 256, 14, True, 1, R)
    with _amp():
        logits, keys, _ = detr_heads(ASSEMBLY, *args)
    assert logits.dtype == BF and keys[0].dtype == BF
    d_logits, d_kp, _, hidden, sig = _direct_forward(ASSEMBLY, args)
    assert torch.equal(d_kp[0].view_as(keys[0]), keys[0])
    assert torch.equal(d_kp[0], sig[0].to(BF) * 2 - 0.5)
    assert (d_kp[0] * 2 - 0.5).dtype == BF


@pytest.mark.parametrize("kind,n_mlp", [(ARCTIC, 2), (ASSEMBLY, 1)])
def test_bitwise_reproducible(kind, n_mlp, knob):
    args = _heads(kind, 3, 2, 45, 256, 14, True, n_mlp, 42)
    a_out, a_grad = _run(kind, *args)
    b_out, b_grad = _run(kind, *args)
    assert all(torch.equal(x, y) for x, y in zip(a_out + a_grad, b_out + b_grad))


@pytest.mark.parametrize("kind,n_mlp", [(ARCTIC, 2), (ASSEMBLY, 1)])
def test_graph_capture_matches_eager(kind, n_mlp, knob):
    hs, init, inter, cls, heads, shared = _heads(kind, 3, 2, 33, 256, 14, True, n_mlp, 42)
    params = _params(cls, heads, shared)
    D = 42 if kind == ARCTIC else 63
    weights = [torch.randn(s, device=DEV) for s in [(3, 2, 33, 14)] + [(3, 2, 33, D)] * n_mlp]

    def step():
        with _amp():
            logits, keys, outs = detr_heads(kind, hs, init, inter, cls, heads, shared)
        loss = sum((t * w).sum() for t, w in zip([logits] + keys, weights)) + sum(o.float().sum() for o in outs)
        return [logits] + keys + list(torch.autograd.grad(loss, [hs] + params))

    n0 = _native.launch_count()
    eager = [t.detach().clone() for t in step()]
    assert _native.launch_count() - n0 == 8
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


def _package_model():
    """test_detr_gpu.py's small ARCTIC whole-model configuration."""
    from uvhand_amd.modules import DeformableTransformer
    torch.manual_seed(0)
    Q = 20
    tr = DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=2, dim_feedforward=512,
                               dropout=0.0, return_intermediate_dec=True, num_feature_levels=2, two_stage=True,
                               two_stage_num_proposals=Q)
    model = ArcticDeformableDETR([None, DI.StubPosition()], tr, 14, Q, 2, with_box_refine=True, two_stage=True)
    g = torch.Generator().manual_seed(9)
    samples = [torch.randn(1, 2, 256, 8, 8, generator=g).to(DEV), torch.randn(1, 2, 256, 4, 4, generator=g).to(DEV)]
    return model.to(DEV).eval(), samples


def test_whole_model_under_autocast(monkeypatch):
    """ArcticDeformableDETR under autocast with the knob on and off: the same keys and dtypes, and the knob-on values within
    the accuracy rule of an fp64 evaluation of the heads over the transformer's own (fp32) results.  (AssemblyHands'
    two-stage query selection does not run under autocast, in the reference either: an index_put of bf16 scores into an fp32
    tensor.)"""
    model, samples = _package_model()
    seen = []
    hook = model.transformer.register_forward_hook(lambda mod, inp, out: seen.append(out))
    results = []
    with torch.no_grad():
        for on in ("1", "0"):
            monkeypatch.setenv("MSDA_HEADS_BF16", on)
            with _amp():
                out = model(samples)
            results.append(DI.flatten_outputs(out))
    hook.remove()
    tr_on, tr_off = seen
    assert tr_on[0].dtype == torch.float32                              # hs: the fp32 residual stream
    assert all(torch.equal(a, b) for a, b in zip(tr_on, tr_off))        # the two runs fed the heads the same tensors
    # the node ran in the first pass: the heads alone, on those tensors
    monkeypatch.setenv("MSDA_HEADS_BF16", "1")
    n0 = _native.launch_count()
    with torch.no_grad(), _amp():
        again = DI.flatten_outputs(model.heads(*tr_on))
    assert 1 <= _native.launch_count() - n0 <= 3
    on, off = results
    assert [k for k, _ in on] == [k for k, _ in off]
    assert [t.dtype for _, t in on] == [t.dtype for _, t in off]
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(on, again))
    twin = copy.deepcopy(model).double()
    with torch.no_grad():
        ref = DI.flatten_outputs(twin.heads(*[t.double() for t in tr_on]))
    assert [k for k, _ in ref] == [k for k, _ in on]
    _check_against_fp64([k for k, _ in on], [t for _, t in on], [t for _, t in off], [t for _, t in ref])
