"""C ABI of the Swin glue kernels over a bf16 residual stream (msda_swin_glue_*_<T>_sbf16, additive at ABI 116), the route's
host-side decisions (MSDA_SWIN_GLUE_BF16 next to MSDA_SWIN_GLUE) and the rounding contract of include/msda.h restated in torch.
No GPU: every C call here fails its host-side checks, which come before any launch, so fake device addresses never reach a
kernel; the autograd functions are run on CPU tensors, where they are the torch expressions."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_swin_glue_abi import BAD_WIDTHS, C, MERGE, OK_PTR, ROWS, RPS, _ARGS, _SCALARS, _autocast, _formula, _refused

BF16 = torch.bfloat16
# (operation, T): the ten entries
ENTRIES = [(op + "_" + d, t) for op, ts in (("norm", ("f32", "bf16")), ("add_norm", ("bf16",)), ("add", ("bf16",)),
                                            ("merge_norm", ("bf16",))) for d in ("forward", "backward") for t in ts]
_STREAM = ("x", "y", "grad_x", "grad_y")                 # rows of the bf16 stream: 8-byte alignment
_TYPED = ("a", "z", "grad_z", "grad_a")                  # rows of T: 8-byte alignment for bf16, 16 for fp32
_F32 = ("gamma", "beta", "workspace")


def _name(op, t):
    return "msda_swin_glue_%s_%s_sbf16" % (op, t)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    handle = _native.declare(ctypes.CDLL(_native.LIB_PATH))
    yield handle
    # leave no error text behind for later tests in this process: an empty problem passes every check and launches nothing
    fn = handle.msda_add_layernorm_forward_f32_bf16res
    assert fn(None, None, None, None, 0, 256, 1e-5, None, None, None, None) == 0
    assert handle.msda_last_error() == b""


def test_library_exports_the_stream_entries_at_abi_116(lib):
    """Fails without the bf16-stream entries."""
    from uvhand_amd import _native
    assert len(ENTRIES) == 10
    for op, t in ENTRIES:
        assert hasattr(lib, _name(op, t)) and _name(op, t) in _native.SIGNATURES, (op, t)
    assert lib.msda_version() == 116


def _call(lib, op, t, **over):
    names = _ARGS[op].split()
    merge = op.startswith("merge")
    width = over.get("C", C)
    rows = MERGE["B"] * 2 * 3 if merge else over.get("rows", ROWS)
    vals = dict(rows=ROWS, rps=RPS, C=C, eps=1e-5, **MERGE)
    vals["wbytes"] = lib.msda_swin_glue_workspace_bytes(rows, 4 * width if merge else width)
    for n in names:
        if n not in _SCALARS:
            vals[n] = OK_PTR
    vals.update(over)
    return getattr(lib, _name(op, t))(*[vals[n] for n in names], None)


@pytest.mark.parametrize("op,t", ENTRIES, ids=["%s_%s" % e for e in ENTRIES])
def test_argument_errors_come_before_any_launch(lib, op, t):
    names = _ARGS[op].split()
    merge = op.startswith("merge")
    for width in BAD_WIDTHS + ((772,) if merge else ()):                        # 4 * 772 > 3072
        assert b"C % 4 == 0" in _refused(lib, _call(lib, op, t, C=width)), width
    if "rps" in names:
        for bad in (0, -3):
            assert b"rows_per_sample" in _refused(lib, _call(lib, op, t, rps=bad))
    if "rows" in names:
        assert b"rows" in _refused(lib, _call(lib, op, t, rows=-1))
    else:
        assert b"H, W > 0" in _refused(lib, _call(lib, op, t, H=0))
    # keep is optional except for add's backward, which has nothing to compute without one; add_norm's grad_a is optional
    # only without keep (it is grad_x then)
    optional = ({"keep"} if op != "add_backward" else set()) | ({"grad_a"} if op == "add_norm_backward" else set())
    for n in names:
        if n in _SCALARS or n in optional:
            continue
        msg = _refused(lib, _call(lib, op, t, **{n: None}))
        assert b"null" in msg and _name(op, t).encode() in msg, n
    if op == "add_norm_backward":
        assert b"null" in _refused(lib, _call(lib, op, t, grad_a=None))         # keep given: grad_a is its own tensor
    for n in names:
        if n in _STREAM or (n in _TYPED and t == "bf16"):
            offs = (2, 4)
        elif n in _TYPED or n in _F32:
            offs = (4, 8)
        elif n == "keep":
            offs = (1,)
        elif n in ("mean", "rstd", "grad_gamma", "grad_beta"):
            offs = (2,)
        else:
            continue
        for off in offs:
            assert b"aligned" in _refused(lib, _call(lib, op, t, **{n: OK_PTR + off})), (n, off)
    if "workspace" in names:
        full = lib.msda_swin_glue_workspace_bytes(MERGE["B"] * 6 if merge else ROWS, 4 * C if merge else C)
        assert full == _formula(MERGE["B"] * 6 if merge else ROWS, 4 * C if merge else C)
        for short in (full - 1, 0):
            assert b"workspace smaller" in _refused(lib, _call(lib, op, t, wbytes=short))


@pytest.mark.filterwarnings("ignore:.*CUDA is not available.*")
def test_route_decisions_without_a_gpu(monkeypatch):
    """Fails without the second knob: bf16 rows never take the glue there."""
    from uvhand_amd.functions.swin_glue_func import glue_route
    cuda, cpu = torch.device("cuda"), torch.device("cpu")

    def knobs(glue, stream):
        for key, value in (("MSDA_SWIN_GLUE", glue), ("MSDA_SWIN_GLUE_BF16", stream)):
            if value is None:
                monkeypatch.delenv(key, raising=False)
            else:
                monkeypatch.setenv(key, value)
    for glue in (None, "0", "", "1"):
        for stream in (None, "0", "", "1"):
            knobs(glue, stream)
            both = glue == "1" and stream == "1"
            assert not glue_route(cuda, BF16, 96)                               # bf16 rows outside autocast: torch
            with _autocast(BF16):
                assert torch.is_autocast_enabled()
                assert glue_route(cuda, BF16, 96) == both, (glue, stream)
                assert not glue_route(cpu, BF16, 96)
                for width in (98, 3076, 0):
                    assert not glue_route(cuda, BF16, width)
                assert glue_route(cuda, BF16, 3072) == both
                # fp32 rows do not depend on the new knob
                assert glue_route(cuda, torch.float32, 96) == (glue == "1")
                assert not glue_route(cuda, torch.float16, 96) and not glue_route(cuda, torch.float64, 96)
            with _autocast(torch.float16):
                assert not glue_route(cuda, BF16, 96) and not glue_route(cuda, torch.float32, 96)
            assert glue_route(cuda, torch.float32, 96) == (glue == "1")
    # the new knob alone switches nothing on; the other two Swin knobs switch nothing here
    knobs("1", "1")
    monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
    monkeypatch.setenv("MSDA_SWIN_BF16", "0")
    with _autocast(BF16):
        assert glue_route(cuda, BF16, 96)
    knobs(None, "1")
    with _autocast(BF16):
        assert not glue_route(cuda, BF16, 96) and not glue_route(cuda, torch.float32, 96)


def _leaves(*tensors):
    return [t.detach().clone().requires_grad_(True) for t in tensors]


def _case(B=3, L=5, width=96, seed=3):
    """bf16 x, a, grad_y, grad_z, fp32 LayerNorm, keep = bf16(1 / 0.7) with one zero."""
    g = torch.Generator().manual_seed(seed)
    x, a, gy, gz = ((torch.randn(B, L, width, generator=g) * 1.5 + 0.3).to(BF16) for _ in range(4))
    norm = nn.LayerNorm(width)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(width, generator=g) * 0.5 + 1)
        norm.bias.copy_(torch.randn(width, generator=g) * 0.5)
    keep = torch.full((B, 1, 1), 1 / 0.7).to(BF16)
    keep[1] = 0
    return x, a, gy, gz, norm, keep


def _autocast_composition(x, a, keep, norm, gy, gz):
    """What the block runs under CUDA bf16 autocast on a bf16 stream, written out: bf16 product and add, F.layer_norm on the
    float32 cast (autocast's fp32 list), and the bf16 cast the Linear that consumes z applies."""
    x, a = _leaves(x, a)
    y = x + (a if keep is None else a * keep)
    z = F.layer_norm(y.float(), norm.normalized_shape, norm.weight, norm.bias, norm.eps).to(BF16)
    torch.autograd.backward([y, z], [gy, gz])
    return y.detach(), z.detach(), x.grad, a.grad


def _contract(x, a, keep, norm, gy, gz):
    """include/msda.h's table in fp32 operations and rnd."""
    def rnd(t):
        return t.to(BF16)
    with torch.no_grad():
        branch = a.float() if keep is None else rnd(a.float() * keep.float()).float()
        y = rnd(x.float() + branch)
    yf = y.float().requires_grad_(True)
    z32 = F.layer_norm(yf, norm.normalized_shape, norm.weight.detach(), norm.bias.detach(), norm.eps)
    z32.backward(gz.float())
    with torch.no_grad():
        gx = rnd(gy.float() + rnd(yf.grad).float())
        ga = gx if keep is None else rnd(gx.float() * keep.float())
    return y, rnd(z32.detach()), gx, ga


def test_contract_table_is_torchs_bf16_autocast_arithmetic():
    """Pins the contract the GPU test uses: y, z, grad_x, grad_a bit for bit, with and without keep."""
    x, a, gy, gz, norm, keep = _case()
    for k in (keep, None):
        got = _contract(x, a, k, norm, gy, gz)
        want = _autocast_composition(x, a, k, norm, gy, gz)
        for name, u, v in zip(("y", "z", "grad_x", "grad_a"), got, want):
            assert u.dtype == v.dtype == BF16 and torch.equal(u, v), (name, k is None)
    # the two readings the contract excludes are visibly different arithmetic at this size
    y, z, gx, _ = _contract(x, a, keep, norm, gy, gz)
    with torch.no_grad():
        unrounded = x.float() + (a.float() * keep.float()).to(BF16).float()
        z_unrounded = F.layer_norm(unrounded, norm.normalized_shape, norm.weight, norm.bias, norm.eps).to(BF16)
    assert (z_unrounded != z).float().mean().item() > 0.05


@pytest.mark.filterwarnings("ignore:.*CUDA is not available.*")
def test_cpu_bf16_tensors_run_the_torch_expressions(monkeypatch):
    """Both knobs on, CPU bf16 tensors, inside and outside autocast: forward and gradients bit for bit the expressions'."""
    from uvhand_amd.functions.swin_glue_func import add_norm_rows, add_rows, merge_norm, norm_rows
    monkeypatch.setenv("MSDA_SWIN_GLUE", "1")
    monkeypatch.setenv("MSDA_SWIN_GLUE_BF16", "1")
    B, H, W, width = 3, 3, 5, 8
    x, a, _, _, _, keep = _case(B, H * W, width, seed=4)
    g = torch.Generator().manual_seed(5)
    norm, norm4 = nn.LayerNorm(width).to(BF16), nn.LayerNorm(4 * width).to(BF16)
    with torch.no_grad():
        for p in list(norm.parameters()) + list(norm4.parameters()):
            p.copy_(torch.randn(p.shape, generator=g))

    def run(fn, params):
        for p in params:
            p.grad = None
        lx, la = _leaves(x, a)
        outs = fn(lx, la)
        outs = outs if isinstance(outs, tuple) else (outs,)
        sum((o * torch.arange(o.numel(), dtype=o.dtype).view(o.shape)).sum() for o in outs).backward()
        return [o.detach() for o in outs] + [lx.grad, la.grad] + [p.grad.clone() for p in params]

    def same(got, want):
        assert len(got) == len(want)
        for u, v in zip(got, want):
            assert (u is None and v is None) or (u.dtype == v.dtype and torch.equal(u, v))

    def merge(u, v):
        t = F.pad(u.view(B, H, W, width), (0, 0, 0, W % 2, 0, H % 2))
        t = torch.cat([t[:, 0::2, 0::2, :], t[:, 1::2, 0::2, :], t[:, 0::2, 1::2, :], t[:, 1::2, 1::2, :]], -1)
        return norm4(t.view(B, -1, 4 * width))
    pn, p4 = list(norm.parameters()), list(norm4.parameters())
    for ctx in (lambda: _autocast(BF16), lambda: torch.autocast("cpu", enabled=False)):
        with ctx():
            same(run(lambda u, v: norm_rows(u, norm), pn), run(lambda u, v: norm(u), pn))
            same(run(lambda u, v: norm_rows(u, norm, fp32_out=True), pn), run(lambda u, v: norm(u), pn))
            for k in (None, keep):
                def comp(u, v, k=k):
                    y = u + (v if k is None else v * k)
                    return y, norm(y)
                same(run(lambda u, v, k=k: add_norm_rows(u, v, k, norm), pn), run(comp, pn))
                same(run(lambda u, v, k=k: add_rows(u, v, k), []), run(lambda u, v, k=k: comp(u, v)[0], []))
            same(run(lambda u, v: merge_norm(u, H, W, norm4), p4), run(merge, p4))


def test_binding_picks_the_entry_from_the_stream_and_branch_types():
    from uvhand_amd import _native
    f32 = torch.float32
    for what, t, stream, want in (("swin_glue_norm_forward", f32, f32, "f32"), ("swin_glue_norm_forward", BF16, f32, "bf16"),
                                  ("swin_glue_norm_forward", f32, BF16, "f32_sbf16"),
                                  ("swin_glue_norm_backward", BF16, BF16, "bf16_sbf16"),
                                  ("swin_glue_add_norm_forward", BF16, BF16, "bf16_sbf16"),
                                  ("swin_glue_add_backward", BF16, f32, "bf16"),
                                  ("swin_glue_merge_norm_backward", BF16, BF16, "bf16_sbf16")):
        assert _native._glue_suffix(what, t, stream) == want
        assert "msda_" + what + "_" + want in _native.SIGNATURES
    for what, t, stream in (("swin_glue_add_forward", f32, BF16), ("swin_glue_merge_norm_forward", f32, BF16),
                            ("swin_glue_add_norm_forward", torch.float16, BF16), ("swin_glue_norm_forward", f32, torch.float16)):
        with pytest.raises(RuntimeError):
            _native._glue_suffix(what, t, stream)
