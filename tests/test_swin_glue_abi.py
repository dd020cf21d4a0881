"""C ABI of the Swin glue kernels (msda_swin_glue_*, additive at ABI 116) and the opt-in route's host-side decisions
(MSDA_SWIN_GLUE).  No GPU: every call here fails its host-side checks, which come before any launch, so fake device addresses
never reach a kernel; the autograd functions are run on CPU tensors, where they are the torch expressions."""
import contextlib
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

OK_PTR = 0x10000                 # 16-byte aligned; only ever passed next to an argument the checks refuse
ROWS, RPS, C = 37, 5, 96
BAD_WIDTHS = (98, 3076, 0, -4)   # C % 4 != 0, C > 3072, empty, negative

ENTRIES = ["msda_swin_glue_supported", "msda_swin_glue_workspace_bytes"] + [
    "msda_swin_glue_%s_%s_%s" % (op, d, t) for op in ("norm", "add_norm", "add", "merge_norm") for d in ("forward", "backward")
    for t in ("f32", "bf16")]


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


def test_library_exports_the_glue_entries_at_abi_116(lib):
    from uvhand_amd import _native
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _native.SIGNATURES, name
    assert lib.msda_version() == 116


def _refused(lib, rc):
    assert rc == 1
    msg = lib.msda_last_error()
    assert msg
    return msg


def _formula(rows, width):
    return min(1024, max(1, -(-rows // 16))) * 2 * width * 4


def test_workspace_query_is_the_documented_formula(lib):
    for rows in (0, 1, 16, 17, 37, 16 * 1024, 16 * 1024 + 1, 10 ** 7):
        for width in (4, 96, 1024, 1028, 3072):
            assert lib.msda_swin_glue_workspace_bytes(rows, width) == _formula(rows, width), (rows, width)
    for width in BAD_WIDTHS:
        assert lib.msda_swin_glue_workspace_bytes(ROWS, width) == 0 and lib.msda_swin_glue_supported(width) == 0
    assert lib.msda_swin_glue_workspace_bytes(-1, 96) == 0
    for width in (4, 96, 3072):
        assert lib.msda_swin_glue_supported(width) == 1


# per entry: the argument names in the C order; "rows", "rps", "C", "eps", "wbytes", "B", "H", "W" are scalars, the rest pointers
_ARGS = {
    "norm_forward": "x gamma beta rows C eps z mean rstd",
    "norm_backward": "grad_z x gamma mean rstd rows C grad_x grad_gamma grad_beta workspace wbytes",
    "add_norm_forward": "x a keep rows rps C gamma beta eps y z mean rstd",
    "add_norm_backward": "grad_y grad_z y keep gamma mean rstd rows rps C grad_x grad_a grad_gamma grad_beta workspace wbytes",
    "add_forward": "x a keep rows rps C y",
    "add_backward": "grad_y keep rows rps C grad_a",
    "merge_norm_forward": "x B H W C gamma beta eps z mean rstd",
    "merge_norm_backward": "grad_z x gamma mean rstd B H W C grad_x grad_gamma grad_beta workspace wbytes",
}
_SCALARS = ("rows", "rps", "C", "eps", "wbytes", "B", "H", "W")
_TYPED = ("a", "z", "grad_z", "grad_a")                  # rows of T: 8-byte alignment for bf16, 16 for fp32
_F32_ROWS = ("x", "y", "grad_x", "grad_y", "gamma", "beta", "workspace")
MERGE = dict(B=2, H=3, W=5)                              # 2 x 2 x 3 merged rows


def _call(lib, op, suf, **over):
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
    return getattr(lib, "msda_swin_glue_%s_%s" % (op, suf))(*[vals[n] for n in names], None)


@pytest.mark.parametrize("suf", ["f32", "bf16"])
@pytest.mark.parametrize("op", list(_ARGS))
def test_argument_errors_come_before_any_launch(lib, op, suf):
    names = _ARGS[op].split()
    merge = op.startswith("merge")
    for width in BAD_WIDTHS + ((772,) if merge else ()):                        # 4 * 772 > 3072
        assert b"C % 4 == 0" in _refused(lib, _call(lib, op, suf, C=width)), width
    if "rps" in names:
        for bad in (0, -3):
            assert b"rows_per_sample" in _refused(lib, _call(lib, op, suf, rps=bad))
    if "rows" in names:
        assert b"rows" in _refused(lib, _call(lib, op, suf, rows=-1))
    else:
        assert b"H, W > 0" in _refused(lib, _call(lib, op, suf, H=0))
    optional = {"keep"} | ({"grad_a"} if (op, suf) == ("add_norm_backward", "f32") else set())
    for n in names:
        if n in _SCALARS:
            continue
        if n in optional:
            continue
        assert b"null" in _refused(lib, _call(lib, op, suf, **{n: None})), n
    if (op, suf) == ("add_norm_backward", "f32"):                               # grad_a may be null only without keep
        assert b"null" in _refused(lib, _call(lib, op, suf, grad_a=None))
    for n in names:
        if n in _F32_ROWS or (n in _TYPED and suf == "f32"):
            offs = (4, 8)
        elif n in _TYPED:
            offs = (2, 4)
        elif n == "keep":
            offs = (1,) if suf == "bf16" else (2,)
        elif n in ("mean", "rstd", "grad_gamma", "grad_beta"):
            offs = (2,)
        else:
            continue
        for off in offs:
            assert b"aligned" in _refused(lib, _call(lib, op, suf, **{n: OK_PTR + off})), (n, off)
    if "workspace" in names:
        full = lib.msda_swin_glue_workspace_bytes(MERGE["B"] * 6 if merge else ROWS, 4 * C if merge else C)
        assert full == _formula(MERGE["B"] * 6 if merge else ROWS, 4 * C if merge else C)
        for short in (full - 1, 0):
            assert b"workspace smaller" in _refused(lib, _call(lib, op, suf, wbytes=short))


@contextlib.contextmanager
def _autocast(dtype):
    """torch.autocast("cuda", dtype); where it switches itself off for want of a GPU, the same thread-local state set directly."""
    with torch.autocast("cuda", dtype=dtype):
        forced = not torch.is_autocast_enabled()
        before = torch.get_autocast_dtype("cuda")
        if forced:
            torch.set_autocast_enabled("cuda", True)
            torch.set_autocast_dtype("cuda", dtype)
        try:
            yield
        finally:
            if forced:
                torch.set_autocast_dtype("cuda", before)
                torch.set_autocast_enabled("cuda", False)


@pytest.mark.filterwarnings("ignore:.*CUDA is not available.*")
def test_route_decisions_without_a_gpu(monkeypatch):
    from uvhand_amd.functions.swin_glue_func import glue_route
    cuda, cpu = torch.device("cuda"), torch.device("cpu")
    for off in (None, "0", ""):                                             # the knob unset or off: today's behaviour
        if off is None:
            monkeypatch.delenv("MSDA_SWIN_GLUE", raising=False)
        else:
            monkeypatch.setenv("MSDA_SWIN_GLUE", off)
        assert not glue_route(cuda, torch.float32, 96)
        with _autocast(torch.bfloat16):
            assert not glue_route(cuda, torch.float32, 96)
    monkeypatch.setenv("MSDA_SWIN_GLUE", "1")
    for width, ok in ((96, True), (3072, True), (3076, False), (98, False), (0, False)):
        assert glue_route(cuda, torch.float32, width) == ok, width
        assert not glue_route(cpu, torch.float32, width)
        with _autocast(torch.bfloat16):
            assert torch.is_autocast_enabled()
            assert glue_route(cuda, torch.float32, width) == ok, width
            assert not glue_route(cpu, torch.float32, width)
        with _autocast(torch.float16):
            assert not glue_route(cuda, torch.float32, width)
    for dtype in (torch.bfloat16, torch.float16, torch.float64):            # the residual stream is fp32
        assert not glue_route(cuda, dtype, 96)
    # neither of the other two Swin knobs switches the glue on or off
    monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    assert glue_route(cuda, torch.float32, 96)
    monkeypatch.delenv("MSDA_SWIN_GLUE")
    assert not glue_route(cuda, torch.float32, 96)


def _leaves(*tensors):
    return [t.detach().clone().requires_grad_(True) for t in tensors]


def test_cpu_tensors_run_the_torch_expressions(monkeypatch):
    """Knob on, CPU tensors: forward and gradients bit for bit those of the expressions the modules run today."""
    from uvhand_amd.functions.swin_glue_func import add_norm_rows, add_rows, merge_norm, norm_rows
    monkeypatch.setenv("MSDA_SWIN_GLUE", "1")
    g = torch.Generator().manual_seed(3)
    B, H, W, width = 3, 3, 5, 8
    x, a, w = (torch.randn(B, H * W, width, generator=g) for _ in range(3))
    keep = torch.tensor([2.0, 0.0, 2.0]).view(B, 1, 1)
    norm = nn.LayerNorm(width)
    norm4 = nn.LayerNorm(4 * width)
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
            assert (u is None and v is None) or torch.equal(u, v)
    pn, p4 = list(norm.parameters()), list(norm4.parameters())
    same(run(lambda u, v: norm_rows(u, norm), pn), run(lambda u, v: norm(u), pn))
    same(run(lambda u, v: norm_rows(u, norm, fp32_out=True), pn), run(lambda u, v: norm(u), pn))
    for k in (None, keep):
        def comp(u, v, k=k):
            y = u + (v if k is None else v * k)
            return y, norm(y)
        same(run(lambda u, v, k=k: add_norm_rows(u, v, k, norm), pn), run(comp, pn))
        same(run(lambda u, v, k=k: add_rows(u, v, k), []), run(lambda u, v, k=k: comp(u, v)[0], []))

    def merge(u, v):
        t = F.pad(u.view(B, H, W, width), (0, 0, 0, W % 2, 0, H % 2))
        t = torch.cat([t[:, 0::2, 0::2, :], t[:, 1::2, 0::2, :], t[:, 0::2, 1::2, :], t[:, 1::2, 1::2, :]], -1)
        return norm4(t.view(B, -1, 4 * width))
    same(run(lambda u, v: merge_norm(u, H, W, norm4), p4), run(merge, p4))


def test_modules_are_unchanged_on_the_cpu(monkeypatch):
    """A block and a PatchMerging on the CPU give the same bits with the knob on and off (the knob reaches CUDA rows only)."""
    from uvhand_amd.modules import BasicLayer, PatchMerging
    torch.manual_seed(5)
    layer = BasicLayer(64, 2, 2, window_size=7, drop_path=0.3, downsample=PatchMerging).train()
    x = torch.randn(2, 9 * 11, 64)
    res = []
    for value in (None, "1"):
        if value is None:
            monkeypatch.delenv("MSDA_SWIN_GLUE", raising=False)
        else:
            monkeypatch.setenv("MSDA_SWIN_GLUE", value)
        layer.zero_grad(set_to_none=True)
        torch.manual_seed(6)
        out = layer(x, 9, 11)
        (out[0].sum() + out[3].sum()).backward()
        res.append([out[0].detach(), out[3].detach()] + [p.grad.clone() for p in layer.parameters()] + [torch.get_rng_state()])
    assert all(torch.equal(u, v) for u, v in zip(*res))
