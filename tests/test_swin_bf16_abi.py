"""C ABI of the bf16 Swin window attention (msda_swin_attn_*_bf16, additive at ABI 116) and the opt-in route's host-side
decisions.  No GPU: every call here fails its host-side checks, which come before any launch, so fake device addresses never
reach a kernel."""
import contextlib
import ctypes

import pytest
import torch

OK_PTR = 0x10000                 # 16-byte aligned; only ever passed next to an argument the checks refuse

GEO = (2, 9, 11, 64, 2, 7, 3)    # B, H, W, C, nH, ws, shift: a supported geometry
BAD_GEOS = [
    (2, 9, 11, 64, 2, 13, 3),    # ws > 12
    (2, 9, 11, 96, 2, 7, 3),     # C != 32 nH
    (2, 9, 11, 64, 2, 7, 7),     # shift >= ws
    (0, 9, 11, 64, 2, 7, 3), (2, 0, 11, 64, 2, 7, 3), (2, 9, -1, 64, 2, 7, 3), (2, 9, 11, 0, 0, 7, 3), (2, 9, 11, 64, 2, 0, 0),
]


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


def test_library_exports_the_bf16_swin_entries_at_abi_116(lib):
    for name in ("msda_swin_attn_forward_bf16", "msda_swin_attn_backward_bf16"):
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def _sizes(lib, geo=GEO):
    return lib.msda_swin_attn_workspace_bytes(*geo, 0), lib.msda_swin_attn_workspace_bytes(*geo, 1)


def _refused(lib, rc):
    assert rc == 1
    msg = lib.msda_last_error()
    assert msg
    return msg


def test_forward_argument_errors(lib):
    fn = lib.msda_swin_attn_forward_bf16
    p = OK_PTR
    lse_bytes, _ = _sizes(lib)
    assert lse_bytes > 0

    def call(geo=GEO, qkv=p, bias=p, table=p, out=p, lse=p, nbytes=lse_bytes):
        return fn(*geo, qkv, bias, table, out, lse, nbytes, None)
    for geo in BAD_GEOS:
        assert b"ws <= 12" in _refused(lib, call(geo=geo)), geo
    for name in ("qkv", "table", "out", "lse"):
        assert b"null" in _refused(lib, call(**{name: None})), name
    for name in ("qkv", "out"):
        for off in (2, 8):                                                   # bf16 element / half a 16-byte row chunk
            assert b"aligned" in _refused(lib, call(**{name: p + off})), name
    assert b"aligned" in _refused(lib, call(bias=p + 4))
    assert b"lse buffer" in _refused(lib, call(nbytes=lse_bytes - 1))
    assert b"lse buffer" in _refused(lib, call(nbytes=0))


def test_backward_argument_errors(lib):
    fn = lib.msda_swin_attn_backward_bf16
    p = OK_PTR
    lse_bytes, ws_bytes = _sizes(lib)
    assert ws_bytes > 0
    names = ("qkv", "bias", "table", "out", "lse", "grad_out", "grad_qkv", "grad_table", "grad_bias", "workspace")

    def call(geo=GEO, nbytes=lse_bytes, wbytes=ws_bytes, **over):
        a = {n: p for n in names}
        a.update(over)
        return fn(*geo, a["qkv"], a["bias"], a["table"], a["out"], a["lse"], nbytes, a["grad_out"], a["grad_qkv"],
                  a["grad_table"], a["grad_bias"], a["workspace"], wbytes, None)
    for geo in BAD_GEOS:
        assert b"ws <= 12" in _refused(lib, call(geo=geo)), geo
    for name in ("qkv", "table", "out", "lse", "grad_out", "grad_qkv", "grad_table", "workspace"):
        assert b"null" in _refused(lib, call(**{name: None})), name
    for name in ("qkv", "out", "grad_out", "grad_qkv"):
        for off in (2, 8):
            assert b"aligned" in _refused(lib, call(**{name: p + off})), name
    assert b"lse buffer" in _refused(lib, call(nbytes=lse_bytes - 1))
    assert b"workspace smaller" in _refused(lib, call(wbytes=ws_bytes - 1))
    assert b"workspace smaller" in _refused(lib, call(wbytes=0))


def test_the_two_forms_share_the_size_queries(lib):
    B, H, W, C, nH, ws, s = GEO
    pairs = B * 2 * 2 * nH                                                   # 9 x 11 padded to 14 x 14: 2 x 2 windows
    assert _sizes(lib) == (pairs * ws * ws * 4, pairs * ((2 * ws - 1) ** 2 + 64) * 4)
    assert lib.msda_swin_attn_supported(*GEO) == 1
    for geo in BAD_GEOS:
        assert lib.msda_swin_attn_supported(*geo) == 0 and _sizes(lib, geo) == (0, 0)


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
    from uvhand_amd.functions.swin_func import fused_route
    cuda, cpu = torch.device("cuda"), torch.device("cpu")
    monkeypatch.delenv("MSDA_SWIN_FUSED", raising=False)
    monkeypatch.setenv("MSDA_SWIN_BF16", "1")
    assert not fused_route(cpu, torch.float32, 192, 6, 12)
    assert not fused_route(cpu, torch.bfloat16, 192, 6, 12)
    with _autocast(torch.bfloat16):
        assert torch.is_autocast_enabled()
        assert not fused_route(cpu, torch.float32, 192, 6, 12)
        assert fused_route(cuda, torch.float32, 192, 6, 12)                 # the fp32 residual stream
        assert fused_route(cuda, torch.bfloat16, 192, 6, 12)                # the qkv Linear's output
        assert not fused_route(cuda, torch.float32, 192, 12, 12)            # head_dim 16
        assert not fused_route(cuda, torch.float32, 192, 6, 13)
        monkeypatch.setenv("MSDA_SWIN_FUSED", "0")
        assert not fused_route(cuda, torch.float32, 192, 6, 12)
        monkeypatch.delenv("MSDA_SWIN_FUSED")
    with _autocast(torch.float16):
        assert not fused_route(cuda, torch.float32, 192, 6, 12)
        assert not fused_route(cuda, torch.float16, 192, 6, 12)
    assert fused_route(cuda, torch.bfloat16, 192, 6, 12)                    # bf16 rows outside autocast
    assert not fused_route(cuda, torch.float16, 192, 6, 12)
    for off in (None, "0", ""):                                             # the knob unset or off: today's behaviour
        if off is None:
            monkeypatch.delenv("MSDA_SWIN_BF16")
        else:
            monkeypatch.setenv("MSDA_SWIN_BF16", off)
        with _autocast(torch.bfloat16):
            assert not fused_route(cuda, torch.float32, 192, 6, 12)
            assert not fused_route(cuda, torch.bfloat16, 192, 6, 12)
        assert fused_route(cuda, torch.float32, 192, 6, 12)
        assert not fused_route(cuda, torch.bfloat16, 192, 6, 12)
