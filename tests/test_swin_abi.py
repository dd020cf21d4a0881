"""C ABI of the Swin window-attention entries (csrc/msda_swin.hip via csrc/msda_abi.hip; added without an ABI version bump):
the symbols are exported, the supported predicate and workspace sizes follow the geometry, and argument errors come back as
codes from the host-side checks before anything is launched (msda_launch_count unchanged) — so no GPU is needed, and the fake
device addresses below never reach a kernel."""
import ctypes

import pytest

P = 0x10000
ERR_ARGUMENT = 1
SYMBOLS = ("msda_swin_attn_supported", "msda_swin_attn_workspace_bytes", "msda_swin_attn_forward_f32",
           "msda_swin_attn_backward_f32")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def test_symbols_and_version(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.msda_version() == 116


@pytest.mark.parametrize("geo,ok", [
    ((1, 14, 14, 768, 24, 12, 6), True), ((32, 56, 56, 192, 6, 12, 6), True), ((2, 9, 11, 64, 2, 7, 3), True),
    ((1, 1, 1, 32, 1, 1, 0), True), ((1, 7, 7, 1536, 48, 7, 3), True),
    ((1, 7, 7, 768, 48, 7, 3), False),        # head_dim 16 (the dilation=True last stage)
    ((1, 7, 7, 96, 2, 7, 3), False),          # head_dim 48
    ((1, 13, 13, 64, 2, 13, 6), False),       # window above 12
    ((1, 7, 7, 64, 2, 7, 7), False), ((1, 7, 7, 64, 2, 7, -1), False),       # shift outside [0, ws)
    ((0, 7, 7, 64, 2, 7, 0), False), ((1, 0, 7, 64, 2, 7, 0), False), ((1, 7, 0, 64, 2, 7, 0), False),
    ((1, 7, 7, 0, 0, 7, 0), False), ((1, 7, 7, 64, 2, 0, 0), False),
    ((4096, 512, 512, 768, 24, 12, 6), False),    # beyond 2^31 elements
])
def test_supported(lib, geo, ok):
    assert bool(lib.msda_swin_attn_supported(*geo)) == ok
    assert (lib.msda_swin_attn_workspace_bytes(*geo, 0) > 0) == ok
    assert (lib.msda_swin_attn_workspace_bytes(*geo, 1) > 0) == ok


def test_workspace_bytes(lib):
    B, H, W, C, nH, ws, s = 2, 14, 14, 768, 24, 12, 6           # 24 x 24 padded: 4 windows
    pairs = B * 4 * nH
    assert lib.msda_swin_attn_workspace_bytes(B, H, W, C, nH, ws, s, 0) == pairs * ws * ws * 4
    assert lib.msda_swin_attn_workspace_bytes(B, H, W, C, nH, ws, s, 1) == pairs * ((2 * ws - 1) ** 2 + 64) * 4
    assert lib.msda_swin_attn_workspace_bytes(B, H, W, C, nH, ws, s, 2) == 0


GOOD = (2, 9, 11, 64, 2, 7, 3)


def _fwd(lib, geo=GOOD, qkv=P, bias=P, table=P, out=P, lse=P, lse_bytes=None):
    if lse_bytes is None:
        lse_bytes = lib.msda_swin_attn_workspace_bytes(*GOOD, 0)
    return lib.msda_swin_attn_forward_f32(*geo, qkv, bias, table, out, lse, lse_bytes, None)


def _bwd(lib, geo=GOOD, ptrs=None, lse_bytes=None, ws_bytes=None):
    p = dict(qkv=P, bias=P, table=P, out=P, lse=P, gout=P, gqkv=P, gtable=P, gbias=P, ws=P)
    p.update(ptrs or {})
    if lse_bytes is None:
        lse_bytes = lib.msda_swin_attn_workspace_bytes(*GOOD, 0)
    if ws_bytes is None:
        ws_bytes = lib.msda_swin_attn_workspace_bytes(*GOOD, 1)
    return lib.msda_swin_attn_backward_f32(*geo, p["qkv"], p["bias"], p["table"], p["out"], p["lse"], lse_bytes, p["gout"],
                                           p["gqkv"], p["gtable"], p["gbias"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("kwargs", [
    dict(geo=(2, 9, 11, 96, 2, 7, 3)), dict(geo=(2, 9, 11, 64, 2, 13, 3)), dict(geo=(2, 9, 11, 64, 2, 7, 7)),
    dict(geo=(0, 9, 11, 64, 2, 7, 3)), dict(qkv=None), dict(table=None), dict(out=None), dict(lse=None),
    dict(qkv=P + 4), dict(bias=P + 8), dict(out=P + 4), dict(lse_bytes=16),
])
def test_forward_argument_errors(lib, kwargs):
    n0 = lib.msda_launch_count()
    assert _fwd(lib, **kwargs) == ERR_ARGUMENT
    assert lib.msda_last_error()
    assert lib.msda_launch_count() == n0


@pytest.mark.parametrize("kwargs", [
    dict(geo=(2, 9, 11, 96, 2, 7, 3)), dict(geo=(1, 7, 7, 64, 2, 7, -1)),
    dict(ptrs=dict(qkv=None)), dict(ptrs=dict(table=None)), dict(ptrs=dict(out=None)), dict(ptrs=dict(lse=None)),
    dict(ptrs=dict(gout=None)), dict(ptrs=dict(gqkv=None)), dict(ptrs=dict(gtable=None)), dict(ptrs=dict(ws=None)),
    dict(ptrs=dict(gqkv=P + 4)), dict(ptrs=dict(gout=P + 8)), dict(ptrs=dict(ws=P + 4)), dict(ptrs=dict(bias=P + 4)),
    dict(lse_bytes=0), dict(ws_bytes=64),
])
def test_backward_argument_errors(lib, kwargs):
    n0 = lib.msda_launch_count()
    assert _bwd(lib, **kwargs) == ERR_ARGUMENT
    assert lib.msda_last_error()
    assert lib.msda_launch_count() == n0
