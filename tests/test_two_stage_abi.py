"""C ABI of the two-stage entries (csrc/msda_two_stage.hip; added without an ABI version bump): the symbols are exported and
argument errors come back as codes from the host-side checks, before anything is launched — so no GPU is needed, and the
fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000                      # 16-byte aligned fake device address, only passed next to an argument the checks refuse
ERR_ARGUMENT = 1

NEW_ENTRIES = ("msda_two_stage_proposals_f32", "msda_two_stage_select_supported", "msda_two_stage_select_f32",
               "msda_proposal_pos_embed_f32", "msda_proposal_pos_linear_relu_f32")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _err(lib):
    return lib.msda_last_error().decode()


def test_entries_exported_abi_unchanged(lib):
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def _levels(*hw):
    hs = (ctypes.c_int * len(hw))(*[h for h, _ in hw])
    ws = (ctypes.c_int * len(hw))(*[w for _, w in hw])
    return ctypes.cast(hs, V), ctypes.cast(ws, V), hs, ws


def test_proposals_argument_errors(lib):
    fn = lib.msda_two_stage_proposals_f32
    hs, ws, _keep1, _keep2 = _levels((4, 4), (2, 2))
    assert fn(P, P, 2, 21, 256, 2, hs, ws, None, P, P, P, None) == ERR_ARGUMENT       # S != sum H*W
    assert "sum" in _err(lib)
    assert fn(P, P, 2, 20, 254, 2, hs, ws, None, P, P, P, None) == ERR_ARGUMENT       # C not a multiple of 4
    assert fn(P, P, 2, 20, 256, 17, hs, ws, None, P, P, P, None) == ERR_ARGUMENT      # L > 16
    assert fn(P, P, 2, 20, 256, 2, None, ws, None, P, P, P, None) == ERR_ARGUMENT     # no level table
    assert fn(None, P, 2, 20, 256, 2, hs, ws, None, P, P, P, None) == ERR_ARGUMENT    # null memory
    assert "null" in _err(lib)
    assert fn(P + 4, P, 2, 20, 256, 2, hs, ws, None, P, P, P, None) == ERR_ARGUMENT   # misaligned rows
    hz, wz, _k1, _k2 = _levels((0, 4))
    assert fn(P, P, 2, 0, 256, 1, hz, wz, None, P, P, P, None) == ERR_ARGUMENT        # empty level


def test_select_supported_and_errors(lib):
    sup = lib.msda_two_stage_select_supported
    assert sup(3060, 14, 300) == 1 and sup(8192, 14, 300) == 1
    assert sup(8193, 14, 300) == 0                   # above the LDS plan: the caller takes the composition
    assert sup(100, 14, 101) == 0 and sup(100, 0, 10) == 0
    fn = lib.msda_two_stage_select_f32
    assert fn(P, P, P, P, 2, 100, 14, 101, 12, 13, None, P, P, None) == ERR_ARGUMENT    # Q > S
    assert "out of range" in _err(lib)
    assert fn(P, P, P, P, 2, 8193, 14, 300, 12, 13, None, P, P, None) == ERR_ARGUMENT   # S above 8192
    assert "8192" in _err(lib)
    assert fn(P, P, P, P, 2, 100, 0, 10, 12, 13, None, P, P, None) == ERR_ARGUMENT      # K = 0
    assert fn(P, None, P, P, 2, 100, 14, 10, 12, 13, None, P, P, None) == ERR_ARGUMENT  # null hand source
    assert fn(P, P, P, P, 2, 100, 14, 10, 12, 13, None, P, None, None) == ERR_ARGUMENT  # null output


def test_pos_embed_argument_errors(lib):
    pe = lib.msda_proposal_pos_embed_f32
    assert pe(P, P, -1, P, None) == ERR_ARGUMENT
    assert pe(None, P, 10, P, None) == ERR_ARGUMENT
    assert pe(P, P, 10, P + 4, None) == ERR_ARGUMENT
    assert pe(P, P, 1 << 20, P, None) == ERR_ARGUMENT                                  # M * 5376 beyond 2^31
    lin = lib.msda_proposal_pos_linear_relu_f32
    assert lin(P, P, P, P, 10, 1022, P, None) == ERR_ARGUMENT                           # out % 4 != 0
    assert lin(P, P, None, P, 10, 1024, P, None) == ERR_ARGUMENT                        # null weight
    assert lin(P, None, P, P, 10, 1024, P, None) == ERR_ARGUMENT                        # null dim_t
    assert lin(P, P, P + 4, P, 10, 1024, P, None) == ERR_ARGUMENT                       # misaligned weight
    assert lin(None, P, P, P, 10, 1024, P, None) == ERR_ARGUMENT                        # null refpoints
    assert "null" in _err(lib)
