"""C ABI of the DINO decoder entries (csrc/msda_dino.hip; added without an ABI version bump): the symbols are exported, they are in
the binding's table, and argument errors come back as codes from the host-side checks, before anything is launched — so no
GPU is needed, and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

P = 0x10000                      # 16-byte aligned fake device address, only passed next to an argument the checks refuse
ERR_ARGUMENT = 1

NEW_ENTRIES = ("msda_dino_sine_embed_f32", "msda_dino_query_pos_supported", "msda_dino_query_pos_forward_f32",
               "msda_dino_refine_forward_f32", "msda_dino_refine_backward_f32")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _err(lib):
    return lib.msda_last_error().decode()


def test_entries_exported_and_in_table(lib):
    from uvhand_amd import _native
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    assert lib.msda_version() == 116


def test_sine_embed_argument_errors(lib):
    fn = lib.msda_dino_sine_embed_f32
    assert fn(P, 4, P, 2, 64, P, P, None) == ERR_ARGUMENT             # width neither 2 nor 42
    assert "width" in _err(lib)
    assert fn(P, 42, P, 3, 64, P, P, None) == ERR_ARGUMENT            # M % N != 0
    assert "multiple of N" in _err(lib)
    assert fn(P, 42, P, 0, 64, P, P, None) == ERR_ARGUMENT            # no frames
    assert fn(P, 2, P, 2, -2, P, P, None) == ERR_ARGUMENT             # M < 0
    assert fn(P, 2, P, 2, 1 << 23, P, P, None) == ERR_ARGUMENT        # M * 256 beyond 2^31
    assert fn(None, 2, P, 2, 64, P, P, None) == ERR_ARGUMENT          # null points
    assert "null" in _err(lib)
    assert fn(P, 2, None, 2, 64, None, P, None) == ERR_ARGUMENT       # null table
    assert fn(P, 2, None, 2, 64, P, P + 4, None) == ERR_ARGUMENT      # misaligned output
    assert "aligned" in _err(lib)
    assert fn(None, 42, None, 2, 0, P, None, None) == 0               # nothing to do: no pointer is read


def test_query_pos_argument_errors_and_supported(lib):
    fn = lib.msda_dino_query_pos_forward_f32
    assert fn(P, 3, P, 2, 64, P, P, P, P, P, P, P, None) == ERR_ARGUMENT          # width
    assert fn(P, 42, P, 5, 64, P, P, P, P, P, P, P, None) == ERR_ARGUMENT         # M % N != 0
    assert fn(P, 42, P, 2, 64, P, None, P, P, P, P, P, None) == ERR_ARGUMENT      # null weight
    assert "null" in _err(lib)
    assert fn(P, 42, P, 2, 64, P, P, P, P, P, None, P, None) == ERR_ARGUMENT      # null h
    assert fn(P, 42, P, 2, 64, P, P + 8, P, P, P, P, P, None) == ERR_ARGUMENT     # misaligned w1
    assert "aligned" in _err(lib)
    assert fn(P, 42, P, 2, 64, P, P, P, P + 4, P, P, P, None) == ERR_ARGUMENT     # misaligned w2
    ok = lib.msda_dino_query_pos_supported
    assert ok(42, 32, 32 * 1098, 256, 256) == 1
    assert ok(2, 1, 1, 256, 256) == 1
    assert ok(42, 32, 32 * 1098, 512, 256) == 0                                    # hidden
    assert ok(42, 32, 32 * 1098, 256, 128) == 0                                    # out
    assert ok(4, 32, 32 * 1098, 256, 256) == 0                                     # width
    assert ok(42, 32, 32 * 1098 + 1, 256, 256) == 0                                # rows not a multiple of the frames
    assert ok(42, 1, 1 << 23, 256, 256) == 0                                       # beyond 2^31 elements


def test_refine_argument_errors(lib):
    fwd, bwd = lib.msda_dino_refine_forward_f32, lib.msda_dino_refine_backward_f32
    assert fwd(P, P, 0, P, P, 12, 13, 64, P, P, None) == ERR_ARGUMENT             # K < 1
    assert "K >= 1" in _err(lib)
    assert fwd(P, P, 14, P, P, 12, 13, -1, P, P, None) == ERR_ARGUMENT            # M < 0
    assert fwd(P, P, 14, P, P, 12, 13, 1 << 26, P, P, None) == ERR_ARGUMENT       # M * 42 beyond 2^31
    assert fwd(P, None, 14, P, P, 12, 13, 64, P, P, None) == ERR_ARGUMENT         # null logits
    assert "null" in _err(lib)
    assert fwd(P, P, 14, P, P, 12, 13, 64, P, None, None) == ERR_ARGUMENT         # null code
    assert fwd(None, None, 14, None, None, 12, 13, 0, None, None, None) == 0      # nothing to do
    assert bwd(P, P, P, -1, P, P, None) == ERR_ARGUMENT
    assert bwd(P, P, P, 1 << 26, P, P, None) == ERR_ARGUMENT
    assert bwd(P, P, None, 64, P, P, None) == ERR_ARGUMENT                        # null code
    assert bwd(None, None, None, 0, None, None, None) == 0


def test_wrappers_refuse_before_launch():
    import torch
    from uvhand_amd import _native
    with pytest.raises(RuntimeError):
        _native.dino_sine_embed(torch.zeros(4, 42), None, 2, torch.ones(64))
    with pytest.raises(RuntimeError):
        _native.dino_refine_forward(torch.zeros(4, 42), torch.zeros(4, 14), torch.zeros(4, 42), torch.zeros(4, 42))
