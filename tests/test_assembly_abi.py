"""C ABI of the AssemblyHands entries (csrc/msda_assembly.hip; added without an ABI version bump): the symbols are exported and
argument errors come back as codes from the host-side checks, before anything is launched — so no GPU is needed, and the
fake device addresses below never reach a kernel."""
import ctypes

import pytest

P = 0x10000                      # 16-byte aligned fake device address, only passed next to an argument the checks refuse
ERR_ARGUMENT = 1

NEW_ENTRIES = ("msda_assembly_refine_f32", "msda_assembly_proposals_f32", "msda_assembly_select_f32")


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


def test_refine_argument_errors(lib):
    fn = lib.msda_assembly_refine_f32
    assert fn(P, 4, P, 3, P, 1200, P, None) == ERR_ARGUMENT           # width neither 2 nor 42
    assert "width" in _err(lib)
    assert fn(P, 2, P, 0, P, 1200, P, None) == ERR_ARGUMENT           # K = 0
    assert fn(P, 2, P, 3, P, -1, P, None) == ERR_ARGUMENT             # M < 0
    assert fn(P, 42, P, 3, P, 1 << 26, P, None) == ERR_ARGUMENT       # M * 63 beyond 2^31
    assert fn(P, 42, None, 3, P, 1200, P, None) == ERR_ARGUMENT       # null logits
    assert "null" in _err(lib)
    assert fn(P, 42, P, 3, P, 1200, None, None) == ERR_ARGUMENT       # null output
    assert fn(None, 42, None, 3, None, 0, None, None) == 0            # nothing to do: no pointer is read


def test_proposals_argument_errors(lib):
    fn = lib.msda_assembly_proposals_f32
    S, C = 16, 256
    stride = 1045 * C
    assert fn(P, stride, P, 1045, 4, 4, 4, 254, P, P, P, None) == ERR_ARGUMENT        # C not a multiple of 4
    assert fn(P, stride, P, 1045, 4, 0, 4, C, P, P, P, None) == ERR_ARGUMENT          # empty level
    assert fn(P, S * C - 4, P, 1045, 4, 4, 4, C, P, P, P, None) == ERR_ARGUMENT       # frame stride below H*W rows
    assert "stride" in _err(lib)
    assert fn(P, stride + 2, P, 1045, 4, 4, 4, C, P, P, P, None) == ERR_ARGUMENT      # stride breaks 16-byte rows
    assert fn(P, stride, P, 8, 4, 4, 4, C, P, P, P, None) == ERR_ARGUMENT             # mask stride below H*W
    assert fn(P, stride, None, 1045, 4, 4, 4, C, P, P, P, None) == ERR_ARGUMENT       # null mask
    assert "null" in _err(lib)
    assert fn(P + 4, stride, P, 1045, 4, 4, 4, C, P, P, P, None) == ERR_ARGUMENT      # misaligned memory
    assert fn(P, stride, P, 1045, 1 << 20, 4, 4, C, P, P, P, None) == ERR_ARGUMENT    # beyond 2^31 elements


def test_select_argument_errors(lib):
    fn = lib.msda_assembly_select_f32
    assert fn(P, P, P, 2, 16, 10, 1, 8, 9, 10, None, P, None) == ERR_ARGUMENT         # class 10 with K = 10
    assert "out of range" in _err(lib)
    assert fn(P, P, P, 2, 16, 11, 8, 1, 9, 10, None, P, None) == ERR_ARGUMENT         # obj_last < obj_first
    assert fn(P, P, P, 2, 16, 40, 1, 20, 21, 22, None, P, None) == ERR_ARGUMENT       # more than 14 object classes
    assert fn(P, P, P, 2, 16, 11, 1, 8, -1, 10, None, P, None) == ERR_ARGUMENT        # negative class
    assert fn(P, P, P, 2, 0, 11, 1, 8, 9, 10, None, P, None) == ERR_ARGUMENT          # no rows
    assert fn(P, None, P, 2, 16, 11, 1, 8, 9, 10, None, P, None) == ERR_ARGUMENT      # null hand source
    assert "null" in _err(lib)
    assert fn(P, P, P, 2, 16, 11, 1, 8, 9, 10, None, None, None) == ERR_ARGUMENT      # null output


def test_wrapper_refuses_before_launch():
    """The Python wrappers refuse CPU tensors and a class layout below 11 classes (IndexError, as the reference's column
    indexing raises) without touching a device."""
    import torch
    from uvhand_amd import _native
    with pytest.raises(RuntimeError):
        _native.assembly_refine(torch.zeros(1, 3, 2), torch.zeros(1, 3, 3), torch.zeros(1, 3, 63))
    with pytest.raises(RuntimeError):
        _native.assembly_select(torch.zeros(1, 4, 11), torch.zeros(1, 4, 63), torch.zeros(1, 4, 63))
