"""C ABI of the grouped query selection (csrc/msda_arctic_item.hip: msda_arctic_item_many_forward / _backward; added without
an ABI version bump): declared in the header, once in the binding's table, exported, and argument errors come back as codes from
the host-side checks before anything is launched (msda_launch_count unchanged) — so no GPU is needed, and the fake device
addresses below never reach a kernel."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
SYMBOLS = ("msda_arctic_item_many_forward", "msda_arctic_item_many_backward")
MAX_SETS = 8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _ptrs(n, value=P):
    return ctypes.cast((V * n)(*([value] * n)), V)


def _fwd(lib, n=2, bs=2, Q=10, K=14, obj_end=12, hand_l=12, hand_r=13, bf16=1, logits=None, sources=None, out=None, idx=P):
    m = max(n, 1)
    return lib.msda_arctic_item_many_forward(n, bs, Q, K, obj_end, hand_l, hand_r, bf16,
                                             logits if logits is not None else _ptrs(m),
                                             sources if sources is not None else _ptrs(6 * m),
                                             out if out is not None else _ptrs(9 * m), idx, None)


def _bwd(lib, n=2, bs=2, Q=10, bf16=1, idx=P, grad_out=None, grad_sources=None):
    m = max(n, 1)
    return lib.msda_arctic_item_many_backward(n, bs, Q, bf16, idx, grad_out if grad_out is not None else _ptrs(9 * m),
                                              grad_sources if grad_sources is not None else _ptrs(6 * m), None)


def test_header_table_export_and_version(lib):
    from uvhand_amd import _native
    header = open(os.path.join(ROOT, "include", "msda.h")).read()
    for name in SYMBOLS:
        assert len(re.findall(r"\bint %s\(" % name, header)) == 1, name
        assert hasattr(lib, name), name
    assert _native.SIGNATURES["msda_arctic_item_many_forward"] == "i iiiiiiii ppppp"
    assert _native.SIGNATURES["msda_arctic_item_many_backward"] == "i iiii pppp"
    assert "arctic_tools/process.py:20-70" in header[:header.index("int msda_arctic_item_many_forward(")].rsplit("/* ----", 1)[1]
    assert _native.SMALL_LOSS_MAX_SETS == MAX_SETS
    assert lib.msda_version() == 116


@pytest.mark.parametrize("case", ["no_sets", "too_many_sets", "bs", "Q", "hand_class", "obj_end", "size", "null_tables",
                                  "null_idx", "null_logits_entry", "null_source_entry", "null_out_entry"])
def test_forward_argument_errors(lib, case):
    n0 = lib.msda_launch_count()
    rc = {"no_sets": lambda: _fwd(lib, n=0),
          "too_many_sets": lambda: _fwd(lib, n=MAX_SETS + 1),
          "bs": lambda: _fwd(lib, bs=0),
          "Q": lambda: _fwd(lib, Q=0),
          "hand_class": lambda: _fwd(lib, hand_r=14),
          "obj_end": lambda: _fwd(lib, obj_end=15),
          "size": lambda: _fwd(lib, bs=1 << 16, Q=1 << 10),                 # bs * Q * 48 >= 2^31
          "null_tables": lambda: lib.msda_arctic_item_many_forward(2, 2, 10, 14, 12, 12, 13, 1, None, None, None, P, None),
          "null_idx": lambda: _fwd(lib, idx=None),
          "null_logits_entry": lambda: _fwd(lib, logits=_ptrs(2, 0)),
          "null_source_entry": lambda: _fwd(lib, sources=_ptrs(12, 0)),
          "null_out_entry": lambda: _fwd(lib, out=_ptrs(18, 0))}[case]()
    assert rc == ERR_ARGUMENT
    assert lib.msda_last_error().decode().startswith("msda_arctic_item_many_forward")
    assert lib.msda_launch_count() == n0


@pytest.mark.parametrize("case", ["no_sets", "too_many_sets", "bs", "Q", "size", "null_idx", "null_tables",
                                  "null_grad_source_entry"])
def test_backward_argument_errors(lib, case):
    n0 = lib.msda_launch_count()
    rc = {"no_sets": lambda: _bwd(lib, n=0),
          "too_many_sets": lambda: _bwd(lib, n=MAX_SETS + 1),
          "bs": lambda: _bwd(lib, bs=0),
          "Q": lambda: _bwd(lib, Q=0),
          "size": lambda: _bwd(lib, bs=1 << 16, Q=1 << 10),
          "null_idx": lambda: _bwd(lib, idx=None),
          "null_tables": lambda: lib.msda_arctic_item_many_backward(2, 2, 10, 1, P, None, None, None),
          "null_grad_source_entry": lambda: _bwd(lib, grad_sources=_ptrs(12, 0))}[case]()
    assert rc == ERR_ARGUMENT
    assert lib.msda_last_error().decode().startswith("msda_arctic_item_many_backward")
    assert lib.msda_launch_count() == n0
