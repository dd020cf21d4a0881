"""C ABI of msda_heads_ref_backward_f32, the reference gradient of the ARCTIC keypoint epilogue (csrc/msda_heads.hip; added
without an ABI version bump): the symbol is exported and declared once in the binding's table, argument errors come back as codes
from the host-side check before anything is launched (msda_launch_count unchanged), and null outputs are accepted — so no GPU is
needed, and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _ptrs(n, value=P):
    return ctypes.cast((V * n)(*([value] * n)), V)


def _err(lib):
    return lib.msda_last_error().decode()


def _call(lib, L=6, M=9600, n_mlp=2, R=42, init=P, inter=P, sig=P, gkp="two", g_init=P, g_inter=P):
    gkp = _ptrs(2) if gkp == "two" else gkp
    return lib.msda_heads_ref_backward_f32(L, M, n_mlp, R, init, inter, sig, gkp, g_init, g_inter, None)


def test_entry_exported_and_declared_once(lib):
    from uvhand_amd import _native
    assert hasattr(lib, "msda_heads_ref_backward_f32")
    assert lib.msda_version() == 116
    assert _native.SIGNATURES["msda_heads_ref_backward_f32"].replace(" ", "") == "iiliippppppp"
    assert callable(_native.heads_ref_backward)


def test_argument_errors_launch_nothing(lib):
    n0 = lib.msda_launch_count()
    assert _call(lib, L=0) == ERR_ARGUMENT and "1 <= L <= 8" in _err(lib)
    assert _call(lib, L=9) == ERR_ARGUMENT and "1 <= L <= 8" in _err(lib)
    assert _call(lib, M=0) == ERR_ARGUMENT and "M >= 1" in _err(lib)
    assert _call(lib, M=-5) == ERR_ARGUMENT
    assert _call(lib, n_mlp=1) == ERR_ARGUMENT and "n_mlp" in _err(lib)
    assert _call(lib, n_mlp=0) == ERR_ARGUMENT
    assert _call(lib, R=2) == ERR_ARGUMENT and "R must be 42" in _err(lib)
    assert _call(lib, R=63) == ERR_ARGUMENT
    assert _call(lib, L=8, M=(1 << 31) // (8 * 42) + 1) == ERR_ARGUMENT and "2^31" in _err(lib)
    assert _call(lib, M=1 << 40) == ERR_ARGUMENT and "2^31" in _err(lib)
    assert _call(lib, M=1 << 62) == ERR_ARGUMENT and "2^31" in _err(lib)
    assert _call(lib, sig=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _call(lib, gkp=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _call(lib, gkp=ctypes.cast((V * 2)(P, None), V)) == ERR_ARGUMENT
    assert _call(lib, gkp=ctypes.cast((V * 2)(None, P), V)) == ERR_ARGUMENT
    assert _call(lib, init=None) == ERR_ARGUMENT and "null" in _err(lib)          # grad_init_ref is asked for
    assert _call(lib, inter=None) == ERR_ARGUMENT and "null" in _err(lib)         # grad_inter_ref is asked for
    assert _call(lib, inter=None, g_init=None) == ERR_ARGUMENT
    assert all(m.startswith("msda_heads_ref_backward: ") for m in [_err(lib)])
    assert lib.msda_launch_count() == n0


def test_null_outputs_are_accepted(lib):
    """Both outputs null: nothing to write, nothing read, no launch.  (One null output beside a written one is a GPU test.)"""
    n0 = lib.msda_launch_count()
    assert _call(lib, g_init=None, g_inter=None) == 0
    assert _call(lib, g_init=None, g_inter=None, init=None, inter=None) == 0
    assert _call(lib, L=1, g_init=None, inter=None) == 0                   # L == 1 has no later level: grad_inter_ref is not read
    assert _call(lib, L=1, g_init=None, g_inter=None, init=None, inter=None) == 0
    assert lib.msda_launch_count() == n0


def test_argument_checks_come_before_the_null_outputs_shortcut(lib):
    assert _call(lib, L=9, g_init=None, g_inter=None) == ERR_ARGUMENT
    assert _call(lib, sig=None, g_init=None, g_inter=None) == ERR_ARGUMENT
