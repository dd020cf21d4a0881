"""C ABI of the matcher entries (csrc/msda_matcher.hip; added without an ABI version bump): the symbols are exported and
argument errors come back as codes from the host-side checks before anything is launched (msda_launch_count unchanged) —
so no GPU is needed, and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
NEW_ENTRIES = ("msda_match_arctic_f32", "msda_match_assembly_f32", "msda_lsap_f32")


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


def test_entries_exported_abi_unchanged(lib):
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def _arctic(lib, sets=7, bs=32, Q=300, K=14, D=42, labels=P, kp=P, off=P, n=96, valid=P, t_max=3, out=P, ptrs=None):
    p = ptrs if ptrs is not None else _ptrs(max(sets, 1))
    return lib.msda_match_arctic_f32(p, p, p, sets, bs, Q, K, D, labels, kp, off, n, valid, t_max, 1.5, 4.0, out, None, None)


def test_arctic_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _arctic(lib, Q=1025) == ERR_ARGUMENT and "Q" in _err(lib)
    assert _arctic(lib, Q=0) == ERR_ARGUMENT
    assert _arctic(lib, t_max=17) == ERR_ARGUMENT                     # more than 16 targets in a frame
    assert _arctic(lib, t_max=-1) == ERR_ARGUMENT
    assert _arctic(lib, sets=0) == ERR_ARGUMENT and "sets" in _err(lib)
    assert _arctic(lib, sets=17) == ERR_ARGUMENT
    assert _arctic(lib, bs=-1) == ERR_ARGUMENT
    assert _arctic(lib, bs=1025) == ERR_ARGUMENT                      # frame (chunk) count
    assert _arctic(lib, K=0) == ERR_ARGUMENT
    assert _arctic(lib, D=65) == ERR_ARGUMENT and "D" in _err(lib)
    assert _arctic(lib, D=5, kp=None) == ERR_ARGUMENT                 # D without keypoints
    assert _arctic(lib, n=-1) == ERR_ARGUMENT
    assert _arctic(lib, off=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _arctic(lib, labels=None) == ERR_ARGUMENT
    assert _arctic(lib, valid=None) == ERR_ARGUMENT
    assert _arctic(lib, out=None) == ERR_ARGUMENT
    assert _arctic(lib, ptrs=_ptrs(7, 0)) == ERR_ARGUMENT             # a null prediction pointer in the set arrays
    assert _arctic(lib, ptrs=V(0)) == ERR_ARGUMENT                    # no set arrays at all
    assert lib.msda_launch_count() == n0


def test_assembly_argument_errors(lib):
    fn = lib.msda_match_assembly_f32
    n0 = lib.msda_launch_count()
    p = _ptrs(7)
    assert fn(p, p, 7, 32, 300, 3, 0, P, P, P, 48, 2, 1.0, 1.0, P, None, None) == ERR_ARGUMENT     # D = 0
    assert fn(p, p, 7, 32, 2000, 3, 63, P, P, P, 48, 2, 1.0, 1.0, P, None, None) == ERR_ARGUMENT  # Q > 1024
    assert fn(p, p, 7, 32, 300, 3, 63, P, None, P, 48, 2, 1.0, 1.0, P, None, None) == ERR_ARGUMENT  # null keypoints
    assert fn(p, _ptrs(7, 0), 7, 32, 300, 3, 63, P, P, P, 48, 2, 1.0, 1.0, P, None, None) == ERR_ARGUMENT
    assert fn(p, p, 20, 32, 300, 3, 63, P, P, P, 48, 2, 1.0, 1.0, P, None, None) == ERR_ARGUMENT  # sets
    assert lib.msda_launch_count() == n0


def test_lsap_argument_errors(lib):
    fn = lib.msda_lsap_f32
    n0 = lib.msda_launch_count()
    assert fn(P, 4, 300, 17, P, None) == ERR_ARGUMENT                 # min(Q, T) > 16
    assert fn(P, 4, 1025, 3, P, None) == ERR_ARGUMENT                 # max(Q, T) > 1024
    assert fn(P, 4, 3, 1025, P, None) == ERR_ARGUMENT
    assert fn(P, 4, 0, 3, P, None) == ERR_ARGUMENT                    # Q = 0
    assert fn(P, 4, 3, -1, P, None) == ERR_ARGUMENT
    assert fn(P, -1, 3, 3, P, None) == ERR_ARGUMENT
    assert fn(None, 4, 3, 3, P, None) == ERR_ARGUMENT and "null" in _err(lib)
    assert fn(P, 4, 3, 3, None, None) == ERR_ARGUMENT
    assert fn(None, 0, 3, 3, None, None) == 0                         # nothing to do: no pointer is read, no launch
    assert lib.msda_launch_count() == n0
