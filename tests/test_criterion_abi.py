"""C ABI of the criterion entries (csrc/msda_criterion.hip; added without an ABI version bump): the symbols are exported and
argument errors come back as codes from the host-side checks before anything is launched (msda_launch_count unchanged) —
so no GPU is needed, and the fake device addresses below never reach a kernel."""
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


def _args(kind=0, sets=7, bs=32, Q=300, K=14, D=42, match=P, t_max=3, labels=P, kp=P, off=P, n=96, valid=P, jv=P, nb=P,
          ptrs=None):
    p = ptrs if ptrs is not None else _ptrs(max(sets, 1))
    return [kind, p, p, p, sets, bs, Q, K, D, match, t_max, labels, kp, off, n, valid, jv, (1 << 12) | (1 << 13), nb, 0.25]


def _fwd(lib, out=P, stats=P, **kw):
    return lib.msda_criterion_fwd_f32(*_args(**kw), out, stats, None)


def _bwd(lib, grad=P, stats=P, g=None, **kw):
    gp = g if g is not None else _ptrs(7)
    return lib.msda_criterion_bwd_f32(*_args(**kw), grad, stats, gp, gp, gp, None)


def test_entries_exported_abi_unchanged(lib):
    assert hasattr(lib, "msda_criterion_fwd_f32") and hasattr(lib, "msda_criterion_bwd_f32")
    assert lib.msda_version() == 116


def test_forward_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _fwd(lib, kind=2) == ERR_ARGUMENT and "kind" in _err(lib)
    assert _fwd(lib, sets=0) == ERR_ARGUMENT and "sets" in _err(lib)
    assert _fwd(lib, sets=17) == ERR_ARGUMENT
    assert _fwd(lib, bs=0) == ERR_ARGUMENT
    assert _fwd(lib, bs=1025) == ERR_ARGUMENT
    assert _fwd(lib, Q=0) == ERR_ARGUMENT
    assert _fwd(lib, K=0) == ERR_ARGUMENT
    assert _fwd(lib, t_max=17) == ERR_ARGUMENT                        # more than 16 targets in a frame
    assert _fwd(lib, t_max=-1) == ERR_ARGUMENT
    assert _fwd(lib, D=0) == ERR_ARGUMENT and "D" in _err(lib)        # keypoints without D
    assert _fwd(lib, kp=None) == ERR_ARGUMENT                         # D without keypoints
    assert _fwd(lib, n=-1) == ERR_ARGUMENT
    assert _fwd(lib, match=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _fwd(lib, off=None) == ERR_ARGUMENT
    assert _fwd(lib, labels=None) == ERR_ARGUMENT
    assert _fwd(lib, nb=None) == ERR_ARGUMENT
    assert _fwd(lib, valid=None) == ERR_ARGUMENT                      # ARCTIC pairs slots through is_valid
    assert _fwd(lib, kind=1, jv=None) == ERR_ARGUMENT                 # AssemblyHands keypoints need joint_valid
    assert _fwd(lib, out=None) == ERR_ARGUMENT
    assert _fwd(lib, stats=None) == ERR_ARGUMENT
    assert _fwd(lib, ptrs=_ptrs(7, 0)) == ERR_ARGUMENT                # a null prediction pointer in the set arrays
    assert _fwd(lib, ptrs=V(0)) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_backward_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _bwd(lib, grad=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _bwd(lib, stats=None) == ERR_ARGUMENT
    assert _bwd(lib, g=_ptrs(7, 0)) == ERR_ARGUMENT                   # a null gradient pointer
    assert _bwd(lib, g=V(0)) == ERR_ARGUMENT
    assert _bwd(lib, sets=20) == ERR_ARGUMENT
    assert _bwd(lib, kind=-1) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0
