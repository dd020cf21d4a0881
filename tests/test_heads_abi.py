"""C ABI of the DETR heads entries (csrc/msda_heads.hip; added without an ABI version bump): the symbols are exported and
argument errors come back as codes from the host-side checks before anything is launched (msda_launch_count unchanged) — so
no GPU is needed, and the fake device addresses below never reach a kernel."""
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


def _args(kind=0, L=6, M=9600, C=256, K=14, n_mlp=2, R=42, flags=0, hs=P, init=P, inter=P, cls=None, mlp=None, sh=None):
    cls = cls if cls is not None else _ptrs(8)
    mlp = mlp if mlp is not None else _ptrs(48)
    sh = sh if sh is not None else _ptrs(6)
    return [kind, L, M, C, K, n_mlp, R, flags, hs, init, inter, cls, cls, mlp, mlp, sh, sh]


def _fwd(lib, logits=P, kp=None, sh_out=None, hidden=P, sig=P, **kw):
    return lib.msda_heads_forward_f32(*_args(**kw), logits, kp if kp is not None else _ptrs(2),
                                      sh_out if sh_out is not None else _ptrs(6), hidden, sig, None)


def _bwd(lib, glog=P, gkp=None, ghs=P, gw=None, ws=P, ws_bytes=1 << 40, **kw):
    g = gw if gw is not None else _ptrs(48)
    return lib.msda_heads_backward_f32(*_args(**kw), P, P, glog, gkp if gkp is not None else _ptrs(2), _ptrs(6), ghs,
                                       g, g, g, g, g, g, ws, ws_bytes, None)


def test_entries_exported_abi_unchanged(lib):
    for name in ("msda_heads_supported", "msda_heads_workspace_bytes", "msda_heads_forward_f32", "msda_heads_backward_f32"):
        assert hasattr(lib, name)
    assert lib.msda_version() == 116
    assert lib.msda_heads_supported(256) == 1
    assert lib.msda_heads_supported(30) == 0 and lib.msda_heads_supported(0) == 0


def test_workspace_grows_with_rows(lib):
    small = lib.msda_heads_workspace_bytes(0, 6, 100, 256, 14, 2, 0)
    big = lib.msda_heads_workspace_bytes(0, 6, 9600, 256, 14, 2, 0)
    assert 0 < small < big
    assert lib.msda_heads_workspace_bytes(0, 9, 100, 256, 14, 2, 0) == 0          # more levels than the kernels take


def test_forward_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _fwd(lib, kind=2) == ERR_ARGUMENT and "kind" in _err(lib)
    assert _fwd(lib, L=0) == ERR_ARGUMENT and "L" in _err(lib)
    assert _fwd(lib, L=9) == ERR_ARGUMENT
    assert _fwd(lib, M=0) == ERR_ARGUMENT
    assert _fwd(lib, C=30) == ERR_ARGUMENT and "C" in _err(lib)
    assert _fwd(lib, K=0) == ERR_ARGUMENT
    assert _fwd(lib, n_mlp=1) == ERR_ARGUMENT                          # ARCTIC has 0 or 2 keypoint MLPs
    assert _fwd(lib, kind=1, n_mlp=2) == ERR_ARGUMENT
    assert _fwd(lib, R=2) == ERR_ARGUMENT                              # ARCTIC references are 42-d
    assert _fwd(lib, kind=1, n_mlp=1, R=3) == ERR_ARGUMENT
    assert _fwd(lib, flags=4) == ERR_ARGUMENT
    assert _fwd(lib, M=1 << 30) == ERR_ARGUMENT and "2^31" in _err(lib)
    assert _fwd(lib, hs=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _fwd(lib, init=None) == ERR_ARGUMENT
    assert _fwd(lib, inter=None) == ERR_ARGUMENT
    assert _fwd(lib, cls=_ptrs(8, 0)) == ERR_ARGUMENT
    assert _fwd(lib, mlp=_ptrs(48, 0)) == ERR_ARGUMENT
    assert _fwd(lib, sh=_ptrs(6, 0)) == ERR_ARGUMENT
    assert _fwd(lib, logits=None) == ERR_ARGUMENT
    assert _fwd(lib, kp=_ptrs(2, 0)) == ERR_ARGUMENT
    assert _fwd(lib, hidden=None) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_backward_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _bwd(lib, glog=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _bwd(lib, ghs=None) == ERR_ARGUMENT
    assert _bwd(lib, gkp=_ptrs(2, 0)) == ERR_ARGUMENT
    assert _bwd(lib, gw=_ptrs(48, 0)) == ERR_ARGUMENT
    assert _bwd(lib, ws=None) == ERR_ARGUMENT
    assert _bwd(lib, ws_bytes=16) == ERR_ARGUMENT and "workspace" in _err(lib)
    assert _bwd(lib, L=0) == ERR_ARGUMENT
    assert _bwd(lib, kind=-1) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0
