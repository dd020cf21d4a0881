"""C ABI of the SmoothNet entries (csrc/msda_smoother.hip, csrc/msda_arctic_item.hip; added without an ABI version bump): the
symbols are exported and argument errors come back as codes from the host-side checks before anything is launched
(msda_launch_count unchanged) — so no GPU is needed, and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
SYMBOLS = ("msda_smoother_supported", "msda_smoother_workspace_bytes", "msda_smoother_forward_f32",
           "msda_smoother_backward_f32", "msda_smoother_dropout_mask_f32", "msda_arctic_item_forward_f32",
           "msda_arctic_item_backward_f32")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _ints(vals):
    return ctypes.cast((ctypes.c_int * len(vals))(*vals), V)


def _ptrs(n, value=P):
    return ctypes.cast((V * n)(*([value] * n)), V)


ARCTIC_MODS = [4, 4, 5, 0, 0, 1, 1, 2, 3]
ARCTIC_C = [3, 3, 3, 48, 48, 10, 10, 3, 1]


def _geo(T=32, O=32, H=512, R=256, nb=3, n_mod=6, mods=None, B=None, C=None):
    mods = ARCTIC_MODS if mods is None else mods
    B = [1] * len(mods) if B is None else B
    C = ARCTIC_C if C is None else C
    return [T, O, H, R, nb, n_mod, len(mods), _ints(mods), _ints(B), _ints(C)]


def _fwd(lib, geo=None, x=None, params=None, out=None, act=P, act_bytes=1 << 40, training=0, p=0.9, seed=P):
    geo = geo or _geo()
    return lib.msda_smoother_forward_f32(*geo, x if x is not None else _ptrs(9), params if params is not None else _ptrs(300),
                                         out if out is not None else _ptrs(9), act, act_bytes, training, p, seed, None)


def _bwd(lib, geo=None, act_bytes=1 << 40, ws=P, ws_bytes=1 << 40, grad_params=P, training=0, p=0.9, seed=P):
    geo = geo or _geo()
    return lib.msda_smoother_backward_f32(*geo, _ptrs(9), _ptrs(300), P, act_bytes, _ptrs(9), None, grad_params, training, p,
                                          seed, ws, ws_bytes, None)


def test_symbols_and_version(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def test_supported(lib):
    assert lib.msda_smoother_supported(32, 32, 512, 256, 3) == 1
    assert lib.msda_smoother_supported(3, 3, 64, 32, 2) == 1
    assert lib.msda_smoother_supported(2, 2, 64, 32, 2) == 0           # acc would be empty
    assert lib.msda_smoother_supported(32, 32, 510, 256, 3) == 0        # H % 4
    assert lib.msda_smoother_supported(32, 32, 512, 256, 5) == 0        # num_blocks


def test_workspace_bytes(lib):
    act = lib.msda_smoother_workspace_bytes(*_geo(), 0)
    ws = lib.msda_smoother_workspace_bytes(*_geo(), 1)
    rows = 2 * 3 + 3 + 2 * 48 + 2 * 10 + 3 + 1
    assert act == rows * (3 * (512 + 3 * (256 + 2 * 512)) + 3 * 32) * 4
    assert ws == rows * (3 * (4 * 512 + 3 * 256) + 3 * 32 + 3 * 32) * 4
    assert lib.msda_smoother_workspace_bytes(*_geo(T=2, O=2), 0) == 0


@pytest.mark.parametrize("case", ["dims", "modules", "calls_per_module", "module_range", "null_x", "null_param", "act_small",
                                  "unaligned_act", "p", "seed"])
def test_forward_argument_errors(lib, case):
    n0 = lib.msda_launch_count()
    params = _ptrs(300)
    if case == "dims":
        rc = _fwd(lib, geo=_geo(H=510))
    elif case == "modules":
        rc = _fwd(lib, geo=_geo(n_mod=7))
    elif case == "calls_per_module":
        rc = _fwd(lib, geo=_geo(mods=[0] * 5, B=[1] * 5, C=[3] * 5, n_mod=1))
    elif case == "module_range":
        rc = _fwd(lib, geo=_geo(mods=[0, 6, 1, 2, 3, 4, 5, 0, 1]))
    elif case == "null_x":
        rc = _fwd(lib, x=_ptrs(9, 0))
    elif case == "null_param":
        rc = _fwd(lib, params=_ptrs(300, 0))
    elif case == "act_small":
        rc = _fwd(lib, act_bytes=16)
    elif case == "unaligned_act":
        rc = _fwd(lib, act=P + 4)
    elif case == "p":
        rc = _fwd(lib, training=1, p=1.0)
    else:
        rc = _fwd(lib, training=1, p=0.5, seed=None)
    assert rc == ERR_ARGUMENT
    assert lib.msda_last_error().decode().startswith("msda_smoother")
    assert lib.msda_launch_count() == n0
    del params


@pytest.mark.parametrize("case", ["ws_small", "null_grad_params", "act_small", "dims"])
def test_backward_argument_errors(lib, case):
    n0 = lib.msda_launch_count()
    if case == "ws_small":
        rc = _bwd(lib, ws_bytes=64)
    elif case == "null_grad_params":
        rc = _bwd(lib, grad_params=None)
    elif case == "act_small":
        rc = _bwd(lib, act_bytes=64)
    else:
        rc = _bwd(lib, geo=_geo(R=6))
    assert rc == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_mask_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert lib.msda_smoother_dropout_mask_f32(None, 0, 1, 4, 4, 0.9, P, None) == ERR_ARGUMENT
    assert lib.msda_smoother_dropout_mask_f32(P, 0, 64, 4, 4, 0.9, P, None) == ERR_ARGUMENT
    assert lib.msda_smoother_dropout_mask_f32(P, 0, 1, 4, 4, 1.0, P, None) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_arctic_item_argument_errors(lib):
    n0 = lib.msda_launch_count()
    f = lib.msda_arctic_item_forward_f32
    assert f(2, 10, 14, 12, 12, 14, P, _ptrs(6), _ptrs(9), P, None) == ERR_ARGUMENT      # hand class out of range
    assert f(2, 10, 14, 15, 12, 13, P, _ptrs(6), _ptrs(9), P, None) == ERR_ARGUMENT      # obj_end > K
    assert f(2, 0, 14, 12, 12, 13, P, _ptrs(6), _ptrs(9), P, None) == ERR_ARGUMENT
    assert f(2, 10, 14, 12, 12, 13, P, _ptrs(6, 0), _ptrs(9), P, None) == ERR_ARGUMENT
    assert f(2, 10, 14, 12, 12, 13, P, _ptrs(6), _ptrs(9), None, None) == ERR_ARGUMENT
    b = lib.msda_arctic_item_backward_f32
    assert b(2, 10, None, _ptrs(9), _ptrs(6), None) == ERR_ARGUMENT
    assert b(2, 10, P, _ptrs(9), _ptrs(6, 0), None) == ERR_ARGUMENT
    assert b(0, 10, P, _ptrs(9), _ptrs(6), None) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0
