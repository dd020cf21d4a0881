"""C ABI of the MANO entries (csrc/msda_mano.hip; added without an ABI version bump): the symbols are exported and argument
errors come back as codes from the host-side checks before anything is launched (msda_launch_count unchanged) — so no GPU is
needed, and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
TIPS = [744, 320, 443, 554, 671]
SYMBOLS = ("msda_mano_supported", "msda_mano_workspace_bytes", "msda_mano_forward_f32", "msda_mano_backward_f32")


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


def _geo(Vn=778, nb=10, E=5, n_layers=2, index=None, layer=(0, 1), B=(32, 32), tensors=None):
    index = (PARENTS + TIPS) * n_layers if index is None else index
    return [Vn, nb, E, n_layers, tensors if tensors is not None else _ptrs(7 * n_layers), _ints(index), len(B), _ints(list(layer)),
            _ints(list(B)), None]


def _fwd(lib, geo=None, inputs=None, outputs=None):
    geo = geo or _geo()
    n = geo[6]
    return lib.msda_mano_forward_f32(*geo, inputs if inputs is not None else _ptrs(4 * n),
                                     outputs if outputs is not None else _ptrs(2 * n), None)


def _bwd(lib, geo=None, grads=None, ws=P, ws_bytes=1 << 40):
    geo = geo or _geo()
    n = geo[6]
    return lib.msda_mano_backward_f32(*geo, _ptrs(4 * n), _ptrs(2 * n), grads if grads is not None else _ptrs(4 * n), ws,
                                      ws_bytes, None)


def test_symbols_and_version(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def test_supported_and_workspace(lib):
    assert lib.msda_mano_supported(778, 10, 5) == 1
    assert lib.msda_mano_supported(778, 17, 5) == 0
    assert lib.msda_mano_supported(778, 10, 9) == 0
    assert lib.msda_mano_supported(0, 10, 5) == 0
    slices = (778 + 63) // 64
    per = 16 * 12 + 135 + 16 + 3
    assert lib.msda_mano_workspace_bytes(778, 10, 5, 2, _ints([32, 7])) == 39 * slices * per * 4
    assert lib.msda_mano_workspace_bytes(778, 10, 5, 17, _ints([1] * 17)) == 0


@pytest.mark.parametrize("case", ["dims", "layers", "groups", "root", "parent_order", "tip_range", "layer_range", "negative_B",
                                  "null_layer_tensor", "null_input", "null_output"])
def test_forward_argument_errors(lib, case):
    n0 = lib.msda_launch_count()
    bad_parents = list(PARENTS)
    if case == "dims":
        rc = _fwd(lib, _geo(nb=17))
    elif case == "layers":
        rc = _fwd(lib, _geo(n_layers=5, layer=(0, 1)))
    elif case == "groups":
        rc = _fwd(lib, _geo(layer=[0] * 17, B=[1] * 17))
    elif case == "root":
        bad_parents[0] = 0
        rc = _fwd(lib, _geo(index=(bad_parents + TIPS) * 2))
    elif case == "parent_order":
        bad_parents[3] = 5
        rc = _fwd(lib, _geo(index=(bad_parents + TIPS) * 2))
    elif case == "tip_range":
        rc = _fwd(lib, _geo(index=(PARENTS + TIPS[:4] + [778]) * 2))
    elif case == "layer_range":
        rc = _fwd(lib, _geo(layer=(0, 2)))
    elif case == "negative_B":
        rc = _fwd(lib, _geo(B=(32, -1)))
    elif case == "null_layer_tensor":
        rc = _fwd(lib, _geo(tensors=_ptrs(14, 0)))
    elif case == "null_input":
        rc = _fwd(lib, inputs=_ptrs(8, 0))
    else:
        rc = _fwd(lib, outputs=_ptrs(4, 0))
    assert rc == ERR_ARGUMENT
    assert lib.msda_last_error().decode().startswith("msda_mano")
    assert lib.msda_launch_count() == n0


@pytest.mark.parametrize("case", ["ws_small", "ws_null", "null_grads", "dims"])
def test_backward_argument_errors(lib, case):
    n0 = lib.msda_launch_count()
    if case == "ws_small":
        rc = _bwd(lib, ws_bytes=64)
    elif case == "ws_null":
        rc = _bwd(lib, ws=None)
    elif case == "null_grads":
        rc = _bwd(lib, grads=_ptrs(8, 0))
    else:
        rc = _bwd(lib, _geo(Vn=9000))
    assert rc == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_empty_groups_launch_nothing(lib):
    n0 = lib.msda_launch_count()
    assert _fwd(lib, _geo(B=(0, 0)), inputs=_ptrs(8, 0), outputs=_ptrs(4, 0)) == 0
    assert lib.msda_launch_count() == n0
