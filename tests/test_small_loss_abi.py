"""C ABI of the ARCTIC object-layer and small-loss entries (csrc/msda_small_loss.hip; added without an ABI version bump): the
symbols are exported, the supported / workspace queries answer on the host, and argument errors come back as codes from the
host-side checks before anything is launched (msda_launch_count unchanged) — so no GPU is needed, and the fake device
addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
SYMBOLS = ("msda_object_supported", "msda_object_forward_f32", "msda_object_backward_f32", "msda_small_loss_supported",
           "msda_small_loss_workspace_bytes", "msda_small_loss_forward_f32", "msda_small_loss_backward_f32")
OBJ_DIMS = [11, 4000, 600, 8, 8, 16, 16]
SL_DIMS = [6, 32, 21, 778, 32, 10, 4000]


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


def _obj_fwd(lib, dims=OBJ_DIMS, B=(32,), lens=(4000,), model=None, inputs=None, outputs=None, n=None):
    n = len(B) if n is None else n
    return lib.msda_object_forward_f32(_ints(dims), model if model is not None else _ptrs(8), n, _ints(list(B)), _ints(list(lens)),
                                       inputs if inputs is not None else _ptrs(4 * len(B)),
                                       outputs if outputs is not None else _ptrs(4 * len(B)), None)


def _sl_fwd(lib, dims=SL_DIMS, img_res=224.0, ws_bytes=1 << 40, targets=None, losses=P):
    return lib.msda_small_loss_forward_f32(_ints(dims), img_res, targets if targets is not None else _ptrs(25),
                                           _ptrs(15 * dims[0]), losses, P, ws_bytes, None)


def test_symbols_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_supported_and_workspace(lib):
    assert lib.msda_object_supported(*OBJ_DIMS) == 1
    assert lib.msda_object_supported(65, 4000, 600, 8, 8, 16, 16) == 0
    assert lib.msda_object_supported(11, 70000, 600, 8, 8, 16, 16) == 0
    assert lib.msda_small_loss_supported(*SL_DIMS) == 1
    assert lib.msda_small_loss_supported(9, 32, 21, 778, 32, 10, 4000) == 0          # more than 8 sets
    assert lib.msda_small_loss_supported(6, 32, 21, 2000, 32, 10, 4000) == 0         # hand vertices over 1024
    assert lib.msda_small_loss_supported(6, 32, 21, 778, 31, 10, 4000) == 0          # odd keypoint count
    assert lib.msda_small_loss_workspace_bytes(*SL_DIMS) == (6 * 32 * 22 + 6 * 20) * 4
    assert lib.msda_small_loss_workspace_bytes(9, 32, 21, 778, 32, 10, 4000) == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(dims=[0, 4000, 600, 8, 8, 16, 16]), b"unsupported object model size"),
    (dict(n=0, B=(), lens=()), b"1 .. 16 groups"),
    (dict(B=(-1,)), b"negative batch"),
    (dict(lens=(4001,)), b"row count"),
    (dict(lens=(0,)), b"row count"),
    (dict(inputs=_ptrs(4, 0)), b"null pointer"),
    (dict(outputs=_ptrs(4, 0)), b"null output"),
    (dict(model=_ptrs(8, 0)), b"null model tensor"),
])
def test_object_argument_errors(lib, kw, msg):
    before = lib.msda_launch_count()
    assert _obj_fwd(lib, **kw) == ERR_ARGUMENT
    assert msg in lib.msda_last_error()
    assert lib.msda_launch_count() == before


@pytest.mark.parametrize("kw,msg", [
    (dict(dims=[9, 32, 21, 778, 32, 10, 4000]), b"unsupported geometry"),
    (dict(img_res=0.0), b"img_res"),
    (dict(ws_bytes=16), b"workspace smaller"),
    (dict(targets=_ptrs(25, 0)), b"null target"),
    (dict(losses=None), b"null pointer"),
])
def test_small_loss_argument_errors(lib, kw, msg):
    before = lib.msda_launch_count()
    assert _sl_fwd(lib, **kw) == ERR_ARGUMENT
    assert msg in lib.msda_last_error()
    assert lib.msda_launch_count() == before


def test_backward_argument_errors(lib):
    before = lib.msda_launch_count()
    rc = lib.msda_small_loss_backward_f32(_ints(SL_DIMS), 224.0, _ptrs(25), _ptrs(90), P, _ptrs(90, 0), P, 1 << 40, None)
    assert rc == ERR_ARGUMENT and b"null gradient" in lib.msda_last_error()
    rc = lib.msda_object_backward_f32(_ints(OBJ_DIMS), _ptrs(8), 1, _ints([32]), _ints([4000]), _ptrs(4), None, _ptrs(3), None)
    assert rc == ERR_ARGUMENT and b"null pointer" in lib.msda_last_error()
    assert lib.msda_launch_count() == before


def test_empty_groups_launch_nothing(lib):
    before = lib.msda_launch_count()
    assert _obj_fwd(lib, B=(0, 0), lens=(10, 10)) == 0
    assert lib.msda_object_backward_f32(_ints(OBJ_DIMS), _ptrs(8), 1, _ints([0]), _ints([10]), _ptrs(4), _ptrs(4), _ptrs(3),
                                        None) == 0
    assert _sl_fwd(lib, dims=[6, 0, 21, 778, 32, 10, 4000]) == 0
    rc = lib.msda_small_loss_backward_f32(_ints([6, 0, 21, 778, 32, 10, 4000]), 224.0, _ptrs(25), _ptrs(90), P, _ptrs(90), P,
                                          1 << 40, None)
    assert rc == 0
    assert lib.msda_launch_count() == before
