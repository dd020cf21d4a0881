"""C ABI of the ARCTIC evaluation entries (csrc/msda_arctic_eval.hip; added without an ABI version bump): the symbols are
exported, the supported queries answer on the host, and argument errors come back as codes from the host-side checks before
anything is launched (msda_launch_count unchanged) — so no GPU is needed, and the fake device addresses never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
SYMBOLS = ("msda_nn_supported", "msda_nn_forward_f32", "msda_nn_backward_f32", "msda_arctic_metrics_supported",
           "msda_arctic_metrics_f32", "msda_arctic_metrics_accumulate_f32")
EV_DIMS = [32, 21, 778, 4000, 4000, 4000]


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


def _nn_fwd(lib, n=2, B=32, N1=4000, N2=778, src=None, trg=None, dists=None, idx=None):
    return lib.msda_nn_forward_f32(n, B, N1, N2, src if src is not None else _ptrs(max(n, 1)),
                                   trg if trg is not None else _ptrs(max(n, 1)), dists if dists is not None else _ptrs(max(n, 1)),
                                   idx if idx is not None else _ptrs(max(n, 1)), None)


def test_symbols_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_supported_limits(lib):
    assert lib.msda_nn_supported(32, 4000, 778) == 1
    assert lib.msda_nn_supported(32, 8192, 1024) == 1
    assert lib.msda_nn_supported(32, 8193, 778) == 0
    assert lib.msda_nn_supported(32, 4000, 1025) == 0
    assert lib.msda_nn_supported(32, 0, 778) == 0
    assert lib.msda_arctic_metrics_supported(*EV_DIMS) == 1
    assert lib.msda_arctic_metrics_supported(32, 21, 778, 8192, 8192, 8192) == 1
    assert lib.msda_arctic_metrics_supported(32, 21, 2000, 4000, 4000, 4000) == 0       # hand vertices over 1024
    assert lib.msda_arctic_metrics_supported(32, 40, 778, 4000, 4000, 4000) == 0        # joints over 32
    assert lib.msda_arctic_metrics_supported(32, 21, 778, 70000, 4000, 4000) == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(n=0), b"1 .. 8 pairs"),
    (dict(n=9), b"1 .. 8 pairs"),
    (dict(N2=1025), b"unsupported geometry"),
    (dict(N1=9000), b"unsupported geometry"),
    (dict(B=-1), b"unsupported geometry"),
    (dict(src=_ptrs(2, 0)), b"null pointer"),
    (dict(idx=_ptrs(2, 0)), b"null output"),
])
def test_nn_argument_errors(lib, kw, msg):
    before = lib.msda_launch_count()
    assert _nn_fwd(lib, **kw) == ERR_ARGUMENT
    assert msg in lib.msda_last_error()
    assert lib.msda_launch_count() == before


def test_nn_backward_argument_errors(lib):
    before = lib.msda_launch_count()
    rc = lib.msda_nn_backward_f32(2, 32, 4000, 778, _ptrs(2), _ptrs(2), _ptrs(2, 0), _ptrs(2), _ptrs(2), _ptrs(2), None)
    assert rc == ERR_ARGUMENT and b"null pointer" in lib.msda_last_error()
    rc = lib.msda_nn_backward_f32(2, 32, 4000, 778, _ptrs(2), _ptrs(2), _ptrs(2), None, _ptrs(2), _ptrs(2), None)
    assert rc == ERR_ARGUMENT and b"null pointer" in lib.msda_last_error()
    assert lib.msda_launch_count() == before


def test_metrics_argument_errors(lib):
    before = lib.msda_launch_count()
    assert lib.msda_arctic_metrics_f32(_ints([32, 21, 2000, 4000, 4000, 4000]), _ptrs(16), _ptrs(4), P, None) == ERR_ARGUMENT
    assert b"unsupported geometry" in lib.msda_last_error()
    assert lib.msda_arctic_metrics_f32(_ints(EV_DIMS), _ptrs(16, 0), _ptrs(4), P, None) == ERR_ARGUMENT
    assert b"null input" in lib.msda_last_error()
    assert lib.msda_arctic_metrics_f32(_ints(EV_DIMS), _ptrs(16), _ptrs(4), None, None) == ERR_ARGUMENT
    assert b"null pointer" in lib.msda_last_error()
    assert lib.msda_arctic_metrics_accumulate_f32(P, 32, None, P, None) == ERR_ARGUMENT
    assert lib.msda_arctic_metrics_accumulate_f32(P, -1, P, P, None) == ERR_ARGUMENT
    assert b"bad frame count" in lib.msda_last_error()
    assert lib.msda_launch_count() == before


def test_empty_batches_launch_nothing(lib):
    before = lib.msda_launch_count()
    assert _nn_fwd(lib, B=0) == 0
    assert lib.msda_nn_backward_f32(2, 0, 4000, 778, _ptrs(2), _ptrs(2), _ptrs(2), _ptrs(2), _ptrs(2), _ptrs(2), None) == 0
    assert lib.msda_arctic_metrics_f32(_ints([0, 21, 778, 4000, 4000, 4000]), _ptrs(16), _ptrs(4), P, None) == 0
    assert lib.msda_arctic_metrics_accumulate_f32(P, 0, P, P, None) == 0
    assert lib.msda_launch_count() == before
