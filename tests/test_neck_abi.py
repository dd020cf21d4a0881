"""CPU-side checks of the input-projection neck's boundary (include/msda.h msda_neck_*, functions/neck_func.py): the symbols
and their signatures, argument errors before any launch, and the CPU route of input_proj_levels."""
import ctypes
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import neck_inputs as NI  # noqa: E402

SYMBOLS = ("msda_neck_supported", "msda_neck_forward_f32", "msda_neck_backward_f32")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    return _native


def test_symbols_exist_with_the_signatures_of_the_table(native):
    lib = native.declare(ctypes.CDLL(native.LIB_PATH))
    for name in SYMBOLS + ("msda_neck_workspace_bytes",):
        assert name in native.SIGNATURES
        fn = getattr(lib, name)
        restype, argtypes = native.signature(name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert native.signature("msda_neck_forward_f32")[1].count(ctypes.c_float) == 1            # eps
    assert len(native.signature("msda_neck_forward_f32")[1]) == 17 and len(native.signature("msda_neck_backward_f32")[1]) == 20


def test_geometry_and_argument_errors_are_host_logic(native):
    lib = native.load()
    I = ctypes.c_int
    hs, ws = (I * 2)(28, 1), (I * 2)(28, 1)
    assert lib.msda_neck_supported(2, 32, 256, 32, hs, ws) == 1
    assert lib.msda_neck_supported(2, 32, 250, 32, hs, ws) == 0                 # C not a multiple of groups
    assert lib.msda_neck_supported(9, 32, 256, 32, hs, ws) == 0                 # more than 8 levels
    assert lib.msda_neck_supported(2, 32, 256, 32, (I * 2)(28, 0), ws) == 0
    assert lib.msda_neck_workspace_bytes(4, 32, 256) == 4 * 3 * 32 * 256 * 4
    assert lib.msda_neck_forward_f32(2, None, None, None, None, None, hs, ws, 1, 256, 32, 1e-5, None, None, None, None, None) == 1
    assert b"null table" in lib.msda_last_error()
    assert lib.msda_neck_forward_f32(2, None, None, None, None, None, hs, ws, 1, 250, 32, 1e-5, None, None, None, None, None) == 1
    assert b"unsupported geometry" in lib.msda_last_error()
    null = (ctypes.c_void_p * 2)()
    assert lib.msda_neck_forward_f32(2, null, None, null, null, None, hs, ws, 1, 256, 32, 1e-5, null, null, null, None, None) == 1
    assert b"null level pointer" in lib.msda_last_error()
    assert lib.msda_neck_backward_f32(2, null, null, None, null, null, null, None, hs, ws, 1, 256, 32, null, None, None, None,
                                      None, 0, None) == 1
    assert b"workspace" in lib.msda_last_error()
    # an empty batch is a successful call without a launch; it also clears this thread's message for the tests that follow
    n0 = lib.msda_launch_count()
    assert lib.msda_neck_forward_f32(2, null, None, null, null, None, hs, ws, 0, 256, 32, 1e-5, null, null, null, None, None) == 0
    assert lib.msda_last_error() == b"" and lib.msda_launch_count() == n0


def test_module_imports_and_the_cpu_route_is_the_reference(native):
    from uvhand_amd.functions import neck_func
    for name in ("mixed", "hidden256"):
        args = NI.build(name)
        got = NI.run(neck_func.input_proj_levels, *args)
        ref = NI.run(neck_func.input_proj_levels_reference, *args)
        for family in NI.NAMES:
            assert all(torch.equal(a, b) for a, b in zip(got[family], ref[family])), family
        shapes = neck_func.output_shapes(args[0], args[1])
        assert shapes == [tuple(o.shape) for o in got["out"]]


def test_modules_and_tensors_are_the_same_call(native):
    from uvhand_amd.functions.neck_func import input_proj_levels
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(8, 64, kernel_size=3, stride=2, padding=1)
    norm = torch.nn.GroupNorm(32, 64)
    x = torch.randn(2, 8, 7, 5)
    a, = input_proj_levels([x], [conv], [norm])
    b, = input_proj_levels([x], [(conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups)],
                           [(32, norm.weight, norm.bias, norm.eps)])
    assert torch.equal(a, b) and torch.equal(a, norm(conv(x)))
    plain = torch.nn.GroupNorm(32, 64, affine=False)
    c, = input_proj_levels([x], [conv], [plain])
    assert torch.equal(c, plain(conv(x)))
