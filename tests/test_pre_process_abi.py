"""C ABI of the target-preparation entries (csrc/msda_pre_process.hip; added without an ABI version bump): the symbols are
exported, the two *_supported limits hold at their edges, and argument errors come back as codes from the host-side checks
before anything is launched (msda_launch_count unchanged) — so no GPU is needed, and the fake device addresses below never
reach a kernel."""
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


def _fit(lib, B=2, NK=16, J=21, res=224.0, ins=None, outs=None, status=P):
    return lib.msda_pre_fit_f32(B, NK, J, res, ins if ins is not None else _ptrs(8), outs if outs is not None else _ptrs(12),
                                status, None)


def _df(lib, B=2, NV=778, L=4000, hr=P, hl=P, obj=P, v_len=P, lo=0.0, hi=float("inf"), dists=None, idx=None):
    return lib.msda_dist_fields_f32(B, NV, L, hr, hl, obj, v_len, lo, hi, dists if dists is not None else _ptrs(4),
                                    idx if idx is not None else _ptrs(4), None)


def test_entries_exported_abi_unchanged(lib):
    for name in ("msda_pre_fit_supported", "msda_pre_fit_f32", "msda_dist_fields_supported", "msda_dist_fields_f32"):
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def test_supported_limits_at_their_edges(lib):
    fit, df = lib.msda_pre_fit_supported, lib.msda_dist_fields_supported
    assert fit(0, 3, 1) == 1 and fit(1 << 20, 64, 32) == 1 and fit(32, 16, 21) == 1
    assert fit(1, 2, 21) == 0 and fit(1, 65, 21) == 0 and fit(1, 16, 0) == 0 and fit(1, 16, 33) == 0 and fit(-1, 16, 21) == 0
    assert df(0, 1, 1) == 1 and df(1 << 20, 1024, 65536) == 1 and df(32, 778, 4000) == 1
    assert df(1, 0, 10) == 0 and df(1, 1025, 10) == 0 and df(1, 778, 0) == 0 and df(1, 778, 65537) == 0 and df(-1, 778, 10) == 0


def test_fit_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _fit(lib, NK=2) == ERR_ARGUMENT and "msda_pre_fit_supported" in _err(lib)
    assert _fit(lib, NK=65) == ERR_ARGUMENT and _fit(lib, J=0) == ERR_ARGUMENT and _fit(lib, J=33) == ERR_ARGUMENT
    assert _fit(lib, B=-1) == ERR_ARGUMENT
    assert _fit(lib, res=0.0) == ERR_ARGUMENT and "img_res" in _err(lib)
    assert _fit(lib, res=float("nan")) == ERR_ARGUMENT
    assert _fit(lib, ins=V(None)) == ERR_ARGUMENT and "null" in _err(lib)
    assert _fit(lib, outs=V(None)) == ERR_ARGUMENT
    assert _fit(lib, ins=_ptrs(8, None)) == ERR_ARGUMENT and "null input" in _err(lib)
    assert _fit(lib, outs=_ptrs(12, None)) == ERR_ARGUMENT and "null output" in _err(lib)
    assert _fit(lib, status=None) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_dist_fields_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _df(lib, NV=0) == ERR_ARGUMENT and "msda_dist_fields_supported" in _err(lib)
    assert _df(lib, NV=1025) == ERR_ARGUMENT and _df(lib, L=0) == ERR_ARGUMENT and _df(lib, L=65537) == ERR_ARGUMENT
    assert _df(lib, B=-1) == ERR_ARGUMENT
    assert _df(lib, lo=1.0, hi=0.5) == ERR_ARGUMENT and "dist_min" in _err(lib)
    assert _df(lib, lo=float("nan")) == ERR_ARGUMENT
    for name in ("hr", "hl", "obj", "v_len"):
        assert _df(lib, **{name: None}) == ERR_ARGUMENT and "null input" in _err(lib), name
    assert _df(lib, dists=V(None)) == ERR_ARGUMENT and _df(lib, idx=V(None)) == ERR_ARGUMENT
    assert _df(lib, dists=_ptrs(4, None)) == ERR_ARGUMENT and "null output" in _err(lib)
    assert lib.msda_launch_count() == n0


def test_an_empty_batch_launches_nothing(lib):
    n0 = lib.msda_launch_count()
    assert _fit(lib, B=0, ins=_ptrs(8, None), outs=_ptrs(12, None), status=None) == 0 and _err(lib) == ""
    assert _df(lib, B=0, hr=None, hl=None, obj=None, v_len=None, dists=_ptrs(4, None), idx=_ptrs(4, None)) == 0 and _err(lib) == ""
    assert lib.msda_launch_count() == n0
