"""C ABI of the device-state step-tail entries (csrc/msda_optim.hip: msda_optim_advance_f32, msda_grad_norm_finish_dev_f32,
msda_adamw_step_dev_f32; added without an ABI version bump): the symbols are exported, and argument errors come back as codes
from the host-side checks before anything is launched (msda_launch_count unchanged) — so no GPU is needed, and the fake device
addresses below never reach a kernel."""
import ctypes

import pytest

P = 0x10000
ERR_ARGUMENT = 1
ENTRIES = ("msda_optim_advance_f32", "msda_grad_norm_finish_dev_f32", "msda_adamw_step_dev_f32")
TABLES = ("p", "g", "m", "v", "numel", "start", "group")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _err(lib):
    return lib.msda_last_error().decode()


def _step(lib, n=3, chunks=5, tables=None, step=P, ng=2, hyper=P, coef=P, skip=P):
    t = dict.fromkeys(TABLES, P)
    t.update(tables or {})
    return lib.msda_adamw_step_dev_f32(n, chunks, t["p"], t["g"], t["m"], t["v"], t["numel"], t["start"], t["group"], step, ng,
                                       hyper, coef, skip, None)


def _finish(lib, chunks=5, partials=P, max_norm=0.1, out=P, n=3, step=P, skip_nonfinite=0, status=P):
    return lib.msda_grad_norm_finish_dev_f32(chunks, partials, max_norm, out, n, step, skip_nonfinite, status, None)


def test_entries_exported_abi_unchanged(lib):
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def test_advance_argument_errors(lib):
    n0 = lib.msda_launch_count()
    adv = lib.msda_optim_advance_f32
    assert adv(-1, P, None) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert adv((1 << 20) + 1, P, None) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert adv(3, None, None) == ERR_ARGUMENT and "null step table" in _err(lib)
    assert lib.msda_launch_count() == n0


def test_finish_argument_errors(lib):
    n0 = lib.msda_launch_count()
    assert _finish(lib, n=-1) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert _finish(lib, n=(1 << 20) + 1) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert _finish(lib, chunks=-1) == ERR_ARGUMENT and _finish(lib, chunks=1 << 31) == ERR_ARGUMENT
    assert _finish(lib, partials=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _finish(lib, out=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _finish(lib, step=None) == ERR_ARGUMENT and "null step table" in _err(lib)
    assert _finish(lib, max_norm=float("nan")) == ERR_ARGUMENT and "max_norm" in _err(lib)
    assert _finish(lib, skip_nonfinite=1, status=None) == ERR_ARGUMENT and "status" in _err(lib)
    assert _finish(lib, chunks=0, n=0, skip_nonfinite=1, status=None) == ERR_ARGUMENT and "status" in _err(lib)
    assert lib.msda_launch_count() == n0


def test_step_argument_errors(lib):
    n0 = lib.msda_launch_count()
    for name in TABLES:
        assert _step(lib, tables={name: None}) == ERR_ARGUMENT and "null table" in _err(lib), name
    assert _step(lib, step=None) == ERR_ARGUMENT and "null step table" in _err(lib)
    assert _step(lib, hyper=None) == ERR_ARGUMENT and "null hyper table" in _err(lib)
    assert _step(lib, n=0, chunks=0, hyper=None) == ERR_ARGUMENT and "null hyper table" in _err(lib)
    assert _step(lib, n=-1) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert _step(lib, n=(1 << 20) + 1) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert _step(lib, ng=0) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert _step(lib, ng=9) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert _step(lib, chunks=-1) == ERR_ARGUMENT and _step(lib, chunks=1 << 31) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_an_empty_list_launches_nothing(lib):
    n0 = lib.msda_launch_count()
    none = dict.fromkeys(TABLES)
    assert lib.msda_optim_advance_f32(0, None, None) == 0 and _err(lib) == ""
    assert _finish(lib, chunks=0, partials=None, out=None, n=0, step=None, status=None) == 0 and _err(lib) == ""
    assert _finish(lib, chunks=0, partials=None, out=None, n=4, step=None, status=None) == 0      # tensors that are all empty
    assert _finish(lib, chunks=5, partials=None, out=None, n=0, step=None, status=None) == 0
    assert _step(lib, n=0, chunks=0, tables=none, step=None, coef=None, skip=None) == 0 and _err(lib) == ""
    assert _step(lib, n=4, chunks=0, tables=none, step=None, coef=None, skip=None) == 0
    assert lib.msda_launch_count() == n0
