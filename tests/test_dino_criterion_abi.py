"""C ABI of the DINO criterion entries (csrc/msda_criterion_dino.hip; added without an ABI version bump): the symbols are
exported and argument errors come back as codes from the host-side checks before anything is launched (msda_launch_count
unchanged) — so no GPU is needed, and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
SETS = 8
QUERIES = [900] * 7 + [198]
MATCH_SET = [0, 1, 2, 3, 4, 5, 6, -1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _ptrs(n, value=P):
    return ctypes.cast((V * n)(*([value] * n)), V)


def _ints(values):
    return ctypes.cast((ctypes.c_int * len(values))(*values), V)


def _err(lib):
    return lib.msda_last_error().decode()


def _args(sets=SETS, bs=32, K=14, D=42, single_pad=6, groups=33, match=P, match_sets=7, t_max=3, labels=P, kp=P, off=P, n=96,
          valid=P, nb=P, logits=None, hand=None, obj=None, Q=None, match_set=None):
    m = max(sets, 1)
    p = _ptrs(m)
    return [logits if logits is not None else p, hand if hand is not None else p, obj if obj is not None else p,
            Q if Q is not None else _ints((QUERIES * 3)[:m]), match_set if match_set is not None else _ints((MATCH_SET * 3)[:m]),
            sets, bs, K, D, single_pad, groups, match, match_sets, t_max, labels, kp, off, n, valid, (1 << 12) | (1 << 13), nb,
            0.25]


def _fwd(lib, ws=P, ws_bytes=1 << 30, out=P, stats=P, **kw):
    return lib.msda_criterion_dino_fwd_f32(*_args(**kw), ws, ws_bytes, out, stats, None)


def _bwd(lib, grad=P, stats=P, g=None, **kw):
    gp = g if g is not None else _ptrs(SETS)
    return lib.msda_criterion_dino_bwd_f32(*_args(**kw), grad, stats, gp, gp, gp, None)


def test_entries_exported_abi_unchanged(lib):
    assert hasattr(lib, "msda_criterion_dino_fwd_f32") and hasattr(lib, "msda_criterion_dino_bwd_f32")
    assert hasattr(lib, "msda_criterion_fwd_f32") and hasattr(lib, "msda_criterion_bwd_f32")
    assert lib.msda_version() == 116


@pytest.mark.parametrize("call", ["fwd", "bwd"])
def test_argument_errors(lib, call):
    f = _fwd if call == "fwd" else _bwd
    n0 = lib.msda_launch_count()
    assert f(lib, sets=0) == ERR_ARGUMENT and "sets" in _err(lib)
    assert f(lib, sets=17) == ERR_ARGUMENT
    assert f(lib, bs=0) == ERR_ARGUMENT
    assert f(lib, bs=1025) == ERR_ARGUMENT
    assert f(lib, K=0) == ERR_ARGUMENT
    assert f(lib, n=-1) == ERR_ARGUMENT
    assert f(lib, Q=_ints([900] * 3 + [0] + [900] * 3 + [198])) == ERR_ARGUMENT and "Q[s]" in _err(lib)
    assert f(lib, match_set=_ints([0, 1, 2, 3, 4, 5, 7, -1])) == ERR_ARGUMENT and "match_sets" in _err(lib)   # 7 >= match_sets
    assert f(lib, match_sets=0) == ERR_ARGUMENT
    assert f(lib, t_max=17) == ERR_ARGUMENT                            # more than 16 targets in a frame
    assert f(lib, t_max=-1) == ERR_ARGUMENT
    assert f(lib, match=None) == ERR_ARGUMENT and "null" in _err(lib)  # a matched set without the match buffer
    assert f(lib, groups=0) == ERR_ARGUMENT and "denoising" in _err(lib)
    assert f(lib, single_pad=0) == ERR_ARGUMENT
    assert f(lib, groups=32) == ERR_ARGUMENT                           # Q[s] != groups * single_pad
    assert f(lib, Q=_ints([900] * 7 + [199])) == ERR_ARGUMENT
    assert f(lib, D=0) == ERR_ARGUMENT and "D" in _err(lib)            # keypoints without D
    assert f(lib, kp=None) == ERR_ARGUMENT                             # D without keypoints
    for name in ("logits", "hand", "obj"):
        assert f(lib, **{name: _ptrs(SETS, 0)}) == ERR_ARGUMENT and "null" in _err(lib)   # a null pointer in a set array
        assert f(lib, **{name: V(0)}) == ERR_ARGUMENT
    assert f(lib, Q=V(0)) == ERR_ARGUMENT
    assert f(lib, match_set=V(0)) == ERR_ARGUMENT
    assert f(lib, off=None) == ERR_ARGUMENT
    assert f(lib, labels=None) == ERR_ARGUMENT
    assert f(lib, valid=None) == ERR_ARGUMENT
    assert f(lib, nb=None) == ERR_ARGUMENT
    assert f(lib, bs=1024, K=1 << 12) == ERR_ARGUMENT and "2^31" in _err(lib)
    assert lib.msda_launch_count() == n0


def test_forward_outputs_and_workspace(lib):
    n0 = lib.msda_launch_count()
    assert _fwd(lib, ws=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _fwd(lib, ws=P + 4) == ERR_ARGUMENT and "workspace" in _err(lib)
    chunks = 32 * (7 * 4 + 1)                                          # ceil(900 / 256) = 4, ceil(198 / 256) = 1
    assert _fwd(lib, ws_bytes=64 * chunks - 1) == ERR_ARGUMENT and "workspace" in _err(lib)
    assert _fwd(lib, out=None) == ERR_ARGUMENT
    assert _fwd(lib, stats=None) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_workspace_bytes_helper_agrees_with_the_header():
    from uvhand_amd import _native
    assert _native.criterion_dino_workspace_bytes(32, QUERIES) == 64 * 32 * (7 * 4 + 1)
    assert _native.criterion_dino_workspace_bytes(1, [256, 257]) == 64 * 3


def test_backward_gradient_pointers(lib):
    n0 = lib.msda_launch_count()
    assert _bwd(lib, grad=None) == ERR_ARGUMENT and "null" in _err(lib)
    assert _bwd(lib, stats=None) == ERR_ARGUMENT
    assert _bwd(lib, g=_ptrs(SETS, 0)) == ERR_ARGUMENT                 # a null gradient pointer
    assert _bwd(lib, g=V(0)) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_only_denoising_sets_need_no_match_buffer(lib):
    """The one argument error left for a call of denoising sets alone is the missing workspace: match may be NULL."""
    n0 = lib.msda_launch_count()
    kw = dict(sets=2, Q=_ints([198, 198]), match_set=_ints([-1, -1]), match=None, match_sets=0, t_max=0)
    assert _fwd(lib, ws=None, **kw) == ERR_ARGUMENT and "null" in _err(lib) and "match" not in _err(lib)
    assert lib.msda_launch_count() == n0
