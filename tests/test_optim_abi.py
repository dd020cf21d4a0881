"""C ABI of the step-tail entries (csrc/msda_optim.hip; added without an ABI version bump): the symbols are exported, the
msda_optim_supported limits hold at their edges, msda_optim_chunks lays chunks out as documented, and argument errors come
back as codes from the host-side checks before anything is launched (msda_launch_count unchanged) — so no GPU is needed, and
the fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
ENTRIES = ("msda_optim_supported", "msda_optim_chunk_elems", "msda_optim_chunks", "msda_grad_sumsq_f32",
           "msda_grad_norm_finish_f32", "msda_grad_scale_f32", "msda_adamw_step_f32")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _err(lib):
    return lib.msda_last_error().decode()


def _doubles(values):
    return ctypes.cast((ctypes.c_double * len(values))(*values), V)


def _chunks(lib, numels):
    n = len(numels)
    numel = (ctypes.c_longlong * max(1, n))(*numels)
    start = (ctypes.c_longlong * (n + 1))(*([-7] * (n + 1)))
    total = lib.msda_optim_chunks(n, ctypes.cast(numel, V), ctypes.cast(start, V))
    return list(start), total


def _step(lib, n=3, chunks=5, tables=None, ng=2, lr=(1e-4, 1e-5), wd=(1e-4, 0.0), b1=(0.9, 0.9), b2=(0.999, 0.999),
          eps=(1e-8, 1e-8), step=1, coef=P, hyper_null=None):
    t = dict(p=P, g=P, m=P, v=P, numel=P, start=P, group=P, offset=P)
    t.update(tables or {})
    cols = dict(lr=_doubles(lr), wd=_doubles(wd), b1=_doubles(b1), b2=_doubles(b2), eps=_doubles(eps))
    if hyper_null:
        cols[hyper_null] = None
    return lib.msda_adamw_step_f32(n, chunks, t["p"], t["g"], t["m"], t["v"], t["numel"], t["start"], t["group"], t["offset"], ng,
                                   cols["lr"], cols["wd"], cols["b1"], cols["b2"], cols["eps"], step, coef, None)


def test_entries_exported_abi_unchanged(lib):
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def test_supported_limits_at_their_edges(lib):
    ok = lib.msda_optim_supported
    assert ok(0, 1) == 1 and ok(1, 1) == 1 and ok(1 << 20, 8) == 1 and ok(700, 3) == 1
    assert ok(-1, 1) == 0 and ok((1 << 20) + 1, 1) == 0 and ok(1, 0) == 0 and ok(1, 9) == 0 and ok(1, -1) == 0


def test_chunks_at_the_sizes_around_a_chunk(lib):
    c = lib.msda_optim_chunk_elems()
    assert c > 0 and c % 4 == 0
    for numel, want in ((0, 0), (1, 1), (c - 1, 1), (c, 1), (c + 1, 2), (2 * c + 5, 3)):
        assert _chunks(lib, [numel]) == ([0, want], want), numel
    start, total = _chunks(lib, [0, 1, c - 1, c, c + 1, 2 * c + 5, 0])
    assert start == [0, 0, 1, 2, 3, 5, 8, 8] and total == 8          # an empty tensor owns no chunk, wherever it stands
    assert _chunks(lib, []) == ([0], 0) and _err(lib) == ""


def test_chunks_argument_errors(lib):
    one = ctypes.cast((ctypes.c_longlong * 1)(5), V)
    out = ctypes.cast((ctypes.c_longlong * 2)(), V)
    assert lib.msda_optim_chunks(-1, one, out) == -1 and "msda_optim_supported" in _err(lib)
    assert lib.msda_optim_chunks(1, None, out) == -1 and "null" in _err(lib)
    assert lib.msda_optim_chunks(1, one, None) == -1
    assert _chunks(lib, [-1])[1] == -1 and "numel" in _err(lib)
    c = lib.msda_optim_chunk_elems()
    assert _chunks(lib, [(1 << 31) * c])[1] == -1 and "chunks" in _err(lib)      # 2^31 chunks: one too many
    assert _chunks(lib, [((1 << 31) - 1) * c])[1] == (1 << 31) - 1


def test_norm_and_scale_argument_errors(lib):
    n0 = lib.msda_launch_count()
    sumsq, finish, scale = lib.msda_grad_sumsq_f32, lib.msda_grad_norm_finish_f32, lib.msda_grad_scale_f32
    for k in range(4):                                               # each null table in turn
        args = [P, P, P, P]
        args[k] = None
        assert sumsq(3, 5, *args, None) == ERR_ARGUMENT and "null table" in _err(lib), k
        assert scale(3, 5, *args, None) == ERR_ARGUMENT and "null table" in _err(lib), k
    assert sumsq(-1, 5, P, P, P, P, None) == ERR_ARGUMENT and sumsq(3, -1, P, P, P, P, None) == ERR_ARGUMENT
    assert sumsq(3, 1 << 31, P, P, P, P, None) == ERR_ARGUMENT and sumsq((1 << 20) + 1, 5, P, P, P, P, None) == ERR_ARGUMENT
    assert scale(-1, 5, P, P, P, P, None) == ERR_ARGUMENT and scale(3, -1, P, P, P, P, None) == ERR_ARGUMENT
    assert finish(-1, P, 0.1, P, None) == ERR_ARGUMENT
    assert finish(5, None, 0.1, P, None) == ERR_ARGUMENT and "null" in _err(lib)
    assert finish(5, P, 0.1, None, None) == ERR_ARGUMENT
    assert finish(5, P, float("nan"), P, None) == ERR_ARGUMENT and "max_norm" in _err(lib)
    assert lib.msda_launch_count() == n0


def test_adamw_argument_errors(lib):
    n0 = lib.msda_launch_count()
    for name in ("p", "g", "m", "v", "numel", "start", "group", "offset"):
        assert _step(lib, tables={name: None}) == ERR_ARGUMENT and "null table" in _err(lib), name
    for name in ("lr", "wd", "b1", "b2", "eps"):
        assert _step(lib, hyper_null=name) == ERR_ARGUMENT and "null hyperparameter" in _err(lib), name
    assert _step(lib, n=-1) == ERR_ARGUMENT and "msda_optim_supported" in _err(lib)
    assert _step(lib, chunks=-1) == ERR_ARGUMENT and _step(lib, chunks=1 << 31) == ERR_ARGUMENT
    nine = (1e-4,) * 9
    assert _step(lib, ng=9, lr=nine, wd=nine, b1=(0.9,) * 9, b2=(0.999,) * 9, eps=nine) == ERR_ARGUMENT
    assert _step(lib, ng=0) == ERR_ARGUMENT
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert _step(lib, b1=(0.9, bad)) == ERR_ARGUMENT and "betas" in _err(lib), bad
        assert _step(lib, b2=(bad, 0.999)) == ERR_ARGUMENT and "betas" in _err(lib), bad
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert _step(lib, lr=(1e-4, bad)) == ERR_ARGUMENT and "finite" in _err(lib), bad
        assert _step(lib, eps=(bad, 1e-8)) == ERR_ARGUMENT and "finite" in _err(lib), bad
    assert _step(lib, step=0) == ERR_ARGUMENT and "global_step" in _err(lib)
    assert _step(lib, step=-3) == ERR_ARGUMENT
    assert lib.msda_launch_count() == n0


def test_an_empty_list_launches_nothing(lib):
    n0 = lib.msda_launch_count()
    none = dict.fromkeys(("p", "g", "m", "v", "numel", "start", "group", "offset"))
    assert lib.msda_grad_sumsq_f32(0, 0, None, None, None, None, None) == 0 and _err(lib) == ""
    assert lib.msda_grad_norm_finish_f32(0, None, 0.1, None, None) == 0 and _err(lib) == ""
    assert lib.msda_grad_scale_f32(0, 0, None, None, None, None, None) == 0 and _err(lib) == ""
    assert _step(lib, n=0, chunks=0, tables=none, coef=None) == 0 and _err(lib) == ""
    # tensors that are all empty own no chunk either
    assert lib.msda_grad_sumsq_f32(4, 0, None, None, None, None, None) == 0
    assert _step(lib, n=4, chunks=0, tables=none, coef=None) == 0
    assert lib.msda_launch_count() == n0
