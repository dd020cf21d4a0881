"""C ABI of the DINO query-selection entries (csrc/msda_dino_select.hip; added without an ABI version bump): the symbols are
exported, they are in the binding's table, msda_dino_select_supported holds at the envelope's edges, the workspace size is a
host function, and argument errors come back as codes from the host-side checks, before anything is launched — so no GPU is
needed, and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

P = 0x10000                      # 16-byte aligned fake device address, only passed next to an argument the checks refuse
ERR_ARGUMENT = 1

NEW_ENTRIES = ("msda_dino_select_supported", "msda_dino_select_workspace_bytes", "msda_dino_select_forward_f32",
               "msda_dino_select_backward_f32")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _err(lib):
    return lib.msda_last_error().decode()


def test_entries_exported_and_in_table(lib):
    from uvhand_amd import _native
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    for name in ("dino_select_supported", "dino_select_workspace_bytes", "dino_select_forward", "dino_select_backward"):
        assert callable(getattr(_native, name)), name
    assert lib.msda_version() == 116


def test_supported_at_the_envelope_edges(lib):
    ok = lib.msda_dino_select_supported                  # (S, K, Q, C)
    assert ok(12276, 14, 900, 256) == 1
    assert ok(100, 14, 0, 256) == 0                      # Q = 0
    assert ok(100, 14, 100, 256) == 1                    # Q = S
    assert ok(100, 14, 101, 256) == 0                    # Q = S + 1
    assert ok(1, 1, 1, 4) == 1
    assert ok(0, 14, 0, 256) == 0
    assert ok(4096, 14, 2048, 256) == 1                  # Q = 2048
    assert ok(4096, 14, 2049, 256) == 0
    assert ok(2048, 14, 2048, 256) == 1
    assert ok(1 << 20, 14, 900, 256) == 1                # S = 2^20
    assert ok((1 << 20) + 1, 14, 900, 256) == 0
    assert ok(100, 0, 7, 256) == 0                       # K = 0
    assert ok(100, 256, 7, 256) == 1
    assert ok(100, 257, 7, 256) == 0
    assert ok(100, 14, 7, 2) == 0                        # C = 2
    assert ok(100, 14, 7, 4) == 1
    assert ok(100, 14, 7, 6) == 0                        # not a multiple of 4
    assert ok(100, 14, 7, 2048) == 1
    assert ok(100, 14, 7, 2052) == 0
    assert ok(100, 14, -1, 256) == 0 and ok(-5, 14, 1, 256) == 0


def test_workspace_is_a_host_function_of_n_and_s(lib):
    ws = lib.msda_dino_select_workspace_bytes
    assert ws(0, 100) == 0 and ws(3, 0) == 0 and ws(-1, 5) == 0
    for N, S in ((1, 1), (2, 43), (8, 12276), (32, 1045), (1, 1 << 20)):
        b = ws(N, S)
        assert b >= N * S * 9, (N, S, b)                 # a 64-bit key and a code byte per row
        assert b <= N * S * 9 + 16 and b == ws(N, S)
    assert ws(2, 43) < ws(2, 44) < ws(3, 44)


def test_forward_argument_errors(lib):
    fn = lib.msda_dino_select_forward_f32   # cls, memory, proposals, N, S, K, Q, C, hand0, hand1, topk, slot, tgt, prop_sel, code, ws
    good = [P, P, P, 2, 100, 14, 7, 256, 12, 13, P, P, P, P, P, P, None]

    def call(**kw):
        a = list(good)
        names = ["cls", "memory", "proposals", "N", "S", "K", "Q", "C", "h0", "h1", "topk", "slot", "tgt", "prop_sel", "code", "ws"]
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    assert call(Q=101) == ERR_ARGUMENT
    assert "out of range" in _err(lib)
    for bad in (dict(Q=0), dict(Q=2049, S=4096), dict(S=(1 << 20) + 1), dict(S=0, Q=0), dict(K=0), dict(K=257), dict(C=2), dict(C=6),
                dict(C=2052), dict(N=-1), dict(N=65536)):
        assert call(**bad) == ERR_ARGUMENT, bad
    assert call(N=4096, S=1 << 20) == ERR_ARGUMENT                       # beyond 2^31 elements
    assert "2^31" in _err(lib)
    for name in ("cls", "memory", "proposals", "topk", "slot", "tgt", "prop_sel", "code", "ws"):
        assert call(**{name: None}) == ERR_ARGUMENT, name
        assert "null" in _err(lib)
    for name in ("memory", "tgt", "ws"):
        assert call(**{name: P + 4}) == ERR_ARGUMENT, name
        assert "aligned" in _err(lib)
    assert fn(None, None, None, 0, 100, 14, 7, 256, 12, 13, None, None, None, None, None, None, None) == 0    # N == 0


def test_backward_argument_errors(lib):
    fn = lib.msda_dino_select_backward_f32                               # slot, grad_tgt, N, S, Q, C, grad_memory
    assert fn(P, P, 2, 100, 101, 256, P, None) == ERR_ARGUMENT           # Q > S
    assert fn(P, P, 2, 100, 0, 256, P, None) == ERR_ARGUMENT
    assert fn(P, P, 2, 100, 7, 6, P, None) == ERR_ARGUMENT
    assert fn(P, P, 2, 100, 7, 2052, P, None) == ERR_ARGUMENT
    assert fn(P, P, -1, 100, 7, 256, P, None) == ERR_ARGUMENT
    assert fn(P, P, 4096, 1 << 20, 7, 256, P, None) == ERR_ARGUMENT
    assert "2^31" in _err(lib)
    assert fn(None, P, 2, 100, 7, 256, P, None) == ERR_ARGUMENT
    assert "null" in _err(lib)
    assert fn(P, None, 2, 100, 7, 256, P, None) == ERR_ARGUMENT
    assert fn(P, P, 2, 100, 7, 256, None, None) == ERR_ARGUMENT
    assert fn(P, P + 8, 2, 100, 7, 256, P, None) == ERR_ARGUMENT
    assert "aligned" in _err(lib)
    assert fn(P, P, 2, 100, 7, 256, P + 4, None) == ERR_ARGUMENT
    assert fn(None, None, 0, 100, 7, 256, None, None) == 0               # N == 0


def test_wrappers_refuse_before_launch():
    import torch
    from uvhand_amd import _native
    with pytest.raises(RuntimeError):
        _native.dino_select_forward(torch.zeros(2, 10, 14), torch.zeros(2, 10, 8), torch.zeros(2, 10, 42), 3)
    with pytest.raises(RuntimeError):
        _native.dino_select_backward(torch.zeros(2, 10, dtype=torch.int32), torch.zeros(2, 3, 8))
