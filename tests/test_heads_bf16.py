"""Host side of the bf16-autocast DETR heads (MSDA_HEADS_BF16, functions/heads_func.py): the knob is read at call time, CPU
tensors keep the composition whatever it says, and the four C entries are declared in the binding's table.  No GPU."""
import ctypes

import pytest
import torch

from uvhand_amd import _native
from uvhand_amd.functions import heads_func
from uvhand_amd.functions.heads_func import ARCTIC, ASSEMBLY, detr_heads, detr_heads_reference
from uvhand_amd.modules.detr import MLP

NAMES = ("msda_heads_bf16_supported", "msda_heads_bf16_workspace_bytes", "msda_heads_forward_bf16", "msda_heads_backward_bf16")


def _heads(kind, L=2, B=2, Q=5, C=16, K=4, R=42):
    torch.manual_seed(0)
    cls = torch.nn.ModuleList(torch.nn.Linear(C, K) for _ in range(L))
    heads = [torch.nn.ModuleList(MLP(C, C, 42 if kind == ARCTIC else 63, 3) for _ in range(L))
             for _ in range(2 if kind == ARCTIC else 1)]
    shared = [torch.nn.Linear(C, w) for w in _native.HEADS_SHARED_WIDTHS] if kind == ARCTIC else None
    return torch.randn(L, B, Q, C), torch.rand(B, Q, R), torch.rand(L, B, Q, R), cls, heads, shared


def test_the_knob_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv("MSDA_HEADS_BF16", raising=False)
    assert not heads_func._bf16_enabled()                               # off by default
    monkeypatch.setenv("MSDA_HEADS_BF16", "1")
    assert heads_func._bf16_enabled()
    monkeypatch.setenv("MSDA_HEADS_BF16", "0")
    assert not heads_func._bf16_enabled()


@pytest.mark.parametrize("kind", [ARCTIC, ASSEMBLY])
@pytest.mark.parametrize("amp", [False, True])
def test_cpu_tensors_keep_the_composition(kind, amp, monkeypatch):
    monkeypatch.setenv("MSDA_HEADS_BF16", "1")
    args = _heads(kind)
    assert heads_func._fused_plan(kind, args[0], args[1], args[2], args[3], list(args[4]), args[5]) is None
    n0 = _native.launch_count()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=amp):
        logits, keys, outs = detr_heads(kind, *args)
        r_logits, r_keys, r_outs = detr_heads_reference(kind, *args)
    assert _native.launch_count() == n0
    got, want = [logits] + keys + outs, [r_logits] + r_keys + r_outs
    assert len(got) == len(want) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got, want))


def test_the_entries_are_declared_and_exported():
    for name in NAMES:
        assert name in _native.SIGNATURES
    assert _native.SIGNATURES["msda_heads_forward_bf16"] == _native.SIGNATURES["msda_heads_forward_f32"]
    assert _native.SIGNATURES["msda_heads_backward_bf16"] == _native.SIGNATURES["msda_heads_backward_f32"]
    lib = _native.load()
    for name in NAMES:
        assert hasattr(lib, name)
    for fn in (_native.heads_bf16_supported, _native.heads_forward_bf16, _native.heads_backward_bf16):
        assert callable(fn)


def test_widths_workspace_and_argument_errors_need_no_gpu():
    """Host logic only: the widths the form takes, its workspace (bf16 hidden gradients: smaller than the fp32 form's), and
    argument errors that come back before anything is launched."""
    lib = _native.load()
    assert [_native.heads_bf16_supported(c) for c in (0, 4, 8, 36, 40, 256, 4096, 4104)] == [False, False, True, False, True, True,
                                                                                          True, False]
    geom = (0, 6, 9600, 256, 14, 2, 0)
    bf, f32 = lib.msda_heads_bf16_workspace_bytes(*geom), lib.msda_heads_workspace_bytes(*geom)
    hidden_grads = 2 * 2 * 6 * 9600 * 256
    assert f32 - bf == hidden_grads * 2 and bf > hidden_grads * 2       # the same partials behind half the bytes
    assert lib.msda_heads_bf16_workspace_bytes(0, 9, 100, 256, 14, 2, 0) == 0
    P = (ctypes.c_void_p * 8)()
    rc = lib.msda_heads_forward_bf16(0, 1, 40, 36, 14, 0, 42, 0, None, None, None, P, P, None, None, P, P, None, None, P, None,
                                     None, None)
    assert rc == 1 and b"C % 8" in lib.msda_last_error()
    rc = lib.msda_heads_forward_bf16(0, 1, 40, 256, 14, 0, 42, 0, None, None, None, P, P, None, None, P, P, None, None, P, None,
                                     None, None)
    assert rc == 1 and b"null pointer" in lib.msda_last_error()
