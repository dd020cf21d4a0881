"""C ABI of the bf16-autocast forms (ABI 116): the bf16 attention core (msda_attn32_*_bf16) and the add + LayerNorm with an fp32
x and a bf16 residual (msda_add_layernorm_*_f32_bf16res).  No GPU: every call here fails its host-side checks, which come before
any launch, so fake device addresses never reach a kernel."""
import ctypes

import pytest

OK_PTR = 0x10000                 # 16-byte aligned; only ever passed next to an argument the checks refuse

NEW_ENTRIES = ("msda_attn32_forward_bf16", "msda_attn32_backward_bf16", "msda_add_layernorm_forward_f32_bf16res",
               "msda_add_layernorm_backward_f32_bf16res")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    handle = _native.declare(ctypes.CDLL(_native.LIB_PATH))
    yield handle
    # leave no error text behind for later tests in this process: an empty problem passes every check and launches nothing
    fn = handle.msda_add_layernorm_forward_f32_bf16res
    assert fn(None, None, None, None, 0, 256, 1e-5, None, None, None, None) == 0
    assert handle.msda_last_error() == b""


def test_library_exports_the_bf16_entries_at_abi_116(lib):
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.msda_version() == 116


def _fwd(lib):
    return lib.msda_attn32_forward_bf16


def _bwd(lib):
    return lib.msda_attn32_backward_bf16


def test_attention_bf16_forward_argument_errors(lib):
    fn = _fwd(lib)
    t = [OK_PTR, 256, 256]
    seed = OK_PTR
    assert fn(*(t * 3), 2, 8, 400, 300, 0.17, 0.0, None, *t, OK_PTR, None) == 1          # too long
    assert b"320" in lib.msda_last_error()
    assert fn(*(t * 3), 2, 8, 300, 321, 0.17, 0.0, None, *t, OK_PTR, None) == 1
    assert fn(*(t * 3), 2, 8, 0, 300, 0.17, 0.0, None, *t, OK_PTR, None) == 1             # empty
    assert fn(*(t * 3), 2, 8, 300, 300, 0.17, 0.1, None, *t, OK_PTR, None) == 1           # dropout without a seed
    assert b"seed" in lib.msda_last_error()
    assert fn(*(t * 3), 2, 8, 300, 300, 0.17, 1.0, seed, *t, OK_PTR, None) == 1           # p = 1
    assert fn(*(t * 3), 2, 8, 300, 300, 0.17, -0.1, seed, *t, OK_PTR, None) == 1          # p < 0
    assert fn(*([None, 256, 256] * 3), 2, 8, 300, 300, 0.17, 0.0, None, None, 256, 256, None, None) == 1   # null tensors
    assert b"aligned" in lib.msda_last_error()
    assert fn(*(t * 3), 2, 8, 300, 300, 0.17, 0.0, None, *t, None, None) == 1              # null lse
    # strides count bf16 elements and must be multiples of 8 (4 is enough for the fp32 entries); bases 16-byte aligned
    assert fn(OK_PTR, 256, 260, *(t * 2), 2, 8, 300, 300, 0.17, 0.0, None, *t, OK_PTR, None) == 1
    assert b"multiples of 8" in lib.msda_last_error()
    assert fn(*(t * 2), OK_PTR, 252, 256, 2, 8, 300, 300, 0.17, 0.0, None, *t, OK_PTR, None) == 1
    assert fn(OK_PTR + 8, 256, 256, *(t * 2), 2, 8, 300, 300, 0.17, 0.0, None, *t, OK_PTR, None) == 1
    assert fn(*(t * 3), 2, 8, 300, 300, 0.17, 0.0, None, OK_PTR, 256, 4, OK_PTR, None) == 1


def test_attention_bf16_backward_argument_errors(lib):
    fn = _bwd(lib)
    t = [OK_PTR, 256, 256]

    def call(Lq=300, Lk=300, p=0.0, seed=None, views=None, lse=OK_PTR):
        v = views or [t] * 8
        return fn(*v[0], *v[1], *v[2], *v[3], lse, *v[4], 2, 8, Lq, Lk, 0.17, p, seed, *v[5], *v[6], *v[7], None)
    assert call(Lq=321) == 1
    assert b"320" in lib.msda_last_error()
    assert call(Lk=0) == 1
    assert call(p=0.2) == 1                                                               # dropout without a seed
    assert b"seed" in lib.msda_last_error()
    assert call(p=1.0, seed=OK_PTR) == 1
    assert call(views=[[None, 256, 256]] * 8) == 1                                        # null tensors
    assert b"aligned" in lib.msda_last_error()
    assert call(lse=None) == 1
    for i in range(8):                                                                    # each view: misaligned stride / base
        views = [t] * 8
        views[i] = [OK_PTR, 256, 260]
        assert call(views=views) == 1
        views[i] = [OK_PTR + 2, 256, 256]
        assert call(views=views) == 1


def test_add_layernorm_bf16res_argument_errors(lib):
    fwd = lib.msda_add_layernorm_forward_f32_bf16res
    assert fwd(None, None, None, None, 4, 6, 1e-5, None, None, None, None) == 1            # width not a multiple of 4
    assert b"multiple of 4" in lib.msda_last_error()
    assert fwd(None, None, None, None, 4, 2048, 1e-5, None, None, None, None) == 1
    assert fwd(None, None, None, None, 4, 256, 1e-5, None, None, None, None) == 1          # null pointers with rows > 0
    p = OK_PTR
    assert fwd(p, None, p, p, 4, 256, 1e-5, p, p, p, None) == 1                            # the bf16 residual is required
    assert b"residual" in lib.msda_last_error()
    assert fwd(p, p + 4, p, p, 4, 256, 1e-5, p, p, p, None) == 1                           # residual not 8-byte aligned
    assert fwd(p, p, p, p, 4, 256, 1e-5, p, None, p, None) == 1                            # null mean
    assert fwd(p + 8, p, p, p, 4, 256, 1e-5, p, p, p, None) == 1                           # x not 16-byte aligned
    bwd = lib.msda_add_layernorm_backward_f32_bf16res
    assert bwd(None, None, None, None, None, None, 4, 6, None, None, None, None, None, None) == 1
    assert b"multiple of 4" in lib.msda_last_error()
    assert bwd(p, p, p, p, p, p, 4, 256, p, None, p, p, p, None) == 1                       # no bf16 gradient for the residual
    assert b"grad_residual" in lib.msda_last_error()
    assert bwd(p, p, None, p, p, p, 4, 256, p, p, p, p, p, None) == 1                       # no residual
    assert bwd(p, p, p, p, p, p, 4, 256, p, p + 2, p, p, p, None) == 1                      # misaligned grad_residual
    assert bwd(p, p, p, p, p, p, 4, 256, p, p, None, p, p, None) == 1                       # no grad_gamma
    assert bwd(p, p, p, p, p, p, 4, 256, p, p, p, p, None, None) == 1                       # no workspace
