"""C ABI of the bf16 form of the masked, long-sequence attention core (msda_attn32x_*_bf16, include/msda.h).  No GPU: every call
here fails its host-side checks, which come before any launch, so fake device addresses never reach a kernel."""
import ctypes

import pytest

OK_PTR = 0x10000                 # 16-byte aligned; only ever passed next to an argument the checks refuse

NEW_ENTRIES = ("msda_attn32x_forward_bf16", "msda_attn32x_backward_bf16")


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


def test_library_exports_and_binds_the_bf16_long_entries_at_abi_116(lib):
    from uvhand_amd import _native
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    # the argument lists are the fp32 entries'
    assert _native.SIGNATURES["msda_attn32x_forward_bf16"] == _native.SIGNATURES["msda_attn32x_forward_f32"]
    assert _native.SIGNATURES["msda_attn32x_backward_bf16"] == _native.SIGNATURES["msda_attn32x_backward_f32"]
    assert lib.msda_version() == 116


def test_forward_argument_errors_launch_nothing(lib):
    fn = lib.msda_attn32x_forward_bf16
    t = [OK_PTR, 256, 256]
    before = lib.msda_launch_count()

    def call(q=t, k=t, v=t, Lq=1098, Lk=1098, p=0.0, seed=None, mask=None, sq=0, o=t, lse=OK_PTR):
        return fn(*q, *k, *v, 2, 8, Lq, Lk, 0.17, p, seed, mask, sq, *o, lse, None)
    for kw in ({"Lq": 0}, {"Lk": 0}, {"Lq": 2049}, {"Lk": 2049}):                         # lengths outside the envelope
        assert call(**kw) == 1, kw
        assert b"2048" in lib.msda_last_error() and b"forward_bf16" in lib.msda_last_error()
    assert call(p=0.1) == 1                                                               # dropout without a seed
    assert b"seed" in lib.msda_last_error()
    assert call(p=1.0, seed=OK_PTR) == 1 and call(p=-0.1, seed=OK_PTR) == 1               # p >= 1, p < 0
    assert b"p < 1" in lib.msda_last_error()
    assert call(mask=OK_PTR, sq=1097) == 1                                                # mask rows shorter than Lk
    assert b"mask_sq" in lib.msda_last_error()
    for name in ("q", "k", "v", "o"):
        assert call(**{name: [OK_PTR + 8, 256, 256]}) == 1, name                          # a base off by 8 bytes
        assert b"aligned" in lib.msda_last_error()
        assert call(**{name: [OK_PTR, 256, 260]}) == 1, name                              # a multiple of 4, not of 8
        assert b"multiples of 8" in lib.msda_last_error()
        assert call(**{name: [OK_PTR, 260, 256]}) == 1, name
        assert call(**{name: [None, 256, 256]}) == 1, name
    assert call(lse=None) == 1
    assert lib.msda_launch_count() == before


def test_backward_argument_errors_launch_nothing(lib):
    fn = lib.msda_attn32x_backward_bf16
    t = [OK_PTR, 256, 256]
    before = lib.msda_launch_count()

    def call(Lq=1098, Lk=1098, p=0.0, seed=None, mask=None, sq=0, views=None, lse=OK_PTR):
        v = views or [t] * 8
        return fn(*v[0], *v[1], *v[2], *v[3], lse, *v[4], 2, 8, Lq, Lk, 0.17, p, seed, mask, sq, *v[5], *v[6], *v[7], None)
    for kw in ({"Lq": 0}, {"Lk": 0}, {"Lq": 2049}, {"Lk": 2049}):
        assert call(**kw) == 1, kw
        assert b"2048" in lib.msda_last_error() and b"backward_bf16" in lib.msda_last_error()
    assert call(p=0.2) == 1
    assert b"seed" in lib.msda_last_error()
    assert call(p=1.0, seed=OK_PTR) == 1 and call(p=-0.5, seed=OK_PTR) == 1
    assert b"p < 1" in lib.msda_last_error()
    assert call(mask=OK_PTR, sq=100) == 1
    assert b"mask_sq" in lib.msda_last_error()
    assert call(lse=None) == 1
    assert b"lse" in lib.msda_last_error()
    for i in range(8):                                                                    # each view: stride / base
        views = [t] * 8
        views[i] = [OK_PTR, 256, 260]
        assert call(views=views) == 1, i
        assert b"multiples of 8" in lib.msda_last_error()
        views[i] = [OK_PTR, 260, 256]
        assert call(views=views) == 1, i
        views[i] = [OK_PTR + 8, 256, 256]
        assert call(views=views) == 1, i
        assert b"aligned" in lib.msda_last_error()
    assert lib.msda_launch_count() == before
