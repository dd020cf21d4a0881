"""C ABI of the masked, long-sequence attention core (msda_attn32x_*_f32, include/msda.h) and the contrastive-denoising mask
(uvhand_amd.utils.cdn_attention_mask).  No GPU: every call here fails its host-side checks, which come before any launch, so
fake device addresses never reach a kernel."""
import ctypes

import pytest
import torch

OK_PTR = 0x10000                 # 16-byte aligned; only ever passed next to an argument the checks refuse

NEW_ENTRIES = ("msda_attn32x_supported", "msda_attn32x_forward_f32", "msda_attn32x_backward_f32")


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


def test_library_exports_and_binds_the_long_entries_at_abi_116(lib):
    from uvhand_amd import _native
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    for name in ("attn32x_supported", "attn32x_forward", "attn32x_backward"):
        assert callable(getattr(_native, name))
    assert lib.msda_version() == 116


def test_supported_envelope(lib):
    assert lib.msda_attn32x_supported(2048, 2048, 32) == 1
    assert lib.msda_attn32x_supported(1, 1, 32) == 1 and lib.msda_attn32x_supported(1098, 1098, 32) == 1
    assert lib.msda_attn32x_supported(2049, 1, 32) == 0
    assert lib.msda_attn32x_supported(1, 0, 32) == 0
    assert lib.msda_attn32x_supported(8, 8, 64) == 0
    from uvhand_amd import _native
    assert _native.attn32x_supported(321, 321, 32) and not _native.attn32x_supported(1, 2049, 32)


def test_forward_argument_errors_launch_nothing(lib):
    fn = lib.msda_attn32x_forward_f32
    t = [OK_PTR, 256, 256]
    before = lib.msda_launch_count()

    def call(q=t, k=t, v=t, Lq=1098, Lk=1098, p=0.0, seed=None, mask=None, sq=0, o=t, lse=OK_PTR):
        return fn(*q, *k, *v, 2, 8, Lq, Lk, 0.17, p, seed, mask, sq, *o, lse, None)
    assert call(Lq=2049) == 1                                                             # lengths outside the envelope
    assert b"2048" in lib.msda_last_error()
    assert call(Lk=2049) == 1 and call(Lq=0) == 1 and call(Lk=0) == 1
    assert b"head_dim 32" in lib.msda_last_error()
    assert call(p=0.1) == 1                                                               # dropout without a seed
    assert b"seed" in lib.msda_last_error()
    assert call(p=1.0, seed=OK_PTR) == 1 and call(p=-0.1, seed=OK_PTR) == 1               # p >= 1, p < 0
    assert b"p < 1" in lib.msda_last_error()
    assert call(mask=OK_PTR, sq=1097) == 1                                                # mask rows shorter than Lk
    assert b"mask_sq" in lib.msda_last_error()
    assert call(q=[OK_PTR + 8, 256, 256]) == 1                                            # misaligned views
    assert b"aligned" in lib.msda_last_error()
    assert call(k=[OK_PTR, 256, 258]) == 1 and call(v=[OK_PTR, 254, 256]) == 1 and call(o=[None, 256, 256]) == 1
    assert call(lse=None) == 1
    assert lib.msda_launch_count() == before


def test_backward_argument_errors_launch_nothing(lib):
    fn = lib.msda_attn32x_backward_f32
    t = [OK_PTR, 256, 256]
    before = lib.msda_launch_count()

    def call(Lq=1098, Lk=1098, p=0.0, seed=None, mask=None, sq=0, views=None, lse=OK_PTR):
        v = views or [t] * 8
        return fn(*v[0], *v[1], *v[2], *v[3], lse, *v[4], 2, 8, Lq, Lk, 0.17, p, seed, mask, sq, *v[5], *v[6], *v[7], None)
    assert call(Lq=2049) == 1
    assert b"2048" in lib.msda_last_error()
    assert call(Lk=0) == 1
    assert call(p=0.2) == 1
    assert b"seed" in lib.msda_last_error()
    assert call(p=1.0, seed=OK_PTR) == 1
    assert call(mask=OK_PTR, sq=100) == 1
    assert b"mask_sq" in lib.msda_last_error()
    assert call(lse=None) == 1
    for i in range(8):                                                                    # each view: misaligned stride / base
        views = [t] * 8
        views[i] = [OK_PTR, 256, 258]
        assert call(views=views) == 1
        assert b"aligned" in lib.msda_last_error()
        views[i] = [OK_PTR + 4, 256, 256]
        assert call(views=views) == 1
    assert lib.msda_launch_count() == before


def _closed_form(single_pad, dn_number, num_queries):
    pad = 2 * single_pad * dn_number
    n = pad + num_queries
    return torch.tensor([[j < pad and (i >= pad or i // (2 * single_pad) != j // (2 * single_pad)) for j in range(n)]
                         for i in range(n)], dtype=torch.bool).reshape(n, n)


@pytest.mark.parametrize("single_pad,dn_number,num_queries", [(1, 1, 1), (3, 1, 5), (3, 2, 20), (2, 5, 7), (3, 33, 900)])
def test_cdn_attention_mask_equals_the_closed_form(single_pad, dn_number, num_queries):
    from uvhand_amd.utils import cdn_attention_mask
    m = cdn_attention_mask(single_pad, dn_number, num_queries, "cpu")
    n = 2 * single_pad * dn_number + num_queries
    assert m.dtype == torch.bool and tuple(m.shape) == (n, n)
    if n <= 64:                                          # (entry by entry in Python; the 1098-row case as tensor comparisons)
        assert torch.equal(m, _closed_form(single_pad, dn_number, num_queries))
    else:
        i, j, pad, g = torch.arange(n)[:, None], torch.arange(n)[None, :], 2 * single_pad * dn_number, 2 * single_pad
        assert torch.equal(m, (j < pad) & ((i >= pad) | (i // g != j // g)))
    if dn_number == 1:                                   # one group: no denoising row is hidden from another
        pad = 2 * single_pad
        assert not m[:pad].any()
