"""One table of refusals for the eight C entries of the decoder self-attention cores (msda_attn32_* and msda_attn32x_*, fp32 and
bf16, forward and backward): they share one host checker (csrc/msda_attn_args.h), so every entry answers every bad argument
the same way — return code MSDA_ERR_ARGUMENT, a message that names the entry and the condition, and no launch.  No GPU: every
call here fails its host-side checks, which come before any launch, so fake device addresses never reach a kernel."""
import ctypes

import pytest

OK_PTR = 0x10000                 # 16-byte aligned; only ever passed next to an argument the checks refuse
MSDA_ERR_ARGUMENT = 1

# entry -> (family's longest sequence, elements in 16 bytes, takes a mask, number of views)
ENTRIES = {
    "msda_attn32_forward_f32": (320, 4, False, 4),
    "msda_attn32_backward_f32": (320, 4, False, 8),
    "msda_attn32_forward_bf16": (320, 8, False, 4),
    "msda_attn32_backward_bf16": (320, 8, False, 8),
    "msda_attn32x_forward_f32": (2048, 4, True, 4),
    "msda_attn32x_backward_f32": (2048, 4, True, 8),
    "msda_attn32x_forward_bf16": (2048, 8, True, 4),
    "msda_attn32x_backward_bf16": (2048, 8, True, 8),
}
CASES = ("Lq past the bound", "Lk past the bound", "Lq = 0", "dropout without a seed", "p = 1", "p < 0", "mask rows shorter than Lk",
         "misaligned base", "stride off the 16-byte grid", "null lse", "too many workgroups")


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


def _call(lib, entry, N=2, H=8, Lq=None, Lk=None, p=0.0, seed=None, mask=None, sq=0, views=None, lse=OK_PTR):
    """The entry with good arguments (fake 16-byte aligned addresses) except the ones given; views: q, k, v, out (backward:
    + grad_out, grad_q, grad_k, grad_v), each [pointer, batch stride, sequence stride]."""
    bound, _, masked, nviews = ENTRIES[entry]
    L = 300 if bound == 320 else 1098
    Lq, Lk = L if Lq is None else Lq, L if Lk is None else Lk
    v = views or [[OK_PTR, 256, 256]] * nviews
    tail = [N, H, Lq, Lk, 0.17, p, seed] + ([mask, sq] if masked else [])
    if nviews == 4:
        return getattr(lib, entry)(*v[0], *v[1], *v[2], *tail, *v[3], lse, None)
    return getattr(lib, entry)(*v[0], *v[1], *v[2], *v[3], lse, *v[4], *tail, *v[5], *v[6], *v[7], None)


@pytest.mark.parametrize("entry,case", [(e, c) for e in sorted(ENTRIES) for c in CASES
                                        if ENTRIES[e][2] or c != "mask rows shorter than Lk"])     # (the resident entries take no mask)
def test_every_entry_refuses_the_same_table(lib, entry, case):
    bound, per16, _, nviews = ENTRIES[entry]
    good = [OK_PTR, 256, 256]
    one_bad_view = lambda bad: [[good] * i + [bad] + [good] * (nviews - 1 - i) for i in range(nviews)]
    # case -> (the calls' arguments, the substrings of the message)
    table = {
        "Lq past the bound": ([dict(Lq=bound + 1)], [b"%d" % bound, b"head_dim 32"]),
        "Lk past the bound": ([dict(Lk=bound + 1)], [b"%d" % bound, b"head_dim 32"]),
        "Lq = 0": ([dict(Lq=0)], [b"%d" % bound, b"head_dim 32"]),
        "dropout without a seed": ([dict(p=0.1)], [b"seed"]),
        "p = 1": ([dict(p=1.0, seed=OK_PTR)], [b"p < 1"]),
        "p < 0": ([dict(p=-0.1, seed=OK_PTR)], [b"p < 1"]),
        "mask rows shorter than Lk": ([dict(mask=OK_PTR, sq=1097)], [b"mask_sq"]),
        "misaligned base": ([dict(views=v) for v in one_bad_view([OK_PTR + 8, 256, 256])], [b"aligned"]),
        "stride off the 16-byte grid": ([dict(views=v) for v in one_bad_view([OK_PTR, 256, 256 + per16 // 2])]
                                        + [dict(views=v) for v in one_bad_view([OK_PTR, 256 + per16 // 2, 256])],
                                        [b"aligned", b"multiples of %d" % per16]),
        "null lse": ([dict(lse=None)], [b"lse"]),
        # N * H * workgroups per pair > 2^31 - 1, with null views: nothing here can get as far as a launch
        "too many workgroups": ([dict(N=65536, H=65536, views=[[None, 256, 256]] * nviews, lse=None)], [b"pairs"]),
    }
    calls, substrings = table[case]
    before = lib.msda_launch_count()
    for kw in calls:
        assert _call(lib, entry, **kw) == MSDA_ERR_ARGUMENT, kw
        msg = lib.msda_last_error()
        assert entry.encode() in msg, (kw, msg)
        for sub in substrings:
            assert sub in msg, (kw, msg)
    assert lib.msda_launch_count() == before
