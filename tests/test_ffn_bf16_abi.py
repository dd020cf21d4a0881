"""C ABI of the bf16-autocast FFN entries (csrc/msda_ffn_bf16.hip; added without an ABI version bump): the symbols are exported,
the envelope is what include/msda.h says on each side of every bound, the workspace grows with the rows, and argument errors
come back as codes from the host-side checks before anything is launched (msda_launch_count unchanged) — so no GPU is needed,
and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

P = 0x10000
ERR_ARGUMENT = 1
NAMES = ("msda_ffn_bf16_supported", "msda_ffn_bf16_workspace_bytes", "msda_ffn_forward_bf16", "msda_ffn_backward_bf16")

SIZES = "msda_ffn_bf16: need C % 64 == 0, 64 <= C <= 256 and F % 64 == 0, 64 <= F <= 8192"
ROWS = "msda_ffn_bf16: need M >= 1"
BIG = "msda_ffn_bf16: tensors beyond 2^31 elements (M * F)"
PROB = "msda_ffn_bf16: need a dropout probability 0 <= p < 1"
NULL = "msda_ffn_bf16: null pointer"
SEED = "msda_ffn_bf16: dropout (p > 0) needs a device seed"
ALIGN_F = "msda_ffn_bf16: x, xb, a, y and the weights must be 16-byte aligned"
ALIGN_B = "msda_ffn_bf16: grad_out, xb, a, grad_x, the weights and the workspace must be 16-byte aligned"
BIAS = "msda_ffn_bf16: a bias gradient comes with its weight gradient (null pointer)"
WS_SMALL = "msda_ffn_bf16: workspace smaller than msda_ffn_bf16_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _err(lib):
    return lib.msda_last_error().decode()


def _fwd(lib, M=130, C=256, F=1024, x=P, x_bf16=0, w1=P, b1=P, w2=P, b2=P, p=0.0, seed=None, xb=P, a=P, y=P):
    return lib.msda_ffn_forward_bf16(M, C, F, x, x_bf16, w1, b1, w2, b2, p, seed, xb, a, y, None)


def _bwd(lib, M=130, C=256, F=1024, go=P, xb=P, a=P, w1=P, w2=P, p=0.0, gx=P, gx_bf16=0, gw1=P, gb1=P, gw2=P, gb2=P, ws=P,
         ws_bytes=1 << 40):
    return lib.msda_ffn_backward_bf16(M, C, F, go, xb, a, w1, w2, p, gx, gx_bf16, gw1, gb1, gw2, gb2, ws, ws_bytes, None)


def test_entries_exported_abi_unchanged(lib):
    for name in NAMES:
        assert hasattr(lib, name)
    assert lib.msda_version() == 116


def test_supported_on_each_side_of_every_bound(lib):
    sup = lib.msda_ffn_bf16_supported
    for C, want in ((64, 1), (256, 1), (128, 1), (192, 1), (320, 0), (72, 0), (0, 0), (-64, 0)):
        assert sup(C, 1024) == want, C
    for F, want in ((64, 1), (8192, 1), (2048, 1), (8256, 0), (72, 0), (0, 0)):
        assert sup(256, F) == want, F
    assert sup(256, 1024) == 1 and sup(256, 2048) == 1                  # the reference's two settings


def test_workspace_grows_with_rows_and_is_zero_for_refused_sizes(lib):
    ws = lib.msda_ffn_bf16_workspace_bytes
    small, big = ws(130, 256, 1024), ws(33440, 256, 1024)
    assert 130 * 1024 * 2 <= small < big                                # gh alone is M * F bf16
    assert ws(131, 256, 1024) >= small
    for geom in ((130, 320, 1024), (130, 72, 1024), (130, 256, 8256), (130, 256, 72), (0, 256, 1024), (1 << 21, 256, 1024)):
        assert ws(*geom) == 0, geom


BAD_FORWARD = [
    (dict(C=320), SIZES), (dict(C=72), SIZES), (dict(C=0), SIZES), (dict(F=8256), SIZES), (dict(F=72), SIZES),
    (dict(M=0), ROWS), (dict(M=-1), ROWS), (dict(M=1 << 21), BIG), (dict(M=1 << 18, F=8192), BIG),
    (dict(p=1.0, seed=P), PROB), (dict(p=-0.1, seed=P), PROB), (dict(p=float("nan"), seed=P), PROB),
    (dict(x=None), NULL), (dict(w1=None), NULL), (dict(b1=None), NULL), (dict(w2=None), NULL), (dict(b2=None), NULL),
    (dict(a=None), NULL), (dict(y=None), NULL), (dict(xb=None), NULL),
    (dict(p=0.1), SEED), (dict(p=0.5, seed=None), SEED),
    (dict(x=P + 4), ALIGN_F), (dict(x=P + 8, x_bf16=1, xb=None), ALIGN_F), (dict(w1=P + 4), ALIGN_F), (dict(w2=P + 8), ALIGN_F),
    (dict(a=P + 2), ALIGN_F), (dict(y=P + 8), ALIGN_F), (dict(xb=P + 8), ALIGN_F),
]
BAD_BACKWARD = [
    (dict(C=320), SIZES), (dict(F=72), SIZES), (dict(M=0), ROWS), (dict(M=1 << 21), BIG), (dict(p=1.0), PROB), (dict(p=-1.0), PROB),
    (dict(go=None), NULL), (dict(xb=None), NULL), (dict(a=None), NULL), (dict(w1=None), NULL), (dict(w2=None), NULL),
    (dict(ws=None), NULL), (dict(gw1=None), BIAS), (dict(gw2=None), BIAS),
    (dict(go=P + 8), ALIGN_B), (dict(xb=P + 2), ALIGN_B), (dict(a=P + 4), ALIGN_B), (dict(w1=P + 4), ALIGN_B),
    (dict(w2=P + 12), ALIGN_B), (dict(gx=P + 4), ALIGN_B), (dict(ws=P + 8), ALIGN_B),
    (dict(ws_bytes=0), WS_SMALL), (dict(ws_bytes=130 * 1024 * 2 - 1), WS_SMALL),
]


def test_forward_argument_errors(lib):
    n0 = lib.msda_launch_count()
    for kw, message in BAD_FORWARD:
        assert _fwd(lib, **kw) == ERR_ARGUMENT and _err(lib) == message, kw
    assert lib.msda_launch_count() == n0


def test_backward_argument_errors(lib):
    n0 = lib.msda_launch_count()
    for kw, message in BAD_BACKWARD:
        assert _bwd(lib, **kw) == ERR_ARGUMENT and _err(lib) == message, kw
    need = lib.msda_ffn_bf16_workspace_bytes(130, 256, 1024)
    assert _bwd(lib, ws_bytes=need - 1) == ERR_ARGUMENT and _err(lib) == WS_SMALL
    assert lib.msda_launch_count() == n0


def test_every_message_names_the_entry_family():
    for message in (SIZES, ROWS, BIG, PROB, NULL, SEED, ALIGN_F, ALIGN_B, BIAS, WS_SMALL):
        assert message.startswith("msda_ffn_bf16")


def test_a_bf16_x_needs_no_xb(lib):
    """x_is_bf16 with a null xb passes the null check (it then fails on the next one asked for here: the seed)."""
    assert _fwd(lib, x_bf16=1, xb=None, p=0.5) == ERR_ARGUMENT and _err(lib) == SEED
