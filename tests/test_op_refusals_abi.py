"""One table of refusals and empty-problem answers for the 20 C entries of the sampling op (msda_forward_*, msda_backward_*,
their _ws_ and fused-prologue forms): they share four host bodies (csrc/msda_abi.hip over the records of csrc/msda_op_args.h),
so every entry answers every bad argument the same way.  The expected messages are whole strings, as the library returned
them before the entries were put behind those bodies.  No GPU: every call here is refused, or returns for an empty problem,
before any launch, so the made-up device addresses are never read."""
import ctypes

import pytest

PTR = 0x10000                    # 16-byte aligned; never dereferenced
MSDA_OK, MSDA_ERR_ARGUMENT = 0, 1
GEOM = dict(N=1, S=16, M=8, D=32, L=2, Lq=4, P=2)      # in the D = 32 family and msda_prologue_supported; M*L*P = 32

# entry -> (tensors before the sizes, tensors behind them, indices of the row tensors among all of them, index of grad_value
#           or None, trailing arguments: "" / "ws" (workspace, bytes) / "wsf" (+ flags), the name its messages carry or None)
FWD, BWD, PFWD, PBWD = (5, 1, (0, 5), None), (6, 3, (0, 1), 6), (6, 3, (0, 6), None), (6, 4, (0, 1), 6)
ENTRIES = {
    "msda_forward_f32": FWD + ("", None), "msda_forward_f64": FWD + ("", None), "msda_forward_bf16": FWD + ("", None),
    "msda_forward_ws_f32": FWD + ("ws", None), "msda_forward_ws_bf16": FWD + ("ws", None),
    "msda_backward_f32": BWD + ("", None), "msda_backward_f64": BWD + ("", None),
    "msda_backward_bf16": BWD + ("", None), "msda_backward_bf16_gv32": BWD + ("", None),
    "msda_backward_ws_f32": BWD + ("wsf", None), "msda_backward_ws_f64": BWD + ("wsf", None),
    "msda_backward_ws_bf16": BWD + ("wsf", None), "msda_backward_ws_bf16_gv32": BWD + ("wsf", None),
    "msda_forward_prologue_f32": PFWD + ("", "msda_forward_prologue_f32"),
    "msda_forward_prologue_ws_f32": PFWD + ("ws", "msda_forward_prologue_f32"),
    "msda_forward_prologue_bf16": PFWD + ("", "msda_forward_prologue_bf16"),
    "msda_forward_prologue_ws_bf16": PFWD + ("ws", "msda_forward_prologue_bf16"),
    "msda_backward_prologue_f32": PBWD + ("", "msda_backward_prologue_f32"),
    "msda_backward_prologue_ws_f32": PBWD + ("wsf", "msda_backward_prologue_f32"),
    "msda_backward_prologue_bf16_gv32": PBWD + ("wsf", "msda_backward_prologue_bf16_gv32"),
}
PROLOGUE = sorted(e for e in ENTRIES if ENTRIES[e][5])
PLAIN = sorted(e for e in ENTRIES if not ENTRIES[e][5])
assert len(ENTRIES) == 20 and len(PROLOGUE) == 7 and len(PLAIN) == 13

SIZES = b"msda: sizes must be positive (N, S, Lq may be 0)"
NULL = b"msda: null device pointer"
GEOMETRY = b"%s: geometry not supported (msda_prologue_supported)"
STRIDES = b"%s: row strides (65, 32) must be >= (64, 32), the first even on an 8-byte aligned base"
ALIGNED = (b"%s: row tensors must be 16-byte (fp32) / 8-byte (bf16) aligned and (x, y) tensors 8-byte aligned (a contiguous view at "
           b"an odd element offset is not)")
BF16_GV = (b"msda_backward_bf16: bf16 grad_value needs the D=32 kernel family (D == 32, L <= 16, L*P <= 32, 8-byte aligned rows); "
           b"msda_backward_bf16_gv32 serves every other shape")


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


def _call(lib, entry, tensors=None, ld_offsets=0, **sizes):
    """The entry with good arguments (made-up aligned addresses, GEOM, dense rows, no workspace, no flags) except the ones
    given; tensors: {index among the entry's tensors: address}.  Returns (return code, message)."""
    n_in, n_out, _, _, tail, _ = ENTRIES[entry]
    t = [PTR] * (n_in + n_out)
    for i, p in (tensors or {}).items():
        t[i] = p
    g = dict(GEOM, **sizes)
    args = t[:n_in] + [g[k] for k in ("N", "S", "M", "D", "L", "Lq", "P")]
    if "prologue" in entry:
        args += [ld_offsets, 0]
    args += t[n_in:] + {"": [], "ws": [None, 0], "wsf": [None, 0, 0]}[tail] + [None]
    rc = getattr(lib, entry)(*args)
    return rc, lib.msda_last_error()


def _cases(entry):
    """[(what, keyword arguments of _call, expected return code, expected whole message)] of one entry."""
    n_in, n_out, rows, gv, _, who = ENTRIES[entry]
    n = n_in + n_out
    who = who.encode() if who else None
    cases = [("M = 0", dict(M=0), MSDA_ERR_ARGUMENT, SIZES)]
    cases += [("tensor %d null" % i, dict(tensors={i: None}), MSDA_ERR_ARGUMENT, NULL) for i in range(n)]
    if who is None:
        cases.append(("N = 0, null tensors", dict(N=0, tensors={i: None for i in range(n)}), MSDA_OK, b""))
    else:
        cases += [(what, kw, MSDA_ERR_ARGUMENT, GEOMETRY % who) for what, kw in
                  (("N = 0", dict(N=0)), ("D = 16", dict(D=16)), ("L*P not a power of two", dict(L=3)))]
        cases.append(("odd ld_offsets", dict(ld_offsets=65), MSDA_ERR_ARGUMENT, STRIDES % who))
        # +4 bytes: off the 16-byte grid of fp32 rows and off the 8-byte grid of bf16 rows
        cases += [("row tensor %d at +4" % i, dict(tensors={i: PTR + 4}), MSDA_ERR_ARGUMENT, ALIGNED % who) for i in rows]
        if entry == "msda_backward_prologue_bf16_gv32":                     # fp32 grad_value beside bf16 rows: 16-byte rule
            cases.append(("grad_value at +8", dict(tensors={gv: PTR + 8}), MSDA_ERR_ARGUMENT, ALIGNED % who))
    if entry in ("msda_backward_bf16", "msda_backward_ws_bf16"):           # (the _ws_ form reports under the plain name)
        cases += [("D = 16", dict(D=16), MSDA_ERR_ARGUMENT, BF16_GV),
                  ("grad_out at +2", dict(tensors={0: PTR + 2}), MSDA_ERR_ARGUMENT, BF16_GV)]
    return cases


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_entry_answers_the_same_table(lib, entry):
    before = lib.msda_launch_count()
    for what, kw, want_rc, want_msg in _cases(entry):
        rc, msg = _call(lib, entry, **kw)
        assert (rc, msg) == (want_rc, want_msg), (entry, what)
    assert lib.msda_launch_count() == before
