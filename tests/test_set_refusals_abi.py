"""The refusals the two matcher entries and the four criterion entries share (csrc/msda_abi.hip), as one table: per
condition and entry the return code and the whole message.  The host-side checks answer before anything is launched
(msda_launch_count unchanged), so no GPU is needed and the fake device addresses below never reach a kernel."""
import ctypes

import pytest

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
HAND_MASK = (1 << 12) | (1 << 13)
BASE = dict(sets=3, bs=4, Q=40, K=14, D=42, t_max=3, n=12, kp=P, arr=None, garr=None)

# entry -> (family, builder of its argument list from a case)
ENTRIES = {}


def _ptrs(n, value=P, null_at=None):
    vals = [value] * n
    if null_at is not None:
        vals[null_at] = 0
    return ctypes.cast((V * n)(*vals), V)


def _arr(c, key):
    return c[key] if c[key] is not None else _ptrs(max(c["sets"], 1))


def _entry(name, family):
    def register(build):
        ENTRIES[name] = (family, build)
        return build
    return register


@_entry("msda_match_arctic_f32", "match")
def _match_arctic(c):
    a = _arr(c, "arr")
    return [a, a, a, c["sets"], c["bs"], c["Q"], c["K"], c["D"], P, c["kp"], P, c["n"], P, c["t_max"], 1.5, 4.0, P, None, None]


@_entry("msda_match_assembly_f32", "match")
def _match_assembly(c):
    a = _arr(c, "arr")
    return [a, a, c["sets"], c["bs"], c["Q"], c["K"], c["D"], P, c["kp"], P, c["n"], c["t_max"], 1.5, 4.0, P, None, None]


def _criterion(c):
    a = _arr(c, "arr")
    return [0, a, a, a, c["sets"], c["bs"], c["Q"], c["K"], c["D"], P, c["t_max"], P, c["kp"], P, c["n"], P, P, HAND_MASK, P, 0.25]


@_entry("msda_criterion_fwd_f32", "criterion")
def _criterion_fwd(c):
    return _criterion(c) + [P, P, None]


@_entry("msda_criterion_bwd_f32", "criterion")
def _criterion_bwd(c):
    g = _arr(c, "garr")
    return _criterion(c) + [P, P, g, g, g, None]


def _criterion_dino(c):
    a, n = _arr(c, "arr"), max(c["sets"], 1)
    ints = ctypes.c_int * n
    return [a, a, a, ints(*[c["Q"]] * n), ints(*range(n)), c["sets"], c["bs"], c["K"], c["D"], 0, 0, P, n, c["t_max"], P, c["kp"],
            P, c["n"], P, HAND_MASK, P, 0.25]


@_entry("msda_criterion_dino_fwd_f32", "criterion_dino")
def _criterion_dino_fwd(c):
    return _criterion_dino(c) + [P, 1 << 40, P, P, None]


@_entry("msda_criterion_dino_bwd_f32", "criterion_dino")
def _criterion_dino_bwd(c):
    g = _arr(c, "garr")
    return _criterion_dino(c) + [P, P, g, g, g, None]


SETS_BS = {"match": "{who}: need 1 <= sets <= 16 and 0 <= bs <= 1024",
           "criterion": "{who}: need 1 <= sets <= 16 and 1 <= bs <= 1024",
           "criterion_dino": "{who}: need 1 <= sets <= 16 and 1 <= bs <= 1024"}
DIM = {"match": "{who}: need 1 <= D <= 64 with target keypoints, D = 0 without",
       "criterion": "{who}: need D >= 1 with target keypoints, D = 0 without",
       "criterion_dino": "{who}: need D >= 1 with target keypoints, D = 0 without"}
BEYOND = {f: "msda_%s: tensors beyond 2^31 elements" % f for f in ("match", "criterion", "criterion_dino")}
NULL = {"match": "msda_match: null device pointer", "criterion": "msda_criterion: null pointer",
        "criterion_dino": "msda_criterion_dino: null pointer"}
T_MAX = {"match": "{who}: need 1 <= Q <= 1024, K >= 1 and 0 <= t_max <= 16",
         "criterion": "{who}: need Q >= 1, K >= 1, D >= 0 and 0 <= t_max <= 16",
         "criterion_dino": "{who}: a matched set needs match_set[s] < match_sets and 0 <= t_max <= 16"}
ALL = tuple(ENTRIES)
BACKWARD = ("msda_criterion_bwd_f32", "msda_criterion_dino_bwd_f32")

# (condition, the case's changes (a dict, or one per family), the messages per family, the entries it applies to)
TABLE = [
    ("sets below the range", dict(sets=0), SETS_BS, ALL),
    ("sets above the range", dict(sets=17), SETS_BS, ALL),
    ("bs below the range", {"match": dict(bs=-1), "criterion": dict(bs=0), "criterion_dino": dict(bs=0)}, SETS_BS, ALL),
    ("bs above the range", dict(bs=1025), SETS_BS, ALL),
    ("target keypoints with D = 0", dict(D=0), DIM, ALL),
    # the AssemblyHands matcher always has target keypoints: without the pointer it has a null pointer, not a D mismatch
    ("D > 0 without target keypoints", dict(kp=None), DIM, tuple(e for e in ALL if e != "msda_match_assembly_f32")),
    ("targets beyond 2^31 elements", dict(n=1 << 31), BEYOND, ALL),
    ("a set's predictions beyond 2^31 elements", dict(bs=1024, Q=1024, K=2048), BEYOND, ALL),
    ("null array of per-set pointers", dict(arr=V(0)), NULL, ALL),
    ("null prediction pointer at set 0", dict(arr=_ptrs(3, null_at=0)), NULL, ALL),
    ("null prediction pointer at the last set", dict(arr=_ptrs(3, null_at=2)), NULL, ALL),
    ("null array of gradient pointers", dict(garr=V(0)), NULL, BACKWARD),
    ("null gradient pointer at set 0", dict(garr=_ptrs(3, null_at=0)), NULL, BACKWARD),
    ("null gradient pointer at the last set", dict(garr=_ptrs(3, null_at=2)), NULL, BACKWARD),
    ("t_max below the range", dict(t_max=-1), T_MAX, ALL),
    ("t_max above the range", dict(t_max=17), T_MAX, ALL),
]
ROWS = [(cond, entry) for cond, _, _, entries in TABLE for entry in entries]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def test_the_table_covers_every_entry_and_condition():
    assert len(ENTRIES) == 6 and len(ROWS) == 6 * 13 - 1 + 2 * 3
    assert {entry for _, entry in ROWS} == set(ENTRIES)


@pytest.mark.parametrize("cond,entry", ROWS, ids=["%s-%s" % (e, c.replace(" ", "_")) for c, e in ROWS])
def test_refusal_code_and_message(lib, cond, entry):
    _, changes, messages, _ = next(row for row in TABLE if row[0] == cond)
    family, build = ENTRIES[entry]
    case = dict(BASE, **(changes[family] if family in changes else changes))
    n0 = lib.msda_launch_count()
    assert getattr(lib, entry)(*build(case)) == ERR_ARGUMENT
    assert lib.msda_last_error().decode() == messages[family].format(who=entry)
    assert lib.msda_launch_count() == n0
