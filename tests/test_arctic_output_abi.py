"""C ABI of make_output's glue entries (csrc/msda_arctic_output.hip; added without an ABI version bump): the symbols are
exported, the supported queries answer on the host at their limits, and argument errors come back as codes from the host-side
checks before anything is launched (msda_launch_count unchanged) — so no GPU is needed, and the fake device addresses never
reach a kernel.  On CPU tensors the three Python functions are the torch composition, bitwise."""
import ctypes

import pytest
import torch

V = ctypes.c_void_p
P = 0x10000
ERR_ARGUMENT = 1
SYMBOLS = ("msda_arctic_pose_supported", "msda_arctic_pose_forward_f32", "msda_arctic_pose_backward_f32",
           "msda_arctic_m2aa_forward_f32", "msda_arctic_m2aa_backward_f32", "msda_arctic_place_supported",
           "msda_arctic_place_forward_f32", "msda_arctic_place_backward_f32")
IMG = 224.0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    yield _native.declare(ctypes.CDLL(_native.LIB_PATH))


def _ints(vals):
    return ctypes.cast((ctypes.c_int * len(vals))(*vals), V)


def _ptrs(n, value=P):
    return ctypes.cast((V * n)(*([value] * n)), V)


def _pose_fwd(lib, nh=2, nr=3, B=32, img=IMG, poses=None, roots=None, K=P, mats=None, aa=None, ct=None):
    d = lambda v, n: v if v is not None else _ptrs(n)  # noqa: E731
    return lib.msda_arctic_pose_forward_f32(nh, nr, B, img, d(poses, 2), d(roots, 3), K, d(mats, 2), d(aa, 2), d(ct, 3), None)


def _place_fwd(lib, n=7, B=32, img=IMG, rows=None, cams=None, proj=None, points=None, cam_t=None, K=P, placed=None, n2=None,
               px=None):
    m = max(n, 1)
    rows = rows if rows is not None else [778, 778, 21, 21, 32, 16, 4000, 5, 5][:m]
    cams = cams if cams is not None else [0, 1, 0, 1, 2, 2, 2, 2, 2][:m]
    proj = proj if proj is not None else [0, 0, 1, 1, 1, 1, 0, 0, 0][:m]
    d = lambda v, k: v if v is not None else _ptrs(k)  # noqa: E731
    return lib.msda_arctic_place_forward_f32(n, B, img, _ints(rows), _ints(cams), _ints(proj), d(points, m), d(cam_t, 3), K,
                                             d(placed, m), d(n2, m), d(px, m), None)


def test_symbols_exported(lib):
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_supported_limits(lib):
    assert lib.msda_arctic_place_supported(8, 32, 8192) == 1
    assert lib.msda_arctic_place_supported(8, 32, 8193) == 0
    assert lib.msda_arctic_place_supported(9, 32, 8192) == 0
    assert lib.msda_arctic_place_supported(1, 0, 1) == 1                   # an empty batch is taken (and launches nothing)
    assert lib.msda_arctic_place_supported(0, 32, 100) == 0
    assert lib.msda_arctic_place_supported(7, 65535, 4000) == 1 and lib.msda_arctic_place_supported(7, 65536, 4000) == 0
    assert lib.msda_arctic_pose_supported(2, 3, 32) == 1
    assert lib.msda_arctic_pose_supported(2, 3, 0) == 1
    assert lib.msda_arctic_pose_supported(3, 3, 32) == 0 and lib.msda_arctic_pose_supported(2, 4, 32) == 0
    assert lib.msda_arctic_pose_supported(0, 0, 32) == 0
    assert lib.msda_arctic_pose_supported(2, 3, 65535) == 1 and lib.msda_arctic_pose_supported(2, 3, 65536) == 0
    assert lib.msda_arctic_pose_supported(2, 3, -1) == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(nh=3), b"unsupported geometry"),
    (dict(nr=4), b"unsupported geometry"),
    (dict(nh=0, nr=0), b"unsupported geometry"),
    (dict(B=-1), b"unsupported geometry"),
    (dict(img=0.0), b"img_res must be positive"),
    (dict(poses=_ptrs(2, 0)), b"null pointer"),
    (dict(roots=_ptrs(3, 0)), b"null pointer"),
    (dict(K=None), b"null pointer"),
    (dict(mats=_ptrs(2, 0)), b"null output"),
    (dict(ct=_ptrs(3, 0)), b"null output"),
])
def test_pose_argument_errors(lib, kw, msg):
    before = lib.msda_launch_count()
    assert _pose_fwd(lib, **kw) == ERR_ARGUMENT
    assert msg in lib.msda_last_error()
    assert lib.msda_launch_count() == before


def test_pose_backward_and_m2aa_argument_errors(lib):
    before = lib.msda_launch_count()
    bwd = lib.msda_arctic_pose_backward_f32
    assert bwd(2, 3, 32, IMG, _ptrs(2), _ptrs(3), P, None, _ptrs(2), _ptrs(3), _ptrs(2), _ptrs(3), None) == ERR_ARGUMENT
    assert b"null pointer" in lib.msda_last_error()
    assert bwd(2, 3, 32, IMG, _ptrs(2), _ptrs(3), P, _ptrs(2), _ptrs(2), _ptrs(3), _ptrs(2), None, None) == ERR_ARGUMENT
    assert bwd(2, 3, 32, IMG, _ptrs(2, 0), _ptrs(3), P, _ptrs(2), _ptrs(2), _ptrs(3), _ptrs(2), _ptrs(3), None) == ERR_ARGUMENT
    assert lib.msda_arctic_m2aa_forward_f32(0, 32, _ptrs(2), _ptrs(2), None) == ERR_ARGUMENT
    assert b"unsupported geometry" in lib.msda_last_error()
    assert lib.msda_arctic_m2aa_forward_f32(3, 32, _ptrs(3), _ptrs(3), None) == ERR_ARGUMENT
    assert lib.msda_arctic_m2aa_forward_f32(2, 32, _ptrs(2, 0), _ptrs(2), None) == ERR_ARGUMENT
    assert b"null pointer" in lib.msda_last_error()
    assert lib.msda_arctic_m2aa_forward_f32(2, 32, _ptrs(2), _ptrs(2, 0), None) == ERR_ARGUMENT
    assert b"null output" in lib.msda_last_error()
    assert lib.msda_arctic_m2aa_backward_f32(2, 32, _ptrs(2), None, _ptrs(2), None) == ERR_ARGUMENT
    assert lib.msda_arctic_m2aa_backward_f32(2, 70000, _ptrs(2), _ptrs(2), _ptrs(2), None) == ERR_ARGUMENT
    assert lib.msda_launch_count() == before


@pytest.mark.parametrize("kw,msg", [
    (dict(n=0), b"1 .. 8 segments"),
    (dict(n=9), b"1 .. 8 segments"),
    (dict(n=1, rows=[8193], cams=[0], proj=[0]), b"1 .. 8192 rows"),
    (dict(n=1, rows=[0], cams=[0], proj=[0]), b"1 .. 8192 rows"),
    (dict(n=1, rows=[21], cams=[3], proj=[0]), b"camera index"),
    (dict(n=1, rows=[21], cams=[-1], proj=[0]), b"camera index"),
    (dict(n=1, rows=[21], cams=[0], proj=[2]), b"project must be 0 or 1"),
    (dict(B=65536), b"unsupported geometry"),
    (dict(img=-1.0), b"img_res must be positive"),
    (dict(points=_ptrs(7, 0)), b"null pointer"),
    (dict(cam_t=_ptrs(3, 0)), b"null pointer"),
    (dict(K=None), b"null pointer"),
    (dict(placed=_ptrs(7, 0)), b"null output"),
    (dict(n2=_ptrs(7, 0)), b"null output"),
])
def test_place_argument_errors(lib, kw, msg):
    before = lib.msda_launch_count()
    assert _place_fwd(lib, **kw) == ERR_ARGUMENT
    assert msg in lib.msda_last_error()
    assert lib.msda_launch_count() == before


def test_place_backward_argument_errors(lib):
    before = lib.msda_launch_count()
    bwd = lib.msda_arctic_place_backward_f32
    geo = (_ints([21, 32]), _ints([0, 2]), _ints([1, 1]))
    assert bwd(2, 32, IMG, *geo, _ptrs(2), _ptrs(3), P, _ptrs(2), _ptrs(2), _ptrs(2), None, _ptrs(3), None) == ERR_ARGUMENT
    assert b"null pointer" in lib.msda_last_error()
    assert bwd(2, 32, IMG, *geo, _ptrs(2, 0), _ptrs(3), P, _ptrs(2), _ptrs(2), _ptrs(2), _ptrs(2), _ptrs(3), None) == ERR_ARGUMENT
    assert bwd(2, 32, IMG, _ints([21, 9000]), geo[1], geo[2], _ptrs(2), _ptrs(3), P, _ptrs(2), _ptrs(2), _ptrs(2), _ptrs(2),
               _ptrs(3), None) == ERR_ARGUMENT
    assert lib.msda_launch_count() == before


def test_empty_batches_launch_nothing(lib):
    before = lib.msda_launch_count()
    assert _pose_fwd(lib, B=0) == 0
    assert lib.msda_arctic_pose_backward_f32(2, 3, 0, IMG, _ptrs(2), _ptrs(3), P, _ptrs(2), _ptrs(2), _ptrs(3), _ptrs(2), _ptrs(3),
                                             None) == 0
    assert lib.msda_arctic_m2aa_forward_f32(2, 0, _ptrs(2), _ptrs(2), None) == 0
    assert lib.msda_arctic_m2aa_backward_f32(2, 0, _ptrs(2), _ptrs(2), _ptrs(2), None) == 0
    assert _place_fwd(lib, B=0) == 0
    geo = (_ints([21, 32]), _ints([0, 2]), _ints([1, 1]))
    assert lib.msda_arctic_place_backward_f32(2, 0, IMG, *geo, _ptrs(2), _ptrs(3), P, _ptrs(2), _ptrs(2), _ptrs(2), _ptrs(2),
                                              _ptrs(3), None) == 0
    assert lib.msda_launch_count() == before


def test_cpu_tensors_take_the_composition_bitwise(lib):
    from uvhand_amd import arctic_output as AO
    from uvhand_amd.object_tensors import axis_angle_to_matrix
    from uvhand_amd.small_loss import project_normalise, weak_perspective_to_perspective

    g = torch.Generator().manual_seed(5)
    B = 3
    poses = [torch.randn(B, 48, generator=g) for _ in range(2)]
    roots = [torch.rand(B, 3, generator=g) for _ in range(3)]
    K = torch.tensor([[1000.0, 0, 112], [0, 1000.0, 112], [0, 0, 1]]).repeat(B, 1, 1)
    before = lib.msda_launch_count()
    mats, aas, cts = AO.pose_heads(poses, roots, K, IMG)
    focal = (K[:, 0, 0] + K[:, 1, 1]) / 2.0
    for p, m, a in zip(poses, mats, aas):
        ref = axis_angle_to_matrix(p.reshape(-1, 3)).reshape(-1, 16, 3, 3)
        assert torch.equal(m, ref) and torch.equal(a, AO.matrix_to_axis_angle(ref.reshape(-1, 3, 3)).reshape(-1, 48))
    for r, c in zip(roots, cts):
        assert torch.equal(c, weak_perspective_to_perspective(r, focal, IMG))
    back = AO.matrix_to_axis_angle_many(mats)
    assert all(torch.equal(b, AO.matrix_to_axis_angle(m)) and b.shape == (B, 16, 3) for b, m in zip(back, mats))
    pts = [torch.randn(B, n, 3, generator=g) for n in (5, 21, 7)]
    res = AO.place_many([(pts[0], 0, False), (pts[1], 2, True), (pts[2], 1, True)], cts, K, IMG)
    for (placed, n2, px), p, cam, proj in zip(res, pts, (0, 2, 1), (False, True, True)):
        ref = p + cts[cam][:, None, :]
        assert torch.equal(placed, ref)
        if proj:
            rn = project_normalise(K, ref, IMG)
            assert torch.equal(n2, rn) and torch.equal(px, 0.5 * IMG * (rn + 1))
        else:
            assert n2 is None and px is None
    assert lib.msda_launch_count() == before
