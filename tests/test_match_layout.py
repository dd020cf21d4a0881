"""The layout of the matchers' int64 result buffer (include/msda.h) as ``_native.match_layout`` states it: the slices equal
the slicing every reader wrote out by hand before there was one place for it, and ``matcher.indices_from_host`` reads a
hand-made buffer as before.  CPU tensors only."""
import pytest
import torch

from uvhand_amd import _native as MSDA
from uvhand_amd import matcher as M

SHAPES = [(1, 1, 0), (1, 1, 1), (3, 2, 16), (16, 1, 5)]


@pytest.mark.parametrize("sets,bs,t_max", SHAPES)
def test_slices_equal_the_hand_written_slicing(sets, bs, t_max):
    numel, slices = MSDA.match_layout(sets, bs, t_max)
    assert numel == 2 * sets * bs * t_max + 2 * sets * bs + 1
    buf = torch.arange(numel, dtype=torch.int64)
    n, W = sets * bs, t_max
    want = (buf[:n * W], buf[n * W:2 * n * W], buf[2 * n * W:2 * n * W + n], buf[2 * n * W + n:2 * n * W + 2 * n], buf[-1:])
    assert len(slices) == len(want)
    for sl, w in zip(slices, want):
        assert torch.equal(buf[sl], w)
    qi, ti, count, status, nvalid = MSDA.match_views(buf, sets, bs, t_max)
    assert torch.equal(qi, want[0].view(sets, bs, W)) and torch.equal(ti, want[1].view(sets, bs, W))
    assert torch.equal(count, want[2].view(sets, bs)) and torch.equal(status, want[3].view(sets, bs))
    assert nvalid.dim() == 0 and int(nvalid) == int(buf[-1])
    assert all(t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()        # views, not copies
               for t in (qi, ti, count, status, nvalid))


def _buffer(qi, ti, count, status, nvalid):
    return torch.tensor([x for part in (qi, ti) for s in part for k in s for x in k]
                        + [x for part in (count, status) for s in part for x in s] + [nvalid], dtype=torch.int64)


def test_indices_from_host_reads_a_hand_made_buffer():
    # 2 sets, 3 frame slots, t_max 2; two valid frames, so slot 2 is past them (count -1)
    qi = [[[4, 7], [0, -1], [-1, -1]], [[1, 2], [-1, -1], [-1, -1]]]
    ti = [[[1, 0], [0, -1], [-1, -1]], [[0, 1], [-1, -1], [-1, -1]]]
    count = [[2, 1, -1], [2, 0, -1]]
    status = [[0, 0, 0], [0, 0, 0]]
    buf = _buffer(qi, ti, count, status, 2)
    assert buf.numel() == MSDA.match_layout(2, 3, 2)[0]
    got = M.indices_from_host(buf, 2, 3, 2)
    assert [[(a.tolist(), b.tolist()) for a, b in per_set] for per_set in got] == \
        [[([4, 7], [1, 0]), ([0], [0])], [([1, 2], [0, 1]), ([], [])]]
    assert all(a.dtype == torch.int64 and b.dtype == torch.int64 for per_set in got for a, b in per_set)
    res = MSDA.match_views(buf, 2, 3, 2)
    assert res[0].tolist() == qi and res[1].tolist() == ti and res[2].tolist() == count and res[3].tolist() == status

    # a set whose valid frames have no pair reads as 0 when asked to
    empty = _buffer(qi, ti, [[2, 1, -1], [0, 0, -1]], status, 2)
    assert M.indices_from_host(empty, 2, 3, 2, zero_if_empty=True)[1] == 0
    assert M.indices_from_host(empty, 2, 3, 2)[1] != 0

    # a slot status raises the reference's error, and only among the valid frames
    for code, exc, text in ((MSDA.MATCH_INVALID, ValueError, M.INVALID_MSG), (MSDA.MATCH_INFEASIBLE, ValueError, M.INFEASIBLE_MSG),
                            (MSDA.MATCH_BAD_LABEL, IndexError, "out of bounds"), (MSDA.MATCH_BAD_TARGETS, RuntimeError, "offsets")):
        with pytest.raises(exc, match=text):
            M.indices_from_host(_buffer(qi, ti, count, [[0, 0, 0], [0, code, 0]], 2), 2, 3, 2)
        M.indices_from_host(_buffer(qi, ti, count, [[0, 0, code], [0, 0, 0]], 2), 2, 3, 2)
