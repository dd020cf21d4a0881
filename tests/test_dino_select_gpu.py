"""The DINO query-selection kernels (csrc/msda_dino_select.hip) against the rule restated in numpy (a stable sort) and
torch.gather / index_put on the same inputs.  Every output is an integer or a copy, so every comparison is exact.  The shapes
are the smallest at which each path of the kernels can go wrong: one row, one wavefront and its neighbours, one 256- and one
1024-thread stride and their neighbours, the 8192 rows the older kernel stops at, a model-sized frame, a row index that needs
three radix digits; Q from one key to the LDS limit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import dino_transformer_inputs as TI  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 8191, 8192, 8193, 12276, 65537]
HAND = (12, 13)


def _dev():
    return torch.device("cuda:0")


def _native():
    from uvhand_amd import _native as MSDA
    return MSDA


def _queries(S):
    qs = [1, 2, min(S, 7), min(S, 900), min(S, 2048)] + ([S] if S <= 2048 else [])
    return sorted({q for q in qs if 1 <= q <= S})


def _order(cls):
    """The whole order of every frame under the rule, and every row's code."""
    return TI.numpy_select_rule(cls.cpu().numpy(), cls.shape[1], HAND)


def _check(cls, mem, prop, Q, order=None):
    """One forward on the kernels, compared exactly; returns (topk, slot)."""
    MSDA = _native()
    N, S, _ = cls.shape
    topk, slot, tgt, prop_sel, code = MSDA.dino_select_forward(cls, mem, prop, Q, HAND)
    if order is None:
        order = _order(cls)
    want = torch.from_numpy(np.ascontiguousarray(order[0][:, :Q])).to(cls.device)
    want_code = torch.from_numpy(np.ascontiguousarray(order[1][:, :Q])).to(cls.device)
    assert topk.dtype == torch.int64 and slot.dtype == torch.int32 and code.dtype == torch.uint8
    assert torch.equal(topk, want), "topk S=%d Q=%d K=%d" % (S, Q, cls.shape[2])
    want_slot = torch.full((N, S), -1, dtype=torch.int32, device=cls.device)
    want_slot.scatter_(1, want, torch.arange(Q, dtype=torch.int32, device=cls.device).expand(N, Q).contiguous())
    assert torch.equal(slot, want_slot)
    assert int((slot >= 0).sum(1).min()) == Q and int((slot >= 0).sum(1).max()) == Q
    assert torch.equal(torch.gather(slot, 1, topk), torch.arange(Q, dtype=torch.int32, device=cls.device).expand(N, Q))
    assert torch.equal(code, want_code)
    assert torch.equal(tgt, torch.gather(mem, 1, want[..., None].expand(-1, -1, mem.shape[-1])))
    assert torch.equal(prop_sel, torch.gather(prop, 1, want[..., None].expand(-1, -1, 42)))
    return topk, slot


def _data(N, S, K, C, seed):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    cls = torch.randn(N, S, K, generator=g, device=_dev())
    if N > 1:
        cls[1] = torch.round(cls[1] * 4) / 4             # a frame of ties: many rows share their maximum
    mem = torch.randn(N, S, C, generator=g, device=_dev())
    prop = torch.randn(N, S, 42, generator=g, device=_dev())
    dead = torch.rand(N, S, generator=g, device=_dev()) < 0.25
    prop[dead] = float("inf")                            # padded / out-of-range rows carry +inf proposals
    return cls, mem, prop


@pytest.mark.parametrize("S", SIZES)
def test_selection_matches_the_rule(S):
    cls14, mem256, prop = _data(2, S, 14, 256, 100 + S)
    inf_rows = 0
    for K in (1, 2, 14):
        cls = cls14[..., :K].contiguous()
        order = _order(cls)
        for C in (4, 256):
            mem = mem256[..., :C].contiguous()
            for Q in _queries(S):
                topk, _ = _check(cls, mem, prop, Q, order)
                inf_rows += int(torch.isinf(torch.gather(prop[..., 0], 1, topk)).sum())
    assert S < 64 or inf_rows > 0, "no +inf proposal row was ever selected: the gather of +inf went untested"


def test_widest_rows():
    cls, mem, prop = _data(3, 300, 256, 2048, 7)
    cls[2, 17, 200] = float("nan")
    for Q in (7, 300):
        _check(cls, mem, prop, Q)


def _patterns(S):
    """{name: row maxima [S] fp32}: value sets built to break a radix select or a tie rule."""
    rs = np.random.RandomState(S)
    bits = lambda u: np.asarray(u, dtype=np.uint32).view(np.float32)
    plateau = min(5000, S - 20)
    above = 899 if S > 2000 else 6
    where = rs.permutation(S)
    vp = np.full(S, 0.25, dtype=np.float32)
    vp[where[:above]] = 1.0 + rs.rand(above).astype(np.float32)
    vp[where[above:above + plateau]] = 0.5
    mixed = rs.standard_normal(S).astype(np.float32)
    mixed[rs.permutation(S)[:S // 5]] = np.inf
    mixed[rs.permutation(S)[:S // 7]] = -np.inf
    mixed[rs.permutation(S)[:S // 9]] = np.nan
    zeros = np.where(rs.rand(S) < 0.5, 0.0, -0.0).astype(np.float32)
    zeros[rs.permutation(S)[:S // 3]] = -1.0
    return {
        "all equal": np.full(S, -3.25, dtype=np.float32),
        "two values": np.where(rs.rand(S) < 0.3, 2.0, -2.0).astype(np.float32),
        "rows above a plateau": vp,
        "lowest mantissa byte": bits(0x3F800000 + rs.randint(0, 256, S)),
        "top byte only": bits((rs.randint(0, 255, S).astype(np.uint32) << 24) | 0x00400000),   # both signs, no NaN / inf
        "negative only": (-np.abs(rs.standard_normal(S)) - 1e-3).astype(np.float32),
        "denormals": bits(rs.randint(1, 1 << 10, S).astype(np.uint32) | (rs.randint(0, 2, S).astype(np.uint32) << 31)),
        "inf and nan": mixed,
        "signed zeros": zeros,
    }


def _threshold_queries(v, S):
    """Q below, at and above the number of rows strictly greater than a plateau's value, and inside / at the end of it."""
    cap = min(S, 2048)
    vv = np.where(np.isnan(v), np.inf, v.astype(np.float64))                  # NaN counted with +inf: only ranks matter here
    desc = -np.sort(-vv, kind="stable")
    qs = {1, cap}
    for rank in (cap // 2, cap - 1, 0):
        t = desc[min(rank, S - 1)]
        g, e = int((vv > t).sum()), int((vv == t).sum())
        qs |= {g - 1, g, g + 1, g + e // 2, g + e - 1, g + e, g + e + 1}
    return sorted(q for q in qs if 1 <= q <= cap)


@pytest.mark.parametrize("S", [257, 8193])
def test_adversarial_values(S):
    g = torch.Generator(device=_dev()).manual_seed(S)
    mem = torch.randn(1, S, 4, generator=g, device=_dev())
    prop = torch.randn(1, S, 42, generator=g, device=_dev())
    for name, v in _patterns(S).items():
        cls = np.repeat((v - np.float32(1.0))[:, None], 3, 1).astype(np.float32)
        cls[np.arange(S), np.arange(S) % 3] = v          # the maximum sits in class s % 3
        cls = torch.from_numpy(cls)[None].to(_dev())
        order = _order(cls)
        for Q in _threshold_queries(v, S):
            try:
                _check(cls, mem, prop, Q, order)
            except AssertionError as exc:
                raise AssertionError("%s, S=%d, Q=%d: %s" % (name, S, Q, exc)) from None


@pytest.mark.parametrize("S", [1, 65, 8193])
@pytest.mark.parametrize("C", [4, 256])
def test_backward_writes_every_element(S, C):
    MSDA = _native()
    cls, mem, prop = _data(2, S, 14, C, 300 + S)
    Q = min(S, 900)
    topk, slot, *_ = MSDA.dino_select_forward(cls, mem, prop, Q, HAND)
    g = torch.Generator(device=_dev()).manual_seed(5)
    grad_tgt = torch.randn(2, Q, C, generator=g, device=_dev())
    buf = torch.full((2, S, C), float("nan"), device=_dev())
    out = MSDA.dino_select_backward(slot, grad_tgt, out=buf)
    frames = torch.arange(2, device=_dev())[:, None].expand(2, Q)
    want = torch.zeros(2, S, C, device=_dev()).index_put((frames, topk), grad_tgt)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(out, want)


def test_autograd_through_the_node_equals_the_composition(monkeypatch):
    from uvhand_amd.functions import dino_func as DF
    cls, mem, prop = _data(2, 1025, 14, 256, 9)
    w = torch.randn(2, 900, 256, device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(1))
    got = []
    for fused in (True, False):
        monkeypatch.setattr(DF, "FUSED", fused)
        m = mem.clone().requires_grad_(True)
        c = cls.clone().requires_grad_(True)
        topk, tgt, prop_sel, code = DF.select_queries_dino(c, m, prop, 900)
        assert tgt.requires_grad and not prop_sel.requires_grad and not code.requires_grad and not topk.requires_grad
        (gm,) = torch.autograd.grad((tgt * w).sum(), m)
        got.append((topk, tgt.detach(), prop_sel, code, gm))
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_bits_repeat_and_frames_are_independent():
    MSDA = _native()
    cls, mem, prop = _data(2, 12276, 14, 256, 21)
    first = MSDA.dino_select_forward(cls, mem, prop, 900, HAND)
    again = MSDA.dino_select_forward(cls, mem, prop, 900, HAND)
    torch.use_deterministic_algorithms(True)
    try:
        strict = MSDA.dino_select_forward(cls, mem, prop, 900, HAND)
        g = torch.ones(2, 900, 256, device=_dev())
        b0, b1 = MSDA.dino_select_backward(first[1], g), MSDA.dino_select_backward(strict[1], g)
    finally:
        torch.use_deterministic_algorithms(False)
    for a, b, c in zip(first, again, strict):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(b0, b1)
    for n in range(2):
        alone = MSDA.dino_select_forward(cls[n:n + 1].contiguous(), mem[n:n + 1].contiguous(), prop[n:n + 1].contiguous(), 900, HAND)
        for a, b in zip(alone, first):
            assert torch.equal(a[0], b[n])


def test_forward_and_backward_replay_from_a_graph():
    from uvhand_amd.functions import dino_func as DF
    cls, mem, prop = _data(2, 8193, 14, 256, 31)
    mem.requires_grad_(True)
    w = torch.randn(2, 900, 256, device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(2))

    def step():
        topk, tgt, prop_sel, code = DF.select_queries_dino(cls, mem, prop, 900)
        (gm,) = torch.autograd.grad((tgt * w).sum(), mem)
        return topk, tgt.detach(), prop_sel, code, gm

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    before = step()[0]
    with torch.no_grad():
        cls.copy_(torch.randn(cls.shape, device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(3)))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = step()
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    assert not torch.equal(replayed[0], before), "the replay did not read the fresh logits"


@pytest.mark.parametrize("S", [1, 257, 1045, 8192])
def test_agrees_with_the_older_kernel_up_to_its_limit(S):
    from uvhand_amd.functions import two_stage_func as TS
    MSDA = _native()
    cls, mem, prop = _data(2, S, 14, 4, 400 + S)
    hand, obj = torch.full_like(prop, 2.0), torch.full_like(prop, 1.0)
    zero = torch.zeros_like(prop)
    for Q in _queries(S):
        unsig, _, idx = TS.select_queries(cls, hand, obj, zero, Q, hand_classes=HAND, return_indices=True)
        topk, _, _, _, code = MSDA.dino_select_forward(cls, mem, prop, Q, HAND)
        assert torch.equal(topk, idx)
        assert torch.equal(code, unsig[..., 0].to(torch.uint8))
