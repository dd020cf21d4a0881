"""Seeded inputs and CPU yardsticks of the two-stage envelope tests (tests/test_two_stage_envelope*.py): plain torch, nothing
read from the reference, shared by the CPU and the GPU file.  The kernels under test are the four of csrc/msda_two_stage.hip
and ``level_proposals_kernel`` of csrc/msda_assembly.hip.

  proposals   ``proposal_mask`` builds N = 4 frames per level (clean; a rectangle padded on the right and bottom; fully padded;
              only the first row padded, so valid_W = 0 and the frame is dead), optionally with the ragged first row and the
              stray pixel of tests/test_two_stage_gpu.py on frame 0 (``ragged``) and with ``pad_cols`` columns padded on every
              frame.  ``proposals_f64`` is the fp64 restatement: extents off the first column / first row, the pixel centre over
              the extent in fp64, the 40 level-constant columns, the validity bit, the logit.  ``proposal_parts`` also returns
              what each row died of, for the vacuity counters of the CPU file.
  selection   ``select_case`` builds class logits of one of ``LOGITS`` with the row maxima placed so that the selected rows
              read every source the class rule can reach; ``select_oracle`` is max / stable descending sort / class rule /
              gather.
  embedding   ``pe_f64``; ``pe_rows`` holds the special values (+-inf, +-88, +-104, +-0, denormals, NaN).
  fused node  ``node_case`` builds r, W, b and the upstream gradient; ``node_f64`` is relu(PE @ W^T + b) and its weight and bias
              gradients under a given ReLU mask; ``node_dev32`` is the deviation of torch's own fp32 composition from it."""
import math

import torch
import torch.nn.functional as F

FLOOR = 16 * 2.0 ** -24
PROPOSAL_BOUND = 2e-6                  # |logit - fp64|, DESIGN.md §4.10
PE_BOUND = 2e-6                        # |PE - fp64|, DESIGN.md §4.10
MARGIN = 1e-4                          # relative distance every learned column keeps from 0.01 and 0.99, at every level

# ---- proposals ----------------------------------------------------------------------------------------------------------------
# name -> (levels, pad_cols, edges the case exists for).  Edges: "rule" rows that die of the (0.01, 0.99) rule on the pixel
# centre alone; "no_rule" no such row (49 is the widest extent without one); "trip2" an extent loop takes a second trip
# (H or W above 256, unpadded there); "xy" levels that die of the level-constant columns without learned offsets
PROPOSAL_CASES = {
    "mixed5": ([(300, 1), (1, 300), (51, 5), (2, 100), (7, 7)], 0, ("rule", "trip2")),
    "50x50": ([(50, 50)], 0, ("rule",)),
    "49x49": ([(49, 49)], 0, ("no_rule",)),
    "1x1": ([(1, 1)], 0, ("no_rule",)),
    "3x2x16": ([(3, 2)] * 16, 0, ("no_rule", "xy")),
    "257": ([(257, 2), (2, 257)], 0, ("rule", "trip2")),
    "4x60pad10": ([(4, 60)], 10, ("rule",)),
}
ASSEMBLY_CASES = {
    "300x1": ((300, 1), 0, ("rule", "trip2")),
    "1x300": ((1, 300), 0, ("rule", "trip2")),
    "50x50": ((50, 50), 0, ("rule",)),
    "49x49": ((49, 49), 0, ("no_rule",)),
    "4x60pad10": ((4, 60), 10, ("rule",)),
}
PATTERNS = ("plain", "ragged")
CHANNELS = (4, 8, 260)
# sigmoid(learnedxy) per mode: (low, high) of the 40 columns, then single columns set apart.  "in_range" is in range at
# levels 0 .. 6 (0.015 * 64 = 0.96): every level of every list except the sixteen-level one, where no value can be
# (0.01 < s and s * 2^15 < 0.99 exclude each other) and levels 7 and up die.
LEARNED = ("none", "in_range", "high_from_3", "low_at_0", "nan")
_LEARNED_RANGE = {"in_range": (0.0102, 0.0150), "high_from_3": (0.13, 0.24), "low_at_0": (0.0102, 0.0150), "nan": (0.0102, 0.0150)}


def proposal_mask(level_hw, pattern="plain", pad_cols=0):
    """[4, S] bool: the four frames of the module docstring over every level."""
    parts = []
    for (h, w) in level_hw:
        m = torch.zeros(4, h, w, dtype=torch.bool)
        if pad_cols:
            m[:, :, w - pad_cols:] = True
        we = w - pad_cols
        m[1, :, we - we // 3:] = True
        m[1, h - h // 3:, :] = True
        m[2] = True
        m[3, 0, :] = True
        if pattern == "ragged":
            m[0, 0, we - max(1, we // 3):] = True            # the valid width is read off the first row only
            if h > 2:
                m[0, 2, 0] = True                            # a hole in the first column: the extent is a count, not a length
        parts.append(m.flatten(1))
    return torch.cat(parts, 1)


def learned_offsets(mode, seed=0):
    """learnedxy [40] fp32 (or None) whose fp64 sigmoid lies where ``mode`` says."""
    if mode == "none":
        return None
    lo, hi = _LEARNED_RANGE[mode]
    g = torch.Generator().manual_seed(4100 + seed)
    s = lo + (hi - lo) * torch.rand(40, generator=g, dtype=torch.float64)
    if mode == "low_at_0":
        s[17] = 0.006                                        # 0.006 < 0.01 at level 0, 0.012 at level 1
    xy = torch.log(s / (1 - s)).float()
    if mode == "nan":
        xy[23] = float("nan")
    return xy


def learned_margin(xy, L):
    """The smallest relative distance of sigmoid(xy) * 2^l from 0.01 and 0.99 over the finite columns and l < L."""
    s = xy.double().sigmoid()
    s = s[torch.isfinite(s)]
    v = s[None, :] * (2.0 ** torch.arange(L, dtype=torch.float64))[:, None]
    return min(((v - 0.01).abs() / 0.01).min().item(), ((v - 0.99).abs() / 0.99).min().item())


def proposal_parts(mask, level_hw, learnedxy):
    """The fp64 restatement of the proposals with what each row died of.  ``mask`` [N, S] bool, ``learnedxy`` [40] or None.
    dict: props [N, S, 42] fp64 (+inf on dead rows), dead [N, S], padded [N, S], centre_ok [N, S] (the pixel-centre rule),
    level_ok [L] (the 40 level-constant columns), level [S], vh / vw [N, L]."""
    N, S = mask.shape
    props, centre_ok, level_of, level_ok, vhs, vws = [], [], [], [], [], []
    base = learnedxy.double().sigmoid() if learnedxy is not None else torch.full((40,), 0.05, dtype=torch.float64)
    cur = 0
    for l, (H, W) in enumerate(level_hw):
        m = mask[:, cur:cur + H * W].view(N, H, W)
        vh = (~m[:, :, 0]).sum(1).double()
        vw = (~m[:, 0, :]).sum(1).double()
        px = (torch.arange(W, dtype=torch.float64) + 0.5)[None, :] / vw[:, None]
        py = (torch.arange(H, dtype=torch.float64) + 0.5)[None, :] / vh[:, None]
        xy = base * 2.0 ** l
        p = torch.cat([px[:, None, :, None].expand(N, H, W, 1), py[:, :, None, None].expand(N, H, W, 1),
                       xy.expand(N, H, W, 40)], -1).reshape(N, H * W, 42)
        props.append(p)
        c = p[..., :2]
        centre_ok.append(((c > 0.01) & (c < 0.99)).all(-1))
        level_ok.append(bool(((xy > 0.01) & (xy < 0.99)).all()))
        level_of.append(torch.full((H * W,), l, dtype=torch.long))
        vhs.append(vh)
        vws.append(vw)
        cur += H * W
    assert cur == S
    p = torch.cat(props, 1)
    centre_ok = torch.cat(centre_ok, 1)
    level_of = torch.cat(level_of)
    level_ok = torch.tensor(level_ok)
    dead = mask | ~centre_ok | ~level_ok[level_of][None, :]
    logit = torch.log(p / (1 - p)).masked_fill(dead[..., None], float("inf"))
    return dict(props=logit, dead=dead, padded=mask, centre_ok=centre_ok, level_ok=level_ok, level=level_of,
                vh=torch.stack(vhs, 1), vw=torch.stack(vws, 1))


def proposals_f64(mask, level_hw, learnedxy):
    """(output_proposals [N, S, 42] fp64 with +inf on dead rows, dead [N, S] bool)."""
    parts = proposal_parts(mask, level_hw, learnedxy)
    return parts["props"], parts["dead"]


def proposal_counters(parts, level_hw):
    """rule: rows that are not padded, on a level whose constant columns are in range, and die of the pixel-centre rule alone;
    xy: levels that die of their constant columns; trip2: unpadded first-column rows / first-row columns at index >= 256."""
    rule = (~parts["padded"] & ~parts["centre_ok"] & parts["level_ok"][parts["level"]][None, :]).sum(1)
    trip2, cur = 0, 0
    for (H, W) in level_hw:
        m = parts["padded"][:, cur:cur + H * W].view(-1, H, W)
        trip2 += int((~m[:, 256:, 0]).sum()) + int((~m[:, 0, 256:]).sum())
        cur += H * W
    return dict(rule=rule, xy=int((~parts["level_ok"]).sum()), trip2=trip2)


def proposal_memory(N, S, C, seed):
    g = torch.Generator().manual_seed(4200 + seed)
    return torch.randn(N, S, C, generator=g), torch.randn(N, S, C, generator=g)


# ---- selection ----------------------------------------------------------------------------------------------------------------
SELECT_SHAPES = [(1, 1, 1, 1), (2, 2, 2, 14), (3, 3, 1, 14), (2, 1024, 300, 14), (2, 1025, 1025, 3), (2, 1023, 1023, 14),
                 (1, 4097, 1, 16), (1, 8192, 8192, 2), (5, 257, 0, 14)]
LOGITS = ("random", "half", "equal", "descending", "ascending", "zeros", "inf", "nan")
TIE_FREE = ("random", "descending", "ascending")            # no two row maxima of a frame equal, no NaN


def hand_classes_of(shape):
    """The hand-class pairs a shape runs with: (12, 13) where K holds them, (1, 2) at K = 3, and a pair at or above K."""
    K = shape[3]
    if K >= 14:
        return [(12, 13), (K, K + 1)] if shape == (2, 1024, 300, 14) else [(12, 13)]
    return [(1, 2)] if K == 3 else [(12, 13)]


SELECT_CASES = [(shape, logits, hc) for shape in SELECT_SHAPES for logits in LOGITS for hc in hand_classes_of(shape)]


def branch_classes(K, hand_classes):
    """{branch: the class indices below K that lead to it}; an empty list is a branch K and hand_classes make impossible."""
    hand = [k for k in range(K) if k in hand_classes]
    return dict(hand=hand, obj=[k for k in range(1, K) if k not in hand_classes], prop=[0])


def select_case(shape, logits, hand_classes, seed=0):
    """dict(cls [N, S, K], hand, obj, prop [N, S, 42], Q, hand_classes).  Row maxima by ``logits``; the class position of the
    maximum cycles through the reachable branches by the row's rank in its frame, so the first rows selected read them all."""
    N, S, Q, K = shape
    g = torch.Generator().manual_seed(4300 + seed + 7 * S + K)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if logits in ("random", "inf", "nan"):
        mx = rnd(N, S) * 2
    elif logits == "half":
        mx = (rnd(N, S) * 2).round() / 2                     # a handful of distinct values: long runs of ties
    elif logits == "equal":
        mx = torch.full((N, S), 0.75)
    elif logits in ("descending", "ascending"):
        mx = torch.sort(rnd(N, S) * 2, dim=1, descending=logits == "descending")[0]
    else:                                                    # zeros: maxima of -0.0 and +0.0 mixed, a third of the rows apart
        mx = torch.where(torch.rand(N, S, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
        other = torch.arange(S) % 3 == 2
        mx[:, other] = rnd(N, int(other.sum()))
    if logits == "inf" and S > 1:
        mx[:, 0::9] = float("inf")
        mx[:, 1::11] = float("-inf")
    rank = torch.argsort(torch.sort(mx, dim=1, descending=True, stable=True)[1], dim=1)
    kinds = [c for c in branch_classes(K, hand_classes).values() if c]
    table = torch.tensor([k + [k[0]] * (K - len(k)) for k in kinds])
    lens = torch.tensor([len(k) for k in kinds])
    rows = torch.arange(S)[None, :].expand(N, S)
    kind = (rank + torch.arange(N)[:, None]) % len(kinds)
    pos = table[kind, (rows // 3) % lens[kind]]
    finite = torch.isfinite(mx).unsqueeze(-1)
    below = mx.unsqueeze(-1) - 0.25 - torch.rand(N, S, K, generator=g) * 3
    if logits == "half":
        below = (below * 2).floor() / 2
    cls = torch.where(finite, below, torch.where(mx.unsqueeze(-1) > 0, rnd(N, S, K), torch.tensor(float("-inf"))))
    cls.scatter_(2, pos.unsqueeze(-1), mx.unsqueeze(-1))
    if logits in ("half", "zeros", "inf"):                   # the maximum once more later in the row (at "zeros" the zero of
        twice = (rows % 2 == 1) & (pos + 1 < K)              # the other sign): the first one is the class
        if logits == "zeros":
            twice &= mx == 0
        again = -mx if logits == "zeros" else mx
        nxt = (pos + 1).clamp(max=K - 1).unsqueeze(-1)
        cls.scatter_(2, nxt, torch.where(twice, again, torch.gather(cls, 2, nxt).squeeze(-1)).unsqueeze(-1))
    if logits == "nan":
        for n in range(N):
            for j, s in enumerate(range(0, S, 19)):          # about 5 % of the rows
                ks = kinds[(j + n) % len(kinds)]
                cls[n, s, ks[j % len(ks)]] = float("nan")    # NaN at differing class positions: the first NaN is the class
                if j % 4 == 3 and K > 1:
                    cls[n, s, K - 1] = float("nan")          # a second NaN later in the row
        if S > 2:
            cls[:, S - 1, :] = float("nan")                  # all NaN: class 0
            hand = branch_classes(K, hand_classes)["hand"]
            if hand:
                cls[:, S - 2, hand[-1]] = float("nan")       # a NaN in a hand column
    hand, obj, prop = (torch.randn(N, S, 42, generator=g) for _ in range(3))
    prop[:, ::17] = float("inf")                             # masked proposals
    return dict(cls=cls, hand=hand, obj=obj, prop=prop, Q=Q, hand_classes=tuple(hand_classes))


def select_oracle(cls, hand, obj, prop, Q, hand_classes):
    """(indices [N, Q], refpoint_unsig [N, Q, 42], {branch: selected rows that read it}).  torch.sort(descending, stable) puts
    NaN first and breaks ties, -0.0 == +0.0 among them, by the lower row; max(-1) returns the first maximum, the first NaN."""
    mx, arg = cls.max(-1)
    order = torch.sort(mx, dim=1, descending=True, stable=True)[1][:, :Q]
    a = torch.gather(arg, 1, order)
    is_hand = (a == hand_classes[0]) | (a == hand_classes[1])
    is_obj = ~is_hand & (a != 0)
    idx = order.unsqueeze(-1).expand(-1, -1, 42)
    ref = torch.where(is_hand.unsqueeze(-1), torch.gather(hand, 1, idx),
                      torch.where(is_obj.unsqueeze(-1), torch.gather(obj, 1, idx), torch.gather(prop, 1, idx)))
    counts = dict(hand=int(is_hand.sum()), obj=int(is_obj.sum()), prop=int((~is_hand & ~is_obj).sum()))
    return order, ref, counts


def impossible_branches(shape, hand_classes):
    """{branch: why no selected row of this case can read it}."""
    N, S, Q, K = shape
    why = {}
    for b, classes in branch_classes(K, hand_classes).items():
        if not classes:
            why[b] = "K = %d, hand classes %s: no class leads to it" % (K, tuple(hand_classes))
    return why


def branches_selected(shape, hand_classes):
    """How many different sources the selected rows must have read: every reachable one, or N * Q of them if that is fewer."""
    N, S, Q, K = shape
    return min(N * Q, 3 - len(impossible_branches(shape, hand_classes)))


# ---- embedding ----------------------------------------------------------------------------------------------------------------
PE_ROWS = (1, 3, 257)
SPECIALS = (float("inf"), float("-inf"), 88.0, -88.0, 104.0, -104.0, 0.0, -0.0, 1e-40, -1e-40, float("nan"))


def dim_t64():
    d = torch.arange(128, dtype=torch.float64)
    return 10000.0 ** (2 * torch.div(d, 2, rounding_mode="floor") / 128)


def pe_f64(r):
    """get_proposal_pos_embed in fp64: [M, 42] -> [M, 5376]."""
    u = r.double().sigmoid() * (2 * math.pi)
    pos = u[..., None] / dim_t64()
    return torch.stack((pos[..., 0::2].sin(), pos[..., 1::2].cos()), -1).flatten(-3)


def pe_rows(M, seed=0):
    """r [M, 42]: every special value in every row (at rotating columns), and at M = 257 also as whole rows."""
    g = torch.Generator().manual_seed(4400 + seed + M)
    r = torch.randn(M, 42, generator=g) * 2.5
    for m in range(M):
        for i, v in enumerate(SPECIALS):
            r[m, (5 * m + 3 * i) % 42] = v
    if M > 64:
        for i, v in enumerate(SPECIALS):
            r[64 + 7 * i, :] = v
    return r


# ---- fused node ---------------------------------------------------------------------------------------------------------------
NODE_CASES = [(1, 4), (63, 128), (64, 124), (65, 132), (129, 260), (130, 640), (513, 128), (100, 1020)]
NODE_TILES = [1, 1, 1, 4, 9, 15, 9, 16]


def node_tiles(M, Nc):
    return -(-M // 64) * -(-Nc // 128)


_NODE = {}


def node_case(M, Nc, seed=0):
    """dict(r [M, 42], w [Nc, 5376], b [Nc], gy [M, Nc]) fp32; weights as nn.Linear(5376, Nc) draws them.  Cached."""
    if (M, Nc, seed) not in _NODE:
        g = torch.Generator().manual_seed(4500 + seed + 31 * M + Nc)
        r = torch.randn(M, 42, generator=g) * 2.5
        if M > 4:
            r[3::37] = float("inf")                          # selected masked proposals
            r[4::41, ::5] = float("-inf")
        k = 1 / math.sqrt(5376)
        w = (torch.rand(Nc, 5376, generator=g) * 2 - 1) * k
        b = (torch.rand(Nc, generator=g) * 2 - 1) * k
        _NODE[M, Nc, seed] = dict(r=r, w=w, b=b, gy=torch.randn(M, Nc, generator=g))
    return _NODE[M, Nc, seed]


def node_f64(r, w, b, gy, mask=None):
    """dict(y, grad_w, grad_b) fp64 of relu(PE(r) @ w^T + b) under upstream gy; ``mask`` [M, Nc] bool is the ReLU mask the
    gradients use (the compared implementation's own y > 0: a flip at |h| of 1e-6 is not GEMM error), default h > 0."""
    pe = pe_f64(r)
    h = pe @ w.double().t()
    if b is not None:
        h = h + b.double()
    gh = gy.double() * ((h > 0) if mask is None else mask)
    return dict(y=h.clamp_min(0), grad_w=gh.t() @ pe, grad_b=gh.sum(0) if b is not None else None)


def rel_dev(got, ref):
    """max |got - ref| over max |ref|."""
    return float((got.double() - ref).abs().max() / ref.abs().max())


_DEV32 = {}


def node_dev32(M, Nc, bias, seed=0):
    """({tensor: deviation of torch's fp32 composition relu(linear(PE32(r))) and its autograd gradients from node_f64, relative
    to the tensor's largest magnitude}, {tensor: that magnitude}) on the CPU.  Cached."""
    from uvhand_amd.functions.two_stage_func import pos_embed_composition
    if (M, Nc, bias, seed) not in _DEV32:
        c = node_case(M, Nc, seed)
        w = c["w"].clone().requires_grad_(True)
        b = c["b"].clone().requires_grad_(True) if bias else None
        y = torch.relu(F.linear(pos_embed_composition(c["r"]), w, b))
        y.backward(c["gy"])
        ref = node_f64(c["r"], c["w"], c["b"] if bias else None, c["gy"], y.detach() > 0)
        got = dict(y=y.detach(), grad_w=w.grad, grad_b=b.grad if bias else None)
        names = [n for n in ("y", "grad_w", "grad_b") if ref[n] is not None]
        _DEV32[M, Nc, bias, seed] = ({n: rel_dev(got[n], ref[n]) for n in names}, {n: float(ref[n].abs().max()) for n in names})
    return _DEV32[M, Nc, bias, seed]


def node_bound(dev32):
    return max(4 * dev32, FLOOR)
