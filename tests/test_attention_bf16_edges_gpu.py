"""The resident bf16 decoder self-attention core (msda_attn32_*_bf16, include/msda.h; uvhand_amd/csrc/msda_attn.hip) at every
edge its code has, against the fp64 formula of tests/test_attention_long_gpu.py on the (bf16-rounded, upcast) inputs, the keep mask
restated in numpy from the same seed.

Tolerance: the project's rule for bf16 nodes as test_attention_long_bf16_gpu._rule16 states it: per tensor — out, dq, dk, dv —
the kernel's largest error against fp64 may be at most 4 times the largest error of a torch restatement of the kernels' own
rounding points (`attn32_bf16_reference` below: fp32 on the GPU, the backward by its explicit formulas), a yardstick that counts
as at least one bf16 ulp of the tensor's largest fp64 value; where the fp64 dq / dk is identically zero (Lk = 1) the floor is
one bf16 ulp of the sum's condition value.  lse is an fp32 output and takes test_attention_long_gpu._rule against the fp32
formula.  The resident kernels' rounding points (attn32_*_bf16_kernel) are not the streaming ones: P_drop is normalised
(p * keep_scale / sum) and THEN rounded to bf16 before P . V; out is rounded once; delta = sum bf16(dO) * bf16(out) in fp32;
P * keep_scale is rounded before dV; dS before dQ and dK; each gradient once, after the multiply by scale.

The edges: rows padded to 32 in LDS and score tiles in pairs of 32
keys (forward, dQ) or queries (dK / dV) — lengths 1, 16, 17, 31, 32, 33, 65 —, a wavefront of dK / dV that owns 16 keys while
it walks 32-query pairs (16, 17 keys against 33, 65 queries), the deal of 16-row tiles to the 12 wavefronts (192, 193), the
rounds of the LDS fill (192, 289), the last sizes (319, 320), and the transposed LDS read that needs every lane of a
wavefront active whatever the lengths are.  Every shape runs flat and peaked (q and k times 3), as in
tests/test_attention_edges_gpu.py, whose view, sentinel and mask-extraction tests run here on bf16 tensors.

Measured on an MI355X (ratio = kernel error / yardstick, worst per tensor and regime): see README, "The resident
decoder self-attention cores at their edges"."""
import numpy as np
import pytest
import torch

from test_attention_gpu import _keep_mask
from test_attention_long_gpu import RATIOS as RATIOS32, SCALE, _formula, _rule, _seed_tensor
from test_attention_long_bf16_gpu import RATIOS as RATIOS16, _rule16, _ulp16
from test_attention_edges_gpu import (GAIN, _extract_forward_mask, _keep, _largest_probability, _nothing_outside_the_views_is_written,
                                      _run, _views_give_the_bits_of_contiguous_tensors)

pytestmark = pytest.mark.gpu

TAG = "resident bf16"                                    # this file's keys in the two RATIOS tables
BF16 = torch.bfloat16
CROSS = (1, 16, 17, 31, 32, 33, 65)
LARGE = [(192, 192), (193, 193), (289, 289), (319, 319), (320, 320), (320, 1), (1, 320), (33, 320), (320, 33)]
SHAPES = [(Lq, Lk) for Lq in CROSS for Lk in CROSS] + LARGE
assert _ulp16(1.0) == 2.0 ** -7


def attn32_bf16_reference(q, k, v, go, heads, keep, p):
    """The resident kernels' rounding points restated in torch, fp32 on the GPU, backward by its formulas (no autograd)."""
    Lq, N, E = q.shape
    Lk, hd = k.shape[0], E // heads
    rb = lambda t: t.to(BF16).float()
    split = lambda t, L: t.float().reshape(L, N * heads, hd).transpose(0, 1)
    join = lambda t, L: t.transpose(0, 1).reshape(L, N, E)
    Q, K, V, G = split(q, Lq), split(k, Lk), split(v, Lk), split(go, Lq)
    ks = 1.0 / (1.0 - float(np.float32(p)))
    s = torch.bmm(Q, K.transpose(1, 2)) * SCALE
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    total = e.sum(-1, keepdim=True)
    kf = keep.float() if p > 0 else torch.ones_like(e)
    out = rb(torch.bmm(rb(e * kf * (ks / total)), V))                       # normalised, then rounded; out rounded once
    lse = m + torch.log(total)
    P = torch.exp(s - lse)                                                  # recomputed from lse, as the backward does
    delta = (G * out).sum(-1, keepdim=True)                                 # from the rounded out, in fp32
    dP = torch.bmm(G, V.transpose(1, 2))
    dV = rb(torch.bmm(rb(P * kf * ks).transpose(1, 2), G))
    dS = rb(P * (dP * kf * ks - delta))
    dQ = rb(torch.bmm(dS, K) * SCALE)
    dK = rb(torch.bmm(dS.transpose(1, 2), Q) * SCALE)
    return {"out": join(out, Lq), "dq": join(dQ, Lq), "dk": join(dK, Lk), "dv": join(dV, Lk), "lse": lse.squeeze(-1)}


def _inputs(Lq, Lk, N, heads, regime):
    """bf16 q and k as column blocks of one packed tensor (what the wrapper passes), v and grad_out dense; the two regimes draw
    the same numbers and differ in the gain of q and k"""
    g = torch.Generator().manual_seed(Lq * 7 + Lk + N)
    E = heads * 32
    qk = (torch.randn(max(Lq, Lk), N, 2 * E, generator=g) * GAIN[regime]).to(BF16).cuda()
    return (qk[:Lq, :, :E], qk[:Lk, :, E:], torch.randn(Lk, N, E, generator=g).to(BF16).cuda(),
            torch.randn(Lq, N, E, generator=g).to(BF16).cuda())


def _check_core(what, regime, Lq, Lk, N, heads, p):
    q, k, v, go = _inputs(Lq, Lk, N, heads, regime)
    seed_value = 0x1234567890ABCDEF ^ (Lq << 20) ^ Lk
    seed = _seed_tensor(seed_value)
    ours = _run(q, k, v, go, heads, p, seed)
    for name in ("out", "dq", "dk", "dv"):
        assert ours[name].dtype == BF16
    assert ours["lse"].dtype == torch.float32
    keep = _keep(seed_value, N * heads, Lq, Lk, p)
    r64 = _formula(q, k, v, go, heads, keep, p, None, torch.float64)
    t32 = _formula(q, k, v, go, heads, keep, p, None, torch.float32)
    rest = attn32_bf16_reference(q, k, v, go, heads, keep, p)
    what = "%s %s %s" % (TAG, regime, what)
    for name in ("out", "dq", "dk", "dv"):
        _rule16(what, "%s %s %s" % (TAG, regime, name), ours[name], rest[name], r64[name], r64.get(name + "_cond", 0.0))
    _rule(what, "%s %s lse" % (TAG, regime), ours["lse"].view(N * heads, Lq), t32["lse"], r64["lse"])
    assert all(torch.isfinite(ours[n]).all() for n in ours)


@pytest.mark.parametrize("regime", ["flat", "peaked"])
@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_core_matches_fp64_at_the_edges(Lq, Lk, regime):
    N, heads = 2, 2
    if regime == "peaked" and Lk >= 48:                  # the regime is what its name says
        q, k, _, _ = _inputs(Lq, Lk, N, heads, regime)
        top = _largest_probability(q, k, heads)
        above_half, one_hot = float((top > 0.5).double().mean()), float((top > 1.0 - 2.0 ** -24).double().mean())
        print("%dx%d peaked: rows with a key above 1/2: %.3f, one-hot to fp32: %.4f" % (Lq, Lk, above_half, one_hot))
        assert above_half >= 0.5 and one_hot < 0.05
    for p in (0.0, 0.1):
        _check_core("%dx%d p=%g" % (Lq, Lk, p), regime, Lq, Lk, N, heads, p)


@pytest.mark.parametrize("Lq,Lk", LARGE)
def test_bf16_core_drops_what_the_fp32_core_drops(Lq, Lk):
    """p = 0.5, one seed tensor through both cores.  The forward's keep mask is read back out of each core key block by key
    block (test_attention_edges_gpu._extract_forward_mask: q = 0, 0 / 1 probes in v — the same values in bf16 and upcast): the
    bf16 core's output is non-zero exactly where the fp32 core's is, and where the numpy restatement keeps.  The bf16 backward is
    tied to the same mask by the parity rule at this rate (one different bit moves a gradient by O(max / Lk), by O(max) in the
    single-key case)."""
    seed_value, p = 0xDEADBEEF12345678 ^ (Lq << 20) ^ Lk, 0.5
    got16 = _extract_forward_mask(BF16, seed_value, p, Lq, Lk)
    got32 = _extract_forward_mask(torch.float32, seed_value, p, Lq, Lk)
    want = torch.from_numpy(_keep_mask(seed_value, 3, Lq, Lk, p))
    if Lq * Lk >= 10000:
        assert 0.49 < float(want.double().mean()) < 0.51
    assert torch.equal(got16, got32) and int((got16 != want).sum()) == 0
    _check_core("%dx%d p=0.5" % (Lq, Lk), "flat", Lq, Lk, 2, 2, 0.5)


def test_views_give_the_bits_of_contiguous_tensors():
    _views_give_the_bits_of_contiguous_tensors(BF16)


def test_nothing_outside_the_views_is_written():
    _nothing_outside_the_views_is_written(BF16)


def test_zz_print_ratios():
    for table in (RATIOS16, RATIOS32):
        for key in sorted(table):
            if key.startswith(TAG):
                print("worst ratio %-50s %.2f" % (key, table[key]))
