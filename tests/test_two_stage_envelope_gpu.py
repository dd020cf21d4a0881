"""The two-stage proposal, selection and embedding kernels (csrc/msda_two_stage.hip) and the one-level proposals kernel
(csrc/msda_assembly.hip) over their envelope on the GPU, against the CPU yardsticks of
tests/golden/two_stage_envelope_inputs.py.  tests/test_two_stage_envelope.py holds the builder's conditions (the edge every
case exists for is counted there), so nothing here passes vacuously.

Which case fails under which mistake:
  ``<`` for ``<=`` (or ``>`` for ``>=``) in the validity compare   proposals 50x50 and 4x60pad10 (valid width exactly 50:
                         0.5 / 50 is 0.01 and 49.5 / 50 is 0.99 in fp32 and fp64 alike, the border ring must die), both kernels
  no second trip of the extent loops (``h += 256``)               proposals mixed5 and 257, assembly 300x1 and 1x300 (the
                         extent would be 256: every logit of the level moves)
  another padding key in the sort                                 selection 1025x1025x3 and 4097x1x16 (half the keys are
                         padding, Q = S selects every real row; -inf rows, the lowest real keys, in ``inf``)
  no ``j >= Nc`` guard, no ``n < Nc`` guard                       fused node (64, 124), (65, 132), (129, 260), (100, 1020): the
                         output is a slice of a larger buffer whose other rows must keep their fill
  a swizzle that loses a tile (``logical >= tiles``)              fused node at 1, 4, 9 and 15 tiles, none a multiple of 8

Bounds, none taken from a kernel: proposals and PE 2e-6 absolute; fused node max(4 x dev32, 16 * 2^-24)
relative to each tensor's largest magnitude, dev32 the deviation of torch's own fp32 composition from the same fp64
restatement on the same inputs.  Selection and every mask, copy and gather: bitwise.

What this module found, both fixed in the kernels.  (1) Fused node (1, 4): y was 2.08e-6 of max |y| with a bias and 2.01e-6
without, 5.1 and 5.3 x dev32 (bound 4 x).  pe_linear_relu_kernel summed all 5376 products of an output in one MFMA chain; a
sequential fp32 chain over these inputs gives 1.5e-6 to 3.1e-6 on the CPU too, against 3e-7 to 6e-7 for torch's blocked GEMM.
It now sums chains of 256 columns into a total: 1.5 x dev32 on the same case, the table below.  (2) Assembly proposals: the
logits were two ulps from the composition's on the device at 300x1, 1x300, 50x50 and 4x60pad10 (bound: one).  The kernel wrote
the correctly rounded log of the fp32 ratio, and torch's device log is up to two ulps from that; the device logf, which the
kernel takes now, is within one ulp of torch's on every ratio of every extent up to 599.  No extent loop, validity compare,
padding key or Nc guard was wrong.  Outside the issue's cases the 2e-6 logit bound does not hold for any fp32 code: over all
extents up to 599 torch's own composition is up to 3.2e-6 from fp64 (the fp32 pixel centre next to 0.99).

Measured on one MI355X (kernel = max deviation of the kernel from fp64, composition = that of torch's fp32 ops):
Proposals, worst |logit - fp64| over both mask patterns and C = 4, 8, 260 (bound 2e-6; the same figure with and without
learned offsets unless noted):
  case        kernel    composition (CPU)
  mixed5      1.21e-06  1.04e-06 (1.29e-06 under high_from_3)
  50x50       1.21e-06  1.04e-06
  49x49       1.92e-06  1.92e-06
  1x1         4.77e-07  1.19e-07 (in_range; 4.48e-08 both without learned offsets)
  3x2x16      1.21e-06  1.29e-06
  257         1.93e-06  1.93e-06
  4x60pad10   1.21e-06  1.04e-06
The 49 and 257 figures are the fp32 pixel centre's: half an ulp of px at 0.98 is 1.5e-6 of the logit, for any fp32 code.
Assembly, kernel / composition on the device / ulps between them: 300x1 and 1x300 1.04e-06 / 1.04e-06 / 1, 50x50 and
4x60pad10 1.21e-06 / 1.21e-06 / 1, 49x49 1.92e-06 / 1.92e-06 / 1.
PE, kernel = composition (CPU): M = 1 6.36e-07, M = 3 1.01e-06, M = 257 1.05e-06 (bound 2e-6).
Fused node, ``kernel:dev32 ratio`` per tensor relative to its largest magnitude (- where dev32 is 0: one row, exact sum):
  (1, 4) bias          y 5.96e-07:4.07e-07 1.47  grad_w 7.95e-07:7.77e-07 1.02  grad_b 0.00e+00:0.00e+00 -
  (1, 4) nobias        y 5.86e-07:3.81e-07 1.54  grad_w 7.95e-07:7.77e-07 1.02
  (63, 128) bias       y 4.11e-07:3.52e-07 1.17  grad_w 3.44e-07:3.30e-07 1.04  grad_b 1.12e-07:6.78e-08 1.64
  (63, 128) nobias     y 4.16e-07:3.40e-07 1.23  grad_w 3.44e-07:3.30e-07 1.04
  (64, 124) bias       y 4.83e-07:2.89e-07 1.67  grad_w 4.30e-07:4.87e-07 0.88  grad_b 7.15e-08:1.21e-07 0.59
  (64, 124) nobias     y 4.66e-07:3.01e-07 1.55  grad_w 4.30e-07:4.87e-07 0.88
  (65, 132) bias       y 4.67e-07:3.64e-07 1.29  grad_w 4.50e-07:4.50e-07 1.00  grad_b 8.61e-08:1.19e-07 0.73
  (65, 132) nobias     y 4.59e-07:3.38e-07 1.36  grad_w 4.50e-07:4.50e-07 1.00
  (129, 260) bias      y 3.89e-07:5.24e-07 0.74  grad_w 5.51e-07:5.51e-07 1.00  grad_b 1.33e-07:7.18e-08 1.85
  (129, 260) nobias    y 3.88e-07:5.22e-07 0.74  grad_w 5.52e-07:5.52e-07 1.00
  (130, 640) bias      y 4.30e-07:3.67e-07 1.17  grad_w 6.94e-07:6.94e-07 1.00  grad_b 1.13e-07:1.14e-07 0.98
  (130, 640) nobias    y 4.19e-07:3.66e-07 1.14  grad_w 6.94e-07:6.94e-07 1.00
  (513, 128) bias      y 3.96e-07:4.64e-07 0.85  grad_w 9.13e-07:5.34e-07 1.71  grad_b 1.10e-07:1.53e-07 0.72
  (513, 128) nobias    y 4.03e-07:4.65e-07 0.87  grad_w 8.94e-07:4.82e-07 1.85
  (100, 1020) bias     y 4.13e-07:3.87e-07 1.07  grad_w 4.69e-07:4.69e-07 1.00  grad_b 1.41e-07:1.20e-07 1.18
  (100, 1020) nobias   y 4.06e-07:3.86e-07 1.05  grad_w 4.69e-07:4.69e-07 1.00
Worst: grad_w of (513, 128) without bias at 1.85 x dev32 and y of (64, 124) at 1.67 x; nothing is above half its bound.
"""
import sys
import types

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import two_stage_envelope_inputs as EI  # noqa: E402
from uvhand_amd import _native as MSDA  # noqa: E402
from uvhand_amd.functions import assembly_func as AF  # noqa: E402
from uvhand_amd.functions import two_stage_func as TS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- proposals ----------------------------------------------------------------------------------------------------------------
def _check_proposals(label, run, mask, levels, xy, C, seed, width):
    """One forward and backward of ``run(memory, mask) -> (memory_out, proposals)`` against the fp64 restatement: the +inf
    pattern, the zeroed rows and the gradient bitwise, the finite logits within 2e-6.  Returns (proposals, kernel deviation)."""
    N, S = mask.shape
    ref, dead = EI.proposals_f64(mask, levels, xy)
    ref = ref[..., :width]
    memory, go = EI.proposal_memory(N, S, C, seed)
    mem_d = memory.to(DEV).requires_grad_(True)
    n0 = MSDA.launch_count()
    mem_out, props = run(mem_d, mask.to(DEV))
    assert MSDA.launch_count() - n0 == 1                     # the kernel ran, not the composition
    assert props.shape == (N, S, width) and not props.requires_grad
    got = props.cpu().double()
    assert torch.equal(torch.isinf(got), dead.unsqueeze(-1).expand(N, S, width)) and not bool(torch.isnan(got).any())
    assert bool((got[torch.isinf(got)] > 0).all())
    assert torch.equal(mem_out.detach().cpu(), memory.masked_fill(dead.unsqueeze(-1), 0.0))
    n0 = MSDA.launch_count()
    mem_out.backward(go.to(DEV))
    assert MSDA.launch_count() - n0 == 1                     # msda_zero_masked_rows_f32
    assert torch.equal(mem_d.grad.cpu(), go.masked_fill(dead.unsqueeze(-1), 0.0))
    fin = ~torch.isinf(ref)
    dev = (got - ref)[fin].abs().max().item() if bool(fin.any()) else 0.0
    return props, dead, ref, dev


@pytest.mark.parametrize("learned", EI.LEARNED)
@pytest.mark.parametrize("name", EI.PROPOSAL_CASES)
def test_proposals_against_fp64(name, learned):
    levels, pad_cols, _ = EI.PROPOSAL_CASES[name]
    xy = EI.learned_offsets(learned)
    worst, worst32 = 0.0, 0.0
    for pattern in EI.PATTERNS:
        mask = EI.proposal_mask(levels, pattern, pad_cols)
        _, props32 = TS.proposals_composition(torch.zeros(4, mask.shape[1], 4), mask, levels, xy)
        for C in EI.CHANNELS:
            xy_d = xy.to(DEV).requires_grad_(True) if xy is not None else None
            run = lambda m, k: TS.encoder_output_proposals(m, k, levels, xy_d)  # noqa: E731
            _, dead, ref, dev = _check_proposals(name, run, mask, levels, xy, C, C, 42)
            if xy is not None:
                assert xy_d.grad is not None and xy_d.grad.shape == (40,) and torch.count_nonzero(xy_d.grad) == 0
            worst = max(worst, dev)
        row_mask = MSDA.two_stage_proposals(torch.zeros(4, mask.shape[1], 4, device=DEV), mask.to(DEV), levels,
                                            xy.to(DEV) if xy is not None else None)[2]
        assert row_mask.dtype == torch.bool and torch.equal(row_mask.cpu(), dead)
        fin = ~dead
        if bool(fin.any()):
            worst32 = max(worst32, (props32.double() - ref)[fin].abs().max().item())
    print("MEASURED proposals %s %s: kernel %.2e composition %.2e" % (name, learned, worst, worst32))
    assert worst <= EI.PROPOSAL_BOUND


@pytest.mark.parametrize("name", EI.ASSEMBLY_CASES)
def test_assembly_level_proposals_against_fp64(name):
    hw, pad_cols, _ = EI.ASSEMBLY_CASES[name]
    S = hw[0] * hw[1]
    worst, worst32, worst_ulp = 0.0, 0.0, 0
    for pattern in EI.PATTERNS:
        mask = EI.proposal_mask([hw], pattern, pad_cols)
        for C in EI.CHANNELS:
            # the level is the tail of a longer flattened pyramid: the frame stride is not H * W * C
            lead = 12
            full_mask = torch.cat([torch.zeros(4, lead, dtype=torch.bool), mask], 1).to(DEV)
            memory, go = EI.proposal_memory(4, lead + S, C, 100 + C)
            full = memory.to(DEV).requires_grad_(True)
            n0 = MSDA.launch_count()
            mem_out, props = AF.encoder_output_proposals(full[:, lead:], full_mask[:, lead:], [hw])
            assert MSDA.launch_count() - n0 == 1
            ref, dead = EI.proposals_f64(mask, [hw], None)
            ref = ref[..., :2]
            got = props.cpu().double()
            assert props.shape == (4, S, 2) and torch.equal(torch.isinf(got), dead.unsqueeze(-1).expand(4, S, 2))
            assert not bool(torch.isnan(got).any()) and bool((got[torch.isinf(got)] > 0).all())
            assert torch.equal(mem_out.detach().cpu(), memory[:, lead:].masked_fill(dead.unsqueeze(-1), 0.0))
            mem_out.backward(go[:, lead:].to(DEV))
            want = torch.cat([torch.zeros(4, lead, C), go[:, lead:].masked_fill(dead.unsqueeze(-1), 0.0)], 1)
            assert torch.equal(full.grad.cpu(), want)
            with torch.no_grad():
                c_mem, c_props = AF.proposals_composition(full[:, lead:], full_mask[:, lead:], [hw])
            assert torch.equal(c_mem, mem_out) and torch.equal(torch.isinf(c_props), torch.isinf(props))
            row_mask = MSDA.assembly_proposals(full.detach()[:, lead:], full_mask[:, lead:], hw)[2]
            assert row_mask.dtype == torch.bool and torch.equal(row_mask.cpu(), dead)
            fin = ~torch.isinf(ref)
            if bool(fin.any()):
                f = fin.to(DEV)
                ulps = (props[f].view(torch.int32).long() - c_props[f].view(torch.int32).long()).abs()
                assert bool((torch.sign(props[f]) == torch.sign(c_props[f])).all())
                worst_ulp = max(worst_ulp, int(ulps.max()))
                worst = max(worst, (got - ref)[fin].abs().max().item())
                worst32 = max(worst32, (c_props.cpu().double() - ref)[fin].abs().max().item())
    print("MEASURED assembly %s: kernel %.2e composition %.2e, ulps from the composition %d" % (name, worst, worst32, worst_ulp))
    assert worst <= EI.PROPOSAL_BOUND and worst_ulp <= 1


def test_proposals_backward_masked_fill_path():
    """The backward of both nodes without the row-zeroing kernel.  A forward that ran the kernel has C % 4 == 0 and hands the
    backward a fresh, aligned clone, so this path is not reachable through it: the backward is called on its own with the
    byte mask of a real forward and a gradient of six columns."""
    levels, pad_cols, _ = EI.PROPOSAL_CASES["4x60pad10"]
    mask = EI.proposal_mask(levels, "ragged", pad_cols)
    _, dead = EI.proposals_f64(mask, levels, None)
    memory, _ = EI.proposal_memory(4, 240, 8, 1)
    _, _, row_mask = MSDA.two_stage_proposals(memory.to(DEV), mask.to(DEV), levels, None)
    assert torch.equal(row_mask.cpu(), dead)
    go = torch.randn(4, 240, 6, generator=torch.Generator().manual_seed(2))
    want = go.masked_fill(dead.unsqueeze(-1), 0.0)
    ctx = types.SimpleNamespace(saved_tensors=(row_mask,), needs_input_grad=(True, False, True, False), xy_shape=(40,))
    n0 = MSDA.launch_count()
    gm, _, gxy, _ = TS._ProposalsFn.backward(ctx, go.to(DEV), None)
    assert torch.equal(gm.cpu(), want) and gxy.shape == (40,) and torch.count_nonzero(gxy) == 0
    _, _, a_mask = MSDA.assembly_proposals(memory.to(DEV), mask.to(DEV), levels[0])
    assert torch.equal(a_mask.cpu(), dead)
    ctx = types.SimpleNamespace(saved_tensors=(a_mask,), needs_input_grad=(True, False, False))
    gm, _, _ = AF._LevelProposalsFn.backward(ctx, go.to(DEV), None)
    assert torch.equal(gm.cpu(), want)
    assert MSDA.launch_count() - n0 == 1                     # the assembly forward alone


# ---- selection ----------------------------------------------------------------------------------------------------------------
def _ids(cases):
    return ["%dx%dx%dx%d-%s-h%d" % (s + (l, hc[0])) for s, l, hc in cases]


@pytest.mark.parametrize("shape,logits,hc", EI.SELECT_CASES, ids=_ids(EI.SELECT_CASES))
def test_selection_against_stable_sort(shape, logits, hc):
    N, S, Q, K = shape
    c = EI.select_case(shape, logits, hc)
    host = (c["cls"], c["hand"], c["obj"], c["prop"])
    o_idx, o_ref, counts = EI.select_oracle(*host, Q, hc)
    assert all(counts[b] == 0 for b in EI.impossible_branches(shape, hc))
    assert sum(v > 0 for v in counts.values()) == EI.branches_selected(shape, hc)          # every reachable source is read
    dev = [t.to(DEV) for t in host]
    n0 = MSDA.launch_count()
    ref, refp, idx = TS.select_queries(*dev, Q, hand_classes=hc, return_indices=True)
    assert MSDA.launch_count() - n0 == (1 if Q else 0)
    assert idx.dtype == torch.int64 and idx.shape == (N, Q) and ref.shape == (N, Q, 42) and refp.shape == (N, Q, 42)
    assert torch.equal(idx.cpu(), o_idx)
    # a gather: bitwise, NaN-free sources, so == on the bits
    assert torch.equal(ref.cpu().view(torch.int32), o_ref.view(torch.int32))
    assert torch.equal(refp, ref.sigmoid() * 2 - 1)
    if Q == S:                                               # every real row once: no padding key was selected
        assert torch.equal(torch.sort(idx, dim=1)[0].cpu(), torch.arange(S)[None, :].expand(N, S))


def test_selection_above_8192_rows_takes_the_composition():
    g = torch.Generator().manual_seed(1)
    big = [torch.randn(1, 8193, k, generator=g).to(DEV) for k in (14, 42, 42, 42)]
    assert not MSDA.two_stage_select_supported(8193, 14, 300) and MSDA.two_stage_select_supported(8192, 14, 8192)
    n0 = MSDA.launch_count()
    ref, refp, idx = TS.select_queries(*big, 300, return_indices=True)
    assert MSDA.launch_count() == n0
    c_ref, c_refp = TS.select_composition(*big, 300)
    o_idx, o_ref, _ = EI.select_oracle(*(t.cpu() for t in big), 300, TS.HAND_CLASSES)
    assert torch.equal(ref, c_ref) and torch.equal(refp, c_refp) and torch.equal(idx.cpu(), o_idx) and torch.equal(ref.cpu(), o_ref)
    with pytest.raises(RuntimeError):
        TS.select_queries(*big, 8194)


# ---- embedding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", EI.PE_ROWS)
def test_pe_special_rows_against_fp64(M):
    r = EI.pe_rows(M)
    ref = EI.pe_f64(r)
    n0 = MSDA.launch_count()
    pe = TS.proposal_pos_embed(r.to(DEV).view(1, M, 42))
    assert MSDA.launch_count() - n0 == 1 and pe.shape == (1, M, 5376)
    got = pe.view(M, -1).cpu().double()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan) and bool(nan.any()) and not bool(torch.isinf(got).any())
    dev = (got - ref)[~nan].abs().max().item()
    dev32 = (TS.pos_embed_composition(r).double() - ref)[~nan].abs().max().item()
    print("MEASURED pe M=%d: kernel %.2e composition %.2e" % (M, dev, dev32))
    assert dev <= EI.PE_BOUND


# ---- fused node ---------------------------------------------------------------------------------------------------------------
def _node_run(c, bias):
    """One forward and backward through _PosEmbedLinearReluFn: (y, grad_w, grad_b or None) on the device."""
    w = c["w"].to(DEV).requires_grad_(True)
    b = c["b"].to(DEV).requires_grad_(True) if bias else None
    dim_t = TS.pe_dim_t(DEV)[0::2].contiguous()
    n0 = MSDA.launch_count()
    y = TS._PosEmbedLinearReluFn.apply(c["r"].to(DEV), dim_t, w, b)
    assert MSDA.launch_count() - n0 == 1
    y.backward(c["gy"].to(DEV))
    return y.detach(), w.grad, b.grad if bias else None


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,Nc", EI.NODE_CASES)
def test_fused_node_against_fp64(M, Nc, bias):
    c = EI.node_case(M, Nc)
    y, gw, gb = _node_run(c, bias)
    assert y.shape == (M, Nc) and gw.shape == (Nc, 5376) and (gb is None) == (not bias)
    ref = EI.node_f64(c["r"], c["w"], c["b"] if bias else None, c["gy"], (y > 0).cpu())
    dev32, _ = EI.node_dev32(M, Nc, bias)
    failed = []
    for name, got in (("y", y), ("grad_w", gw), ("grad_b", gb)):
        if got is None:
            assert ref[name] is None and name not in dev32
            continue
        assert bool(torch.isfinite(got).all()), name
        kernel, bound = EI.rel_dev(got.cpu(), ref[name]), EI.node_bound(dev32[name])
        print("MEASURED node (%d, %d) %s %s: kernel %.2e dev32 %.2e ratio %.2f bound %.2e"
              % (M, Nc, "bias" if bias else "nobias", name, kernel, dev32[name], kernel / (dev32[name] + 1e-300), bound))
        if not kernel <= bound:
            failed.append((name, kernel, bound))
    assert not failed, failed
    again = _node_run(c, bias)
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip((y, gw, gb), again))   # bitwise reproducible


@pytest.mark.parametrize("M,Nc", EI.NODE_CASES)
def test_fused_node_writes_its_rows_only_and_keeps_nan_to_its_row(M, Nc):
    """The kernel's output as a slice of a filled buffer: what lies before and behind it keeps the fill (the column guard of
    the epilogue at a partial tile, the row guard at a partial row tile).  A NaN row of r is a NaN row of y and changes no
    other row by a bit."""
    c = EI.node_case(M, Nc)
    r, w, b = (c[k].to(DEV) for k in ("r", "w", "b"))
    dim_t = TS.pe_dim_t(DEV)[0::2].contiguous()
    clean = MSDA.proposal_pos_linear_relu(r, dim_t, w, b)
    fill = -7.0
    buf = torch.full((M + 2, Nc), fill, device=DEV)
    MSDA._launch(DEV, "msda_proposal_pos_linear_relu_f32", "proposal_pos_linear_relu", r.data_ptr(), dim_t.data_ptr(),
                 w.data_ptr(), b.data_ptr(), M, Nc, buf[1:].data_ptr())
    assert torch.equal(buf[1:M + 1], clean) and bool((buf[0] == fill).all()) and bool((buf[M + 1] == fill).all())
    assert bool((clean >= 0).all())
    bad = M // 2
    r_nan = r.clone()
    r_nan[bad, 17] = float("nan")
    y = MSDA.proposal_pos_linear_relu(r_nan, dim_t, w, b)
    assert bool(torch.isnan(y[bad]).all())
    keep = torch.arange(M, device=DEV) != bad
    assert torch.equal(y[keep], clean[keep])
