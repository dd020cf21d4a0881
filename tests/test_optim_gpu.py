"""uvhand_amd.optim on the GPU: clip(0.1) + AdamW as multi-tensor HIP launches against torch.optim.AdamW(foreach=False) +
clip_grad_norm_ on fp64 CPU copies.

The parity rule, for every tensor of param, exp_avg and exp_avg_sq: err = max|x - x64| / max|x64| may be at most 4 times the
same error of torch's own fp32 route (torch's clip_grad_norm_ + torch.optim.AdamW on the same device and inputs, computed
here).  The factor 4 is the margin for the fused form's different rounding order: it sums squares in a fixed tree order and
rounds the clipped gradient once.  The three steps' norms, taken as one tensor, are held to fp64 under the same rule against
torch.linalg.vector_norm in fp32.  Every figure is printed before it is asserted (pytest -s shows them).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_NORM = 0.1
STEPS = 3
VIEWS = (4, 7)          # (65,) and (c + 1,): views at an odd element offset into one buffer, 4-byte aligned
BIG = 9                 # (257, 33): its gradient is 1000 times the others'
LATE = 3                # (64,): a gradient from the second step on, so its own step count lags
NEVER = 11              # an extra (5,) parameter that never has a gradient
SEED = 20


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    return _native


def _shapes(c):
    return [(1,), (3,), (63,), (64,), (65,), (c - 1,), (c,), (c + 1,), (2 * c + 5,), (257, 33), (0,), (5,)]


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _make_inputs(c, seed):
    gen = torch.Generator().manual_seed(seed)
    shapes = _shapes(c)
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = []
    for step in range(STEPS):
        row = []
        for k, s in enumerate(shapes):
            if k == NEVER or (k == LATE and step == 0):
                row.append(None)
            else:
                row.append(torch.randn(s, generator=gen) * (1000.0 if k == BIG else 1.0))
        grads.append(row)
    return shapes, init, grads


@pytest.fixture(scope="module")
def inputs(native):
    """Initial values and the gradients of every step, fp32 on the CPU; made once, read by every test, never changed."""
    return _make_inputs(native.optim_chunk_elems(), SEED)


def _view_offsets(shapes):
    """Element offsets of the two views in their shared buffer, both = 1 mod 4, and the buffer's length."""
    first = 1
    second = first + _numel(shapes[VIEWS[0]])
    second += (1 - second) % 4
    return {VIEWS[0]: first, VIEWS[1]: second}, second + _numel(shapes[VIEWS[1]]) + 3


def _place(values, shapes, device, dtype, views):
    """The tensors of `values` (None entries kept) on `device`; with `views`, the two VIEWS tensors inside one fresh buffer."""
    out = [None if v is None else v.to(device=device, dtype=dtype).clone() for v in values]
    if views:
        offsets, length = _view_offsets(shapes)
        buf = torch.zeros(length, device=device, dtype=dtype)
        for k, off in offsets.items():
            if values[k] is not None:
                view = buf[off:off + _numel(shapes[k])].view(shapes[k])
                view.copy_(values[k])
                assert view.data_ptr() % 16 == 4 and view.is_contiguous()
                out[k] = view
    return out


def _groups(params):
    return [{"params": params[0::2], "lr": 1e-2, "weight_decay": 1e-2}, {"params": params[1::2], "lr": 3e-3, "weight_decay": 0.0}]


def _run(inputs, device, dtype, classes, views=False, fused_clip=None, onecycle=False, **kwargs):
    """STEPS steps of clip(MAX_NORM) + AdamW.  classes: the optimizer class of each step; a change of class hands the state over
    through state_dict().  fused_clip: per step, whether step(max_norm=) does the clip.  Returns (params, state per param, norms
    [STEPS], lr per step)."""
    shapes, init, grads = inputs
    params = [torch.nn.Parameter(t) for t in _place(init, shapes, device, dtype, views)]
    opt, sched, norms, lrs = None, None, [], []
    for step in range(STEPS):
        cls = classes[step]
        if opt is None or type(opt) is not cls:
            new = cls(_groups(params), **kwargs)
            if opt is not None:
                new.load_state_dict(opt.state_dict())
            opt = new
            if onecycle:
                sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[2e-2, 6e-3], total_steps=STEPS + 1,
                                                            last_epoch=step - 1 if step else -1)
        for p, g in zip(params, _place(grads[step], shapes, device, dtype, views)):
            p.grad = g
        lrs.append([g["lr"] for g in opt.param_groups])
        if fused_clip is not None and fused_clip[step]:
            opt.step(max_norm=MAX_NORM)
            norms.append(opt.last_grad_norm)
        else:
            norms.append(torch.nn.utils.clip_grad_norm_(params, MAX_NORM))
            opt.step()
        if sched is not None:
            sched.step()
    return params, [opt.state.get(p, {}) for p in params], torch.stack([n.detach().cpu() for n in norms]), lrs


def _err(x, x64):
    return float((x.detach().double().cpu() - x64.detach()).abs().max() / x64.detach().abs().max())


def _check_parity(what, ours, torch32, ref64):
    """The parity rule of the module's head over every tensor of param, exp_avg and exp_avg_sq; returns the worst ratio."""
    worst = 0.0
    for k, (p, q, r) in enumerate(zip(ours[0], torch32[0], ref64[0])):
        triples = [("param", p, q, r)]
        assert ours[1][k].keys() == torch32[1][k].keys() == ref64[1][k].keys(), k
        for name in ("exp_avg", "exp_avg_sq"):
            if name in ref64[1][k]:
                triples.append((name, ours[1][k][name], torch32[1][k][name], ref64[1][k][name]))
        if "step" in ref64[1][k]:
            assert float(ours[1][k]["step"]) == float(ref64[1][k]["step"]), k
        for name, a, b, r64 in triples:
            if r64.numel() == 0:
                continue
            e_ours, e_torch = _err(a, r64), _err(b, r64)
            ratio = e_ours / e_torch if e_torch else (float("inf") if e_ours else 0.0)
            print("%s tensor %2d %-10s ours %.3e torch %.3e ratio %.2f" % (what, k, name, e_ours, e_torch, ratio))
            worst = max(worst, ratio)
            assert e_ours <= 4.0 * e_torch, (what, k, name, e_ours, e_torch)
    return worst


@pytest.fixture(scope="module")
def references(inputs):
    """The fp64 reference and torch's own fp32 route, computed once."""
    ref64 = _run(inputs, "cpu", torch.float64, [torch.optim.AdamW] * STEPS, foreach=False)
    torch32 = _run(inputs, "cuda", torch.float32, [torch.optim.AdamW] * STEPS)
    return ref64, torch32


def _ours(inputs, **kwargs):
    from uvhand_amd.optim import AdamW
    kwargs.setdefault("classes", [AdamW] * STEPS)
    kwargs.setdefault("fused_clip", [True] * STEPS)
    return _run(inputs, "cuda", torch.float32, views=True, **kwargs)


def test_three_clipped_steps_against_fp64(native, inputs, references):
    ref64, torch32 = references
    n0 = native.launch_count()
    ours = _ours(inputs)
    assert native.launch_count() - n0 == 3 * STEPS                   # the kernels ran, three launches per clipped step
    assert float(ref64[2].min()) > 100 * MAX_NORM                    # the clip is active in every step
    assert ours[1][NEVER] == {} and float(ours[1][LATE]["step"]) == STEPS - 1
    assert torch.equal(ours[0][NEVER].cpu(), inputs[1][NEVER])       # no gradient: never touched
    _check_parity("parity", ours, torch32, ref64)
    # the norm of each step, the three taken as one tensor, against torch.linalg.vector_norm in fp32
    shapes, _, grads = inputs
    flat32 = torch.stack([torch.linalg.vector_norm(torch.cat([g.flatten() for g in row if g is not None]).cuda()).cpu()
                          for row in grads])
    e_ours, e_torch = _err(ours[2], ref64[2]), _err(flat32, ref64[2])
    print("norm ours %.3e torch %.3e ratio %.2f" % (e_ours, e_torch, e_ours / e_torch if e_torch else float("inf")))
    assert e_ours <= 4.0 * e_torch
    assert ours[2].dtype == torch.float32 and ours[2].shape == (STEPS,)


def test_clip_grad_norm_drop_in_is_g_times_coef_bit_for_bit(native, inputs):
    from uvhand_amd.optim import clip_grad_norm_, grad_norm
    shapes, init, grads = inputs
    for max_norm, clipped in ((MAX_NORM, True), (1e6, False)):
        params = [torch.nn.Parameter(t) for t in _place(init, shapes, "cuda", torch.float32, True)]
        placed = _place(grads[1], shapes, "cuda", torch.float32, True)
        before = [None if g is None else g.clone() for g in placed]
        for p, g in zip(params, placed):
            p.grad = g
        n0 = native.launch_count()
        alone = grad_norm(params)
        norm = clip_grad_norm_(params, max_norm)
        assert native.launch_count() - n0 == 2 + 3
        assert norm.dim() == 0 and norm.is_cuda and norm.dtype == torch.float32 and torch.equal(norm, alone)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)        # torch's formula on the returned norm, in fp32
        assert (float(coef) < 1.0) == clipped
        for k, (p, g0) in enumerate(zip(params, before)):
            if g0 is None:
                assert p.grad is None
            elif clipped:
                assert torch.equal(p.grad, g0 * coef), k
            else:
                assert torch.equal(p.grad, g0), k


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_poisons_what_torchs_route_poisons(native, inputs, bad):
    from uvhand_amd.optim import AdamW
    shapes, init, grads = inputs
    results = []
    for cls in (AdamW, torch.optim.AdamW):
        params = [torch.nn.Parameter(t) for t in _place(init, shapes, "cuda", torch.float32, cls is AdamW)]
        for p, g in zip(params, _place(grads[1], shapes, "cuda", torch.float32, cls is AdamW)):
            p.grad = g
        params[5].grad[17] = bad
        opt = cls(_groups(params))
        if cls is AdamW:
            n0 = native.launch_count()
            opt.step(max_norm=MAX_NORM)
            assert native.launch_count() - n0 == 3
            norm = opt.last_grad_norm
        else:
            norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
        results.append((params, norm))
    (ours, norm), (ref, ref_norm) = results
    assert torch.equal(norm.isnan(), ref_norm.isnan()) and (bool(norm.isnan()) or torch.equal(norm, ref_norm))
    poisoned = 0
    for k, (p, q) in enumerate(zip(ours, ref)):
        assert torch.equal(p.isnan(), q.isnan()), k
        poisoned += int(p.isnan().sum())
    # inf: the coefficient is 0 and 0 * inf poisons that one element; nan: every parameter with a gradient
    assert poisoned == (1 if bad == float("inf") else sum(_numel(s) for k, s in enumerate(shapes) if k != NEVER))


def test_the_same_steps_twice_give_the_same_bits(inputs):
    a, b = _ours(inputs), _ours(inputs)
    assert torch.equal(a[2], b[2])
    for k in range(len(a[0])):
        assert torch.equal(a[0][k], b[0][k]), k
        for name in ("exp_avg", "exp_avg_sq"):
            if name in a[1][k]:
                assert torch.equal(a[1][k][name], b[1][k][name]), (k, name)


def test_launches_and_host_syncs_do_not_grow_with_the_tensors(native):
    from uvhand_amd.optim import AdamW
    gen = torch.Generator().manual_seed(5)
    sizes = [1 + (37 * k) % 300 for k in range(40)]
    params = [torch.nn.Parameter(torch.randn(n, generator=gen).cuda()) for n in sizes]
    opt = AdamW([{"params": params[:20]}, {"params": params[20:], "lr": 1e-4}], lr=1e-3)

    def fresh_grads(keep):
        for p in params:
            p.grad = torch.randn_like(p)                            # freshly allocated; the old ones stay alive in `keep`
            keep.append(p.grad)

    keep = []
    fresh_grads(keep)
    opt.step(max_norm=MAX_NORM)                                     # warm-up: builds the tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            fresh_grads(keep)
            n0 = native.launch_count()
            opt.step(max_norm=MAX_NORM)
            assert native.launch_count() - n0 <= 3
            assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda
        fresh_grads(keep)
        n0 = native.launch_count()
        opt.step()
        assert native.launch_count() - n0 == 1
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len({g.data_ptr() for g in keep}) == len(keep)           # the gradients' addresses did change every step
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert float(opt.state[params[0]]["step"]) == 5


def test_checkpoints_move_between_this_class_and_torchs(inputs, references):
    from uvhand_amd.optim import AdamW
    ref64, torch32 = references
    T = torch.optim.AdamW
    there = _ours(inputs, classes=[AdamW, AdamW, T], fused_clip=[True, True, False])
    _check_parity("ours -> torch", there, torch32, ref64)
    back = _ours(inputs, classes=[T, T, AdamW], fused_clip=[False, False, True])
    _check_parity("torch -> ours", back, torch32, ref64)


def test_one_cycle_lr_steps_between_the_optimizer_steps(inputs):
    ref64 = _run(inputs, "cpu", torch.float64, [torch.optim.AdamW] * STEPS, onecycle=True, foreach=False)
    torch32 = _run(inputs, "cuda", torch.float32, [torch.optim.AdamW] * STEPS, onecycle=True)
    ours = _ours(inputs, onecycle=True)
    assert ours[3] == torch32[3] == ref64[3]                         # the lr sequence torch's optimizer sees, both groups
    assert len({tuple(row) for row in ours[3]}) == STEPS             # and it does move
    _check_parity("onecycle", ours, torch32, ref64)


def test_amsgrad_falls_back_without_a_library_launch(native, inputs):
    from uvhand_amd.optim import AdamW
    n0 = native.launch_count()
    ours = _run(inputs, "cuda", torch.float32, [AdamW] * STEPS, fused_clip=[True] * STEPS, amsgrad=True)
    assert native.launch_count() == n0
    ref = _run(inputs, "cuda", torch.float32, [torch.optim.AdamW] * STEPS, amsgrad=True)
    assert torch.equal(ours[2], ref[2])
    for k in range(len(ours[0])):
        assert torch.equal(ours[0][k], ref[0][k]), k
        assert ours[1][k].keys() == ref[1][k].keys()
        for name in ours[1][k]:
            assert torch.equal(ours[1][k][name], ref[1][k][name]), (k, name)
