"""uvhand_amd.optim.AdamW(capturable=True) on the GPU: the device-state form of clip(0.1) + AdamW, eagerly and as a replayed HIP
graph, against the non-capturable route of the same class (bit for bit: the two run the same arithmetic) and against fp64.

The fp64 parity rule (restated from tests/test_optim_gpu.py, whose margin it keeps), for every tensor of param, exp_avg and
exp_avg_sq: err = max|x - x64| / max|x64| may be at most 4 times the same error of torch's own fp32 route (torch's clip_grad_norm_
+ torch.optim.AdamW on the same device and inputs, computed here).  The factor 4 is the margin for the fused form's different
rounding order: it sums squares in a fixed tree order and rounds the clipped gradient once.  Every ratio is printed before it is
asserted (pytest -s shows them).

Capture hygiene (uvhand_amd/graphs.py: this PyTorch-ROCm build crashes in capture_end otherwise): before every capture earlier
losses are dropped, garbage is collected and the device is synchronised; warm-up steps and captures run on a side stream, as
torch's recipe does; only linear chains are captured, and no capture is left empty.
"""
import contextlib
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_NORM = 0.1
VIEWS = (1, 4)          # (3,) and (c + 1,): views at an element offset of 1 mod 4 into one buffer, so 4-byte aligned only
BIG = 7                 # (257, 33): its gradient is 1000 times the others'
LATE = 0                # test 1: (1,) gets its first gradient in step 2, so its own step count lags
SEED = 31
ROWS = 6                # rows of gradients made once: the longest test takes six steps
MAX_LR = [2e-2, 6e-3, 2e-3]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    return _native


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


@pytest.fixture(scope="module")
def inputs(native):
    """Shapes, initial values and ROWS rows of gradients (and of the element-wise model's x), fp32 on the CPU; made once, read
    by every test, never changed."""
    c = native.optim_chunk_elems()
    shapes = [(1,), (3,), (c - 1,), (c,), (c + 1,), (2 * c + 5,), (0,), (257, 33)]
    gen = torch.Generator().manual_seed(SEED)
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[torch.randn(s, generator=gen) * (1000.0 if k == BIG else 1.0) for k, s in enumerate(shapes)] for _ in range(ROWS)]
    xs = [[torch.randn(s, generator=gen) * (1000.0 ** 0.5 if k == BIG else 1.0) for k, s in enumerate(shapes)] for _ in range(ROWS)]
    return shapes, init, grads, xs


def _place(values, shapes, device="cuda", dtype=torch.float32, views=True):
    """The tensors of `values` on `device`; with `views`, the two VIEWS tensors inside one fresh buffer at offsets = 1 mod 4."""
    out = [v.to(device=device, dtype=dtype).clone() for v in values]
    if views:
        first = 1
        second = first + _numel(shapes[VIEWS[0]])
        second += (1 - second) % 4
        buf = torch.zeros(second + _numel(shapes[VIEWS[1]]) + 3, device=device, dtype=dtype)
        for k, off in zip(VIEWS, (first, second)):
            view = buf[off:off + _numel(shapes[k])].view(shapes[k])
            view.copy_(values[k])
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            out[k] = view
    return out


def _groups(params):
    """Three groups with distinct lr and weight_decay, one weight_decay = 0."""
    return [{"params": params[0::3], "lr": 1e-2, "weight_decay": 1e-2}, {"params": params[1::3], "lr": 3e-3, "weight_decay": 0.0},
            {"params": params[2::3], "lr": 1e-3, "weight_decay": 5e-2}]


def _fresh(inputs, capturable, cls=None, **kwargs):
    """(params, static gradient buffers, optimizer): parameters and buffers placed with the two views."""
    from uvhand_amd.optim import AdamW
    shapes, init = inputs[0], inputs[1]
    params = [torch.nn.Parameter(t) for t in _place(init, shapes)]
    bufs = _place([torch.zeros(s) for s in shapes], shapes)
    opt = (cls or AdamW)(_groups(params), capturable=capturable, **kwargs)
    return params, bufs, opt


def _load(params, bufs, row, skip=()):
    """Refresh the static gradient buffers with copy_ and make them the gradients (None for the parameters in `skip`)."""
    for k, (p, b, g) in enumerate(zip(params, bufs, row)):
        if k in skip:
            p.grad = None
            continue
        b.copy_(g)
        p.grad = b


def _one_cycle(opt, steps):
    return torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=MAX_LR, total_steps=steps + 1)      # cycle_momentum: the default, on


def _snapshot(params, opt):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append({"param": p.detach().clone(), "exp_avg": st["exp_avg"].clone() if st else None,
                    "exp_avg_sq": st["exp_avg_sq"].clone() if st else None, "step": float(st["step"]) if st else None})
    return out


def _assert_same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert a["step"] == b["step"], (what, k, a["step"], b["step"])
        for name in ("param", "exp_avg", "exp_avg_sq"):
            if b[name] is None:
                assert a[name] is None, (what, k, name)
            else:
                assert torch.equal(a[name], b[name]), (what, k, name)


@contextlib.contextmanager
def _side_stream():
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        yield side
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def _capture(side, fn):
    """fn captured on the side stream into a new graph, after the hygiene of the module's head."""
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    return graph


def _eager(inputs, rows, capturable=False, one_cycle=False, late=False, lrs=None, nan_at=None, skip_nonfinite=False):
    """Eager steps of clip(MAX_NORM) + AdamW over the gradient rows `rows`.  lrs: per step, a factor on every group's initial lr.
    nan_at: the step before which a NaN is written into one gradient.  Returns (snapshot, norms, launches per step, optimizer)."""
    from uvhand_amd import _native
    params, bufs, opt = _fresh(inputs, capturable)
    base = [g["lr"] for g in opt.param_groups]
    sched = _one_cycle(opt, len(rows)) if one_cycle else None
    norms, launches = [], []
    for i, r in enumerate(rows):
        _load(params, bufs, inputs[2][r], skip=(LATE,) if late and i == 0 else ())
        if lrs is not None:
            for g, lr in zip(opt.param_groups, base):
                g["lr"] = lr * lrs[i]
        if nan_at == i:
            bufs[2][17] = float("nan")
        n0 = _native.launch_count()
        if skip_nonfinite:
            opt.step(max_norm=MAX_NORM, skip_nonfinite=True)
        else:
            opt.step(max_norm=MAX_NORM)
        launches.append(_native.launch_count() - n0)
        norms.append(opt.last_grad_norm.clone())
        if sched is not None:
            sched.step()
    return _snapshot(params, opt), torch.stack(norms), launches, opt


def _warm_up(inputs, rows, one_cycle_steps=None, **kwargs):
    """A capturable instance after eager warm-up steps over `rows` (on the current stream), its hyper table refreshed."""
    params, bufs, opt = _fresh(inputs, True, **kwargs)
    sched = _one_cycle(opt, one_cycle_steps) if one_cycle_steps else None
    norms = []
    for r in rows:
        _load(params, bufs, inputs[2][r])
        opt.step(max_norm=MAX_NORM)
        norms.append(opt.last_grad_norm.clone())
        if sched is not None:
            sched.step()
    opt.refresh_hyper()
    return params, bufs, opt, sched, norms


def test_eager_device_state_equals_the_host_state_route(native, inputs):
    want, want_norms, want_launches, _ = _eager(inputs, range(4), capturable=False, one_cycle=True, late=True)
    got, norms, launches, opt = _eager(inputs, range(4), capturable=True, one_cycle=True, late=True)
    assert launches == [3] * 4 and want_launches == [3] * 4
    assert float(want_norms.min()) > 100 * MAX_NORM                   # the clip acts in every step
    _assert_same(got, want, "eager")
    assert got[LATE]["step"] == 3.0 and got[BIG]["step"] == 4.0      # the late parameter's own count lags
    assert torch.equal(norms, want_norms)
    for p in opt.state:
        step = opt.state[p]["step"]
        assert step.is_cuda and step.dtype == torch.float32 and step.dim() == 0     # torch's capturable state
    assert int(opt.skipped_steps) == 0
    # an unclipped step over the same gradients: advance + update
    n0 = native.launch_count()
    opt.step()
    assert native.launch_count() - n0 == 2


def test_replays_of_a_captured_step_equal_eager_steps(native, inputs):
    """Fails on the parent commit: there the capture raises (torch's 'capturable is False', or no device-state form at all)."""
    want, want_norms, _, _ = _eager(inputs, range(6), capturable=False, one_cycle=True)
    with _side_stream() as side:
        params, bufs, opt, sched, norms = _warm_up(inputs, range(2), one_cycle_steps=6)
        _load(params, bufs, inputs[2][2])
        n0 = native.launch_count()
        graph = _capture(side, lambda: opt.step(max_norm=MAX_NORM))
        assert native.launch_count() - n0 == 3                        # the capture enqueued exactly the three launches
        for r in range(2, 6):
            _load(params, bufs, inputs[2][r])
            graph.replay()
            norms.append(opt.last_grad_norm.clone())                  # static memory, refreshed by every replay
            sched.step()
            assert opt.refresh_hyper() is True                        # OneCycleLR moved lr and beta1
        assert native.launch_count() - n0 == 3                        # replays enqueue nothing through the library
    _assert_same(_snapshot(params, opt), want, "replay")
    assert torch.equal(torch.stack(norms), want_norms)


def test_torchs_whole_network_recipe(native, inputs):
    """zero_grad(set_to_none=True), then forward + backward + step(max_norm) in one capture: the gradients are allocated from the
    graph's pool, at addresses the optimizer has never seen.  The model is element-wise, so eager and captured gradients are the
    same bits."""
    shapes, _, _, xs = inputs

    def run(capturable):
        params, _, opt = _fresh(inputs, capturable)
        x = _place([torch.zeros(s) for s in shapes], shapes, views=False)

        def step():
            loss = sum(((p * xk) ** 2).sum() for p, xk in zip(params, x))
            loss.backward()
            opt.step(max_norm=MAX_NORM)

        def set_x(r):
            for xk, v in zip(x, xs[r]):
                xk.copy_(v)

        norms = []
        if not capturable:
            for r in range(5):
                set_x(r)
                opt.zero_grad(set_to_none=True)
                step()
                norms.append(opt.last_grad_norm.clone())
            return _snapshot(params, opt), torch.stack(norms)
        with _side_stream() as side:
            for r in range(2):
                set_x(r)
                opt.zero_grad(set_to_none=True)
                step()
                norms.append(opt.last_grad_norm.clone())
            opt.zero_grad(set_to_none=True)
            n0 = native.launch_count()
            graph = _capture(side, step)
            assert native.launch_count() - n0 == 3
            for r in range(2, 5):
                set_x(r)
                graph.replay()
                norms.append(opt.last_grad_norm.clone())
        return _snapshot(params, opt), torch.stack(norms)

    want, want_norms = run(False)
    got, norms = run(True)
    assert float(want_norms.min()) > 100 * MAX_NORM
    _assert_same(got, want, "whole network")
    assert torch.equal(norms, want_norms)


def test_a_replay_keeps_the_old_hyperparameters_until_refresh_hyper(native, inputs):
    stale, _, _, _ = _eager(inputs, range(4), lrs=[1.0, 1.0, 1.0, 1.0])
    fresh, _, _, _ = _eager(inputs, range(5), lrs=[1.0, 1.0, 1.0, 1.0, 3.0])
    with _side_stream() as side:
        params, bufs, opt, _, _ = _warm_up(inputs, range(2))
        _load(params, bufs, inputs[2][2])
        graph = _capture(side, lambda: opt.step(max_norm=MAX_NORM))
        graph.replay()
        for g in opt.param_groups:
            g["lr"] = g["lr"] * 3.0
        _load(params, bufs, inputs[2][3])
        graph.replay()                                                # no refresh_hyper(): the device table still has the old lr
        torch.cuda.synchronize()
        _assert_same(_snapshot(params, opt), stale, "stale lr")
        assert opt.refresh_hyper() is True and opt.refresh_hyper() is False
        _load(params, bufs, inputs[2][4])
        graph.replay()
    _assert_same(_snapshot(params, opt), fresh, "refreshed lr")


@pytest.mark.parametrize("skip_nonfinite", [True, False])
def test_a_non_finite_norm_skips_the_step_or_poisons_it(native, inputs, skip_nonfinite):
    """Replays over rows 2, 3, 4, 5 with a NaN written into one static gradient before the second (data, not a fault)."""
    with _side_stream() as side:
        params, bufs, opt, _, _ = _warm_up(inputs, range(2))
        _load(params, bufs, inputs[2][2])
        if skip_nonfinite:
            graph = _capture(side, lambda: opt.step(max_norm=MAX_NORM, skip_nonfinite=True))
        else:
            graph = _capture(side, lambda: opt.step(max_norm=MAX_NORM))
        for i, r in enumerate(range(2, 6)):
            _load(params, bufs, inputs[2][r])
            if i == 1:
                bufs[2][17] = float("nan")
                torch.cuda.synchronize()
                before = _snapshot(params, opt)
            graph.replay()
            if i == 1:
                torch.cuda.synchronize()
                after = _snapshot(params, opt)
                assert bool(opt.last_grad_norm.isnan())
    if skip_nonfinite:
        _assert_same(after, before, "skipped replay")                 # no parameter, moment or step moved
        assert int(opt.skipped_steps) == 1 and opt.skipped_steps.dtype == torch.int32 and opt.skipped_steps.is_cuda
        want, _, _, _ = _eager(inputs, [0, 1, 2, 4, 5])               # the other three replays: three more eager steps
        _assert_same(_snapshot(params, opt), want, "around the skip")
        # the same eagerly
        eager, _, _, eager_opt = _eager(inputs, range(6), capturable=True, nan_at=3, skip_nonfinite=True)
        _assert_same(eager, want, "eager skip")
        assert int(eager_opt.skipped_steps) == 1
    else:
        assert int(opt.skipped_steps) == 0
        want, _, _, _ = _eager(inputs, range(6), nan_at=3)            # what the present route poisons
        got = _snapshot(params, opt)
        poisoned = 0
        for k, (a, b) in enumerate(zip(got, want)):
            assert a["step"] == b["step"] == 6.0, k
            for name in ("param", "exp_avg", "exp_avg_sq"):
                assert torch.equal(a[name].isnan(), b[name].isnan()), (k, name)
            poisoned += int(a["param"].isnan().sum())
        assert poisoned == sum(_numel(s) for s in inputs[0])          # a NaN coefficient reaches every parameter


def test_refusals_under_a_capture_and_what_stays_on_torchs_route(native, inputs, monkeypatch):
    from uvhand_amd.optim import AdamW
    tick = torch.zeros(1, device="cuda")

    def refused(opt, match):
        """The step raises inside a capture (kept non-empty by one add) and enqueues no library launch."""
        n0 = native.launch_count()
        with pytest.raises(RuntimeError, match=match):
            def body():
                tick.add_(1)
                opt.step(max_norm=MAX_NORM)
            _capture(side, body)
        assert native.launch_count() == n0

    with _side_stream() as side:
        # a missing warm-up
        params, bufs, opt = _fresh(inputs, True)
        _load(params, bufs, inputs[2][0])
        refused(opt, "warm-up")
        assert all(len(opt.state[p]) == 0 for p in params)
        # a hyper shadow that differs from param_groups
        params, bufs, opt, _, _ = _warm_up(inputs, range(1))
        opt.param_groups[1]["lr"] = 7e-3
        before = _snapshot(params, opt)
        refused(opt, r"refresh_hyper\(\)")
        _assert_same(_snapshot(params, opt), before, "refused")
        # a non-capturable instance: torch's route and torch's own error, as before
        params, bufs, opt = _fresh(inputs, False)
        _load(params, bufs, inputs[2][0])
        opt.step(max_norm=MAX_NORM)
        refused(opt, "capturable is False")

    # mixed capturable groups and MSDA_OPTIM_FUSED=0 stay on torch's route: no library launch, torch's bits
    def torch_route(make):
        results = []
        for cls in (AdamW, torch.optim.AdamW):
            params, bufs, opt = _fresh(inputs, True, cls=cls)
            make(opt)
            n0 = native.launch_count()
            for r in range(2):
                _load(params, bufs, inputs[2][r])
                if cls is AdamW:
                    opt.step(max_norm=MAX_NORM)
                    assert opt.refresh_hyper() is False
                else:
                    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                    opt.step()
            assert native.launch_count() == n0
            results.append(_snapshot(params, opt))
        _assert_same(results[0], results[1], "torch's route")

    def mixed(opt):
        opt.param_groups[1]["capturable"] = False
    torch_route(mixed)
    monkeypatch.setenv("MSDA_OPTIM_FUSED", "0")
    torch_route(lambda opt: None)


def _err(x, x64):
    return float((x.detach().double().cpu() - x64.detach()).abs().max() / x64.detach().abs().max())


def _chain(inputs, device, dtype, classes):
    """Three steps of clip(MAX_NORM) + AdamW; classes: per step (class, kwargs).  A change of class hands the state over through
    state_dict() / load_state_dict().  This package's class clips inside step(max_norm=)."""
    from uvhand_amd.optim import AdamW
    shapes, init, grads = inputs[0], inputs[1], inputs[2]
    views = device == "cuda"
    params = [torch.nn.Parameter(t) for t in _place(init, shapes, device, dtype, views)]
    opt = None
    for step, (cls, kwargs) in enumerate(classes):
        if opt is None or type(opt) is not cls:
            new = cls(_groups(params), **kwargs)
            if opt is not None:
                new.load_state_dict(opt.state_dict())
            opt = new
        for p, g in zip(params, _place(grads[step], shapes, device, dtype, views)):
            p.grad = g
        if cls is AdamW:
            opt.step(max_norm=MAX_NORM)
        else:
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
    return _snapshot(params, opt)


def test_checkpoints_move_to_and_from_torchs_capturable_class_within_fp64_parity(native, inputs):
    from uvhand_amd.optim import AdamW
    T = torch.optim.AdamW
    ref64 = _chain(inputs, "cpu", torch.float64, [(T, {"foreach": False})] * 3)
    torch32 = _chain(inputs, "cuda", torch.float32, [(T, {"capturable": True})] * 3)
    ours, theirs = (AdamW, {"capturable": True}), (T, {"capturable": True})
    n0 = native.launch_count()
    chains = {"torch -> ours -> torch": _chain(inputs, "cuda", torch.float32, [theirs, ours, theirs]),
              "ours -> torch -> ours": _chain(inputs, "cuda", torch.float32, [ours, theirs, ours])}
    assert native.launch_count() - n0 == 3 * 3                        # every step of this class ran the device-state kernels
    failures = []
    for what, got in chains.items():
        for k, (a, b, r) in enumerate(zip(got, torch32, ref64)):
            assert a["step"] == b["step"] == r["step"] == 3.0, (what, k)
            for name in ("param", "exp_avg", "exp_avg_sq"):
                if r[name].numel() == 0:
                    continue
                e_ours, e_torch = _err(a[name], r[name]), _err(b[name], r[name])
                ratio = e_ours / e_torch if e_torch else (float("inf") if e_ours else 0.0)
                print("%s tensor %d %-10s ours %.3e torch %.3e ratio %.2f" % (what, k, name, e_ours, e_torch, ratio))
                if not e_ours <= 4.0 * e_torch:
                    failures.append((what, k, name, e_ours, e_torch))
    assert not failures, failures
