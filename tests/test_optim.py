"""uvhand_amd.optim without a GPU: where the kernels do not apply (CPU parameters, amsgrad, MSDA_OPTIM_FUSED=0) the drop-ins
are torch's own functions bit for bit and the library launches nothing, and the optimizer's state is exactly torch's."""
import pytest
import torch

SHAPES = [(5, 3), (7,), (1,), (2, 3, 4)]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    return _native


def _params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]


def _groups(params):
    return [{"params": params[:2], "lr": 1e-2, "weight_decay": 1e-2}, {"params": params[2:], "lr": 1e-3, "weight_decay": 0.0}]


def _run(native, monkeypatch, env=None, **kwargs):
    from uvhand_amd.optim import AdamW
    if env is not None:
        monkeypatch.setenv("MSDA_OPTIM_FUSED", env)
    a, b = _params(), _params()
    ours, ref = AdamW(_groups(a), **kwargs), torch.optim.AdamW(_groups(b), **kwargs)
    n0 = native.launch_count()
    g = torch.Generator().manual_seed(4)
    for step in range(3):
        for k, (x, y) in enumerate(zip(a, b)):
            if k == 1 and step == 0:
                x.grad = y.grad = None                       # a gradient from the second step on: its own step count lags
                continue
            grad = torch.randn(x.shape, generator=g) * (1000.0 if k == 0 else 1.0)
            x.grad, y.grad = grad.clone(), grad.clone()
        ours.step(max_norm=0.1)
        norm = torch.nn.utils.clip_grad_norm_(b, 0.1)
        ref.step()
        assert torch.equal(ours.last_grad_norm, norm)
        for x, y in zip(a, b):                               # this route scales .grad as torch's clip does
            assert (x.grad is None and y.grad is None) or torch.equal(x.grad, y.grad)
    assert native.launch_count() == n0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    return ours, ref


def _same_state(sa, sb):
    assert sa["param_groups"] == sb["param_groups"]
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert list(sa["state"][k]) == list(sb["state"][k]), k
        for name, t in sa["state"][k].items():
            u = sb["state"][k][name]
            assert t.dtype == u.dtype and t.device == u.device and t.shape == u.shape and torch.equal(t, u), (k, name)


def test_cpu_parameters_are_torch_bit_for_bit(native, monkeypatch):
    ours, ref = _run(native, monkeypatch)
    _same_state(ours.state_dict(), ref.state_dict())


def test_amsgrad_is_torch_bit_for_bit(native, monkeypatch):
    ours, ref = _run(native, monkeypatch, amsgrad=True)
    _same_state(ours.state_dict(), ref.state_dict())
    assert "max_exp_avg_sq" in ours.state_dict()["state"][0]


def test_switched_off_is_torch_bit_for_bit(native, monkeypatch):
    ours, ref = _run(native, monkeypatch, env="0")
    _same_state(ours.state_dict(), ref.state_dict())


def test_state_dict_keys_and_dtypes_equal_torchs(native, monkeypatch):
    ours, ref = _run(native, monkeypatch)
    state = ours.state_dict()["state"]
    assert sorted(state) == [0, 1, 2, 3]
    for k, entry in state.items():
        assert list(entry) == ["step", "exp_avg", "exp_avg_sq"]
        assert entry["step"].dtype == torch.float32 and entry["step"].device.type == "cpu" and entry["step"].dim() == 0
        assert entry["exp_avg"].dtype == torch.float32 and entry["exp_avg_sq"].shape == torch.Size(SHAPES[k])
    assert float(state[0]["step"]) == 3 and float(state[1]["step"]) == 2
    # and the checkpoint loads into torch's class and back
    other = torch.optim.AdamW(_groups(_params()))
    other.load_state_dict(ours.state_dict())
    _same_state(other.state_dict(), ref.state_dict())
    ours.load_state_dict(ref.state_dict())
    _same_state(ours.state_dict(), ref.state_dict())


def test_clip_grad_norm_on_cpu_is_torchs(native):
    from uvhand_amd.optim import clip_grad_norm_, grad_norm
    a, b = _params(), _params()
    for x, y in zip(a, b):
        x.grad = torch.full_like(x, 2.0)
        y.grad = torch.full_like(y, 2.0)
    n0 = native.launch_count()
    assert torch.equal(grad_norm(a), torch.nn.utils.get_total_norm([y.grad for y in b]))
    for kwargs in ({}, {"norm_type": 1.0}, {"norm_type": float("inf")}, {"foreach": False}):
        assert torch.equal(clip_grad_norm_(a, 0.5, **kwargs), torch.nn.utils.clip_grad_norm_(b, 0.5, **kwargs))
        for x, y in zip(a, b):
            assert torch.equal(x.grad, y.grad)
    assert torch.equal(clip_grad_norm_(a[0], 0.5), torch.nn.utils.clip_grad_norm_(b[0], 0.5))      # a single tensor
    with pytest.raises(RuntimeError, match="non-finite"):
        a[0].grad[0, 0] = float("inf")
        clip_grad_norm_(a, 0.5, error_if_nonfinite=True)
    assert native.launch_count() == n0


def test_hooks_run_once_and_schedulers_see_the_step(native):
    from uvhand_amd.optim import AdamW
    params = _params()
    opt = AdamW(params, lr=1e-3)
    calls = []
    opt.register_step_post_hook(lambda *a: calls.append(1))
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.01, total_steps=5)
    ref_params = _params()
    ref = torch.optim.AdamW(ref_params, lr=1e-3)
    ref_sched = torch.optim.lr_scheduler.OneCycleLR(ref, max_lr=0.01, total_steps=5)
    for _ in range(4):
        for p in params:
            p.grad = torch.ones_like(p)
        opt.step(max_norm=0.1)
        sched.step()
        for p in ref_params:
            p.grad = torch.ones_like(p)
        ref.step()
        ref_sched.step()
        assert opt.param_groups[0]["lr"] == ref.param_groups[0]["lr"]
    assert len(calls) == 4
