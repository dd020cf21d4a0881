"""uvhand_amd.optim.AdamW(capturable=True) where there is no GPU: on CPU parameters the class is torch.optim.AdamW(capturable=
True) itself, whatever that does, and the library launches nothing.

What torch does there depends on its version: torch.optim.AdamW(capturable=True) either updates CPU parameters or refuses them
with an AssertionError ("... must be on supported devices", torch 2.10).  The tests below therefore run both classes through the
same three steps and hold this class to torch's outcome: the same exceptions, the same state and the same bits.  The state that
the device-state form itself creates is compared with torch's on the GPU (tests/test_optim_capture_gpu.py)."""
import pytest
import torch

STEPS = 3
SHAPES = [(1,), (7,), (33, 5), (0,)]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    return _native


def _three_steps(cls):
    """(optimizer, params, what each step did: None or (exception type, message))."""
    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in SHAPES]
    opt = cls([{"params": params[:2], "lr": 1e-2, "weight_decay": 1e-2}, {"params": params[2:], "lr": 3e-3, "weight_decay": 0.0}],
              capturable=True)
    outcomes = []
    for _ in range(STEPS):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen)
        try:
            opt.step()
            outcomes.append(None)
        except Exception as exc:                                      # noqa: BLE001 (whatever torch raises is the reference)
            outcomes.append((type(exc), str(exc)))
    return opt, params, outcomes


@pytest.fixture(scope="module")
def both(native):
    from uvhand_amd.optim import AdamW
    n0 = native.launch_count()
    ours = _three_steps(AdamW)
    launches = native.launch_count() - n0
    return ours, _three_steps(torch.optim.AdamW), launches


def test_cpu_parameters_are_torchs_route_bit_for_bit_without_a_launch(both):
    (opt, params, outcomes), (ref_opt, ref_params, ref_outcomes), launches = both
    assert launches == 0
    assert outcomes == ref_outcomes                                   # the same steps succeed, the same exceptions otherwise
    for k, (p, q) in enumerate(zip(params, ref_params)):
        assert torch.equal(p, q), k
        assert opt.state[p].keys() == ref_opt.state[q].keys(), k
        for name in opt.state[p]:
            assert torch.equal(opt.state[p][name], ref_opt.state[q][name]), (k, name)


def test_state_dict_has_torchs_keys_dtypes_and_devices(both):
    (opt, _, _), (ref_opt, _, _), _ = both
    sd, ref = opt.state_dict(), ref_opt.state_dict()
    assert sd.keys() == ref.keys() and sd["param_groups"] == ref["param_groups"]
    assert sd["state"].keys() == ref["state"].keys()
    for k in ref["state"]:                                            # whatever state torch got as far as creating
        assert sd["state"][k].keys() == ref["state"][k].keys(), k
        for name, t in ref["state"][k].items():
            mine = sd["state"][k][name]
            assert (mine.dtype, mine.device, mine.shape) == (t.dtype, t.device, t.shape), (k, name)
    # and a state_dict of torch's class loads into this one and back
    from uvhand_amd.optim import AdamW
    opt.load_state_dict(ref)
    ref_opt.load_state_dict(opt.state_dict())
    assert all(g["capturable"] for g in opt.param_groups)
    assert isinstance(opt, AdamW)


def test_refresh_hyper_is_a_no_op_off_the_device_state_route(both, native):
    from uvhand_amd.optim import AdamW
    (opt, _, _), _, _ = both
    n0 = native.launch_count()
    assert opt.refresh_hyper() is False
    opt.param_groups[0]["lr"] = 5e-2
    assert opt.refresh_hyper() is False                               # capturable, but CPU parameters: torch's route
    plain = AdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)      # not capturable
    assert plain.refresh_hyper() is False and plain.skipped_steps is None and opt.skipped_steps is None
    assert native.launch_count() == n0


def test_skip_nonfinite_is_refused_where_it_cannot_be_honoured(native):
    from uvhand_amd.optim import AdamW
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.ones(3)
    before = p.detach().clone()
    for kwargs in ({}, {"capturable": True}):
        opt = AdamW([p], lr=1e-3, **kwargs)
        with pytest.raises(RuntimeError, match="skip_nonfinite"):
            opt.step(max_norm=0.1, skip_nonfinite=True)
        assert torch.equal(p, before) and len(opt.state[p]) == 0     # refused before anything ran
