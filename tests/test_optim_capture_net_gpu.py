"""uvhand_amd.optim.AdamW(capturable=True) on the GPU, two cases tests/test_optim_capture_gpu.py does not reach:

* thousands of tensors: more than 256 (optim_advance_kernel then runs more than one workgroup) and more than 1024
  (norm_finish_dev_kernel's threads then go round their loop over the steps twice);
* torch's whole-network recipe on a network with matrix products: forward + backward + step(max_norm) in one capture, the
  gradients coming out of GEMMs on the autograd thread into the graph's pool, against the eager non-capturable loop, once with
  a new input copied in before every replay and once with the replays back to back and nothing between them.

Tolerance of the second case.  Eager and captured GEMMs may sum in another order, so their gradients may differ by a relative
delta of about K * 2^-24 (K <= 65 terms here: 4e-6).  One AdamW step moves an element by lr * m_hat / (sqrt(v_hat) + eps), of
size lr in these first steps, so such a delta moves the result by about lr * 1e-5 per step.  An optimizer that read a wrong
gradient table, a stale coefficient or a step count that did not advance is off by a fraction of lr per step in whole tensors.
The bound stands between the two: |difference| <= 1e-2 * lr * steps for every parameter, 1e-2 * steps for exp_avg relative to its
largest element, and 1e-4 relative for each step's loss and total norm (1e-4: 25 times the delta above).

Capture hygiene as in tests/test_optim_capture_gpu.py: earlier losses dropped, garbage collected, device synchronised, warm-up
and capture on a side stream, a linear chain.
"""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_NORM = 0.1
LR = 1e-2
STEPS = 6               # two eager warm-up steps and four replays
BATCH, D_IN, D_HID, D_OUT = 19, 33, 65, 17


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from uvhand_amd import _native
    _native.load()
    return _native


def _many(native, capturable, n):
    """n one-element parameters in two groups: three clipped steps, then two unclipped ones."""
    from uvhand_amd.optim import AdamW
    gen = torch.Generator().manual_seed(5)
    init, grads = torch.randn(n, generator=gen), torch.randn(5, n, generator=gen).cuda()
    params = [torch.nn.Parameter(v.reshape(1).clone().cuda()) for v in init]
    opt = AdamW([{"params": params[: n // 3], "lr": 1e-2}, {"params": params[n // 3:], "lr": 3e-3, "weight_decay": 0.0}],
                capturable=capturable)
    launches = []
    for i in range(5):
        for k, p in enumerate(params):
            p.grad = grads[i, k:k + 1]
        n0 = native.launch_count()
        if i < 3:
            opt.step(max_norm=MAX_NORM)
        else:
            opt.step()
        launches.append(native.launch_count() - n0)
    steps = torch.stack([opt.state[p]["step"].to("cuda", torch.float32) for p in params])
    return torch.cat([p.detach() for p in params]), steps, launches


def test_every_step_count_advances_with_thousands_of_tensors(native):
    n = 2500
    assert n > 2 * 1024 and native.optim_supported(n, 2)
    want, want_steps, want_launches = _many(native, False, n)
    got, steps, launches = _many(native, True, n)
    assert launches == [3, 3, 3, 2, 2] and want_launches == [3, 3, 3, 1, 1]
    assert torch.equal(steps, torch.full((n,), 5.0, device="cuda")) and torch.equal(want_steps, steps)
    assert torch.equal(got, want)


def _net():
    torch.manual_seed(11)
    return torch.nn.Sequential(torch.nn.Linear(D_IN, D_HID), torch.nn.Tanh(), torch.nn.Linear(D_HID, D_OUT)).cuda()


def _run_net(capturable, xs, back_to_back=False):
    """STEPS steps of the network.  back_to_back: the input stays xs[0] and the replays follow each other with nothing between
    them, no copy, no clone, no read; only the last step's loss and norm are returned then."""
    from uvhand_amd.optim import AdamW
    net = _net()
    params = list(net.parameters())
    opt = AdamW([{"params": params[:2], "lr": LR, "weight_decay": 1e-2}, {"params": params[2:], "lr": LR, "weight_decay": 0.0}],
                capturable=capturable)
    x = torch.zeros(BATCH, D_IN, device="cuda")
    losses, norms = [], []

    def step():
        loss = net(x).pow(2).sum()
        loss.backward()
        opt.step(max_norm=MAX_NORM)
        return loss

    def eager(r):
        x.copy_(xs[0 if back_to_back else r])
        opt.zero_grad(set_to_none=True)
        losses.append(step().detach().clone())
        norms.append(opt.last_grad_norm.clone())

    if not capturable:
        for r in range(STEPS):
            eager(r)
    else:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for r in range(2):
                eager(r)
            opt.zero_grad(set_to_none=True)
            gc.collect()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                static_loss = step()
            if back_to_back:
                torch.cuda.synchronize()
                for r in range(2, STEPS):
                    graph.replay()
                losses += [static_loss.detach().clone()] * (STEPS - 2)  # the graph's memory after the last replay
                norms += [opt.last_grad_norm.clone()] * (STEPS - 2)
            else:
                for r in range(2, STEPS):
                    x.copy_(xs[r])
                    graph.replay()
                    losses.append(static_loss.detach().clone())
                    norms.append(opt.last_grad_norm.clone())       # static memory, refreshed by every replay
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    state = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), float(opt.state[p]["step"])) for p in params]
    return state, torch.stack(losses), torch.stack(norms)


def test_whole_network_recipe_with_matrix_products_tracks_the_eager_loop(native):
    gen = torch.Generator().manual_seed(13)
    xs = torch.randn(STEPS, BATCH, D_IN, generator=gen).cuda()
    want, want_losses, want_norms = _run_net(False, xs)
    got, losses, norms = _run_net(True, xs)
    assert float(want_norms.min()) > 10 * MAX_NORM                    # the clip acts in every step
    print("loss  eager", want_losses.tolist(), "captured", losses.tolist())
    print("norm  eager", want_norms.tolist(), "captured", norms.tolist())
    for k, ((p, m, t), (p0, m0, t0)) in enumerate(zip(got, want)):
        dp, dm = float((p - p0).abs().max()), float((m - m0).abs().max() / m0.abs().max())
        print("tensor %d: |param difference| %.3e (bound %.3e), exp_avg %.3e (bound %.3e)" % (k, dp, 1e-2 * LR * STEPS, dm, 1e-2 * STEPS))
    torch.testing.assert_close(losses, want_losses, rtol=1e-4, atol=0.0)
    torch.testing.assert_close(norms, want_norms, rtol=1e-4, atol=0.0)
    for k, ((p, m, t), (p0, m0, t0)) in enumerate(zip(got, want)):
        assert t == t0 == float(STEPS), k
        assert float((p - p0).abs().max()) <= 1e-2 * LR * STEPS, k
        assert float((m - m0).abs().max() / m0.abs().max()) <= 1e-2 * STEPS, k


def test_replays_back_to_back_with_nothing_between_them_track_the_eager_loop(native):
    """The replay loop of a run without a moving schedule: graph.replay() four times in a row on a fixed input, nothing enqueued
    between two replays.  Each replay's forward must see the update of the one before; the end state is held to the eager loop
    by the bounds at the head of this file, the last replay's loss and norm too."""
    gen = torch.Generator().manual_seed(17)
    xs = torch.randn(1, BATCH, D_IN, generator=gen).cuda()
    want, want_losses, want_norms = _run_net(False, xs, back_to_back=True)
    got, losses, norms = _run_net(True, xs, back_to_back=True)
    assert float(want_norms.min()) > 10 * MAX_NORM
    print("last loss eager %.8g captured %.8g, last norm eager %.8g captured %.8g"
          % (float(want_losses[-1]), float(losses[-1]), float(want_norms[-1]), float(norms[-1])))
    for k, ((p, m, t), (p0, m0, t0)) in enumerate(zip(got, want)):
        dp, dm = float((p - p0).abs().max()), float((m - m0).abs().max() / m0.abs().max())
        print("tensor %d: |param difference| %.3e (bound %.3e), exp_avg %.3e (bound %.3e)" % (k, dp, 1e-2 * LR * STEPS, dm, 1e-2 * STEPS))
    torch.testing.assert_close(losses[-1], want_losses[-1], rtol=1e-4, atol=0.0)
    torch.testing.assert_close(norms[-1], want_norms[-1], rtol=1e-4, atol=0.0)
    for k, ((p, m, t), (p0, m0, t0)) in enumerate(zip(got, want)):
        assert t == t0 == float(STEPS), k
        assert float((p - p0).abs().max()) <= 1e-2 * LR * STEPS, k
        assert float((m - m0).abs().max() / m0.abs().max()) <= 1e-2 * STEPS, k
