"""Drop-ins for the tail of the reference's training step (engine.py:644-648, util/settings.py:434):

    grad_total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
    optimizer.step()                                         # torch.optim.AdamW, three parameter groups

``clip_grad_norm_`` and ``AdamW`` below have torch's signatures, return values and state, and run as multi-tensor HIP launches
(csrc/msda_optim.hip) whose number does not grow with the number of tensors: three for a clipped step, one for an unclipped
one.  ``AdamW.step(max_norm=...)`` folds the clip into the update: the gradients are read twice and never written.

Where the kernels do not apply (see ``AdamW.step``), torch's own functions run instead and the library launches nothing; that
is the whole behaviour of this module on CPU tensors.  ``MSDA_OPTIM_FUSED=0``, read at call time, forces that route.

Steady state without a host sync.  The kernels read device-resident tables (addresses, sizes, chunk starts, groups, step
offsets).  They are uploaded when the set of parameters with a gradient changes; the gradients' addresses can change every
step (``zero_grad(set_to_none=True)``), so their list is compared on the host and that one table is re-sent when it differs.
Every upload is a non-blocking copy out of a pinned buffer that is not rewritten while that copy may be pending: a ring of
buffers, each with an event that is polled with ``query()``; the ring grows rather than waits.
"""
import os

import torch

from . import _native

try:
    from torch.optim.optimizer import _get_scalar_dtype
except ImportError:                                          # pragma: no cover - torch without the private helper
    def _get_scalar_dtype():
        return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32

__all__ = ["AdamW", "clip_grad_norm_", "grad_norm"]


def _enabled():
    return os.environ.get("MSDA_OPTIM_FUSED", "1") != "0"


class _Uploader:
    """Non-blocking host-to-device copies of int64 tables through a ring of pinned buffers (one ring per device)."""

    def __init__(self):
        self.slots = []                                      # [pinned int64 buffer, event of its last copy or None]

    def send(self, values, dst):
        """values: CPU int64 tensor; dst: device int64 tensor of the same length.  Enqueues on the current stream."""
        n = values.numel()
        slot = None
        for s in self.slots:
            if s[0].numel() >= n and (s[1] is None or s[1].query()):
                slot = s
                break
        if slot is None:
            # buffers too small for this table will not be needed again once their copies are done
            self.slots = [s for s in self.slots if s[0].numel() >= n or not (s[1] is None or s[1].query())]
            slot = [torch.empty(max(n, 256), dtype=torch.int64, pin_memory=True), None]
            self.slots.append(slot)
        buf = slot[0][:n]
        buf.copy_(values)
        dst.copy_(buf, non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()


_uploaders = {}


def _uploader(dev):
    up = _uploaders.get(dev)
    if up is None:
        up = _uploaders[dev] = _Uploader()
    return up


def _dense_f32_cuda(t):
    return t.layout == torch.strided and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


class _GradTables:
    """Device tables of a list of gradients for the norm and the scaling: g [n], numel [n], chunk_start [n + 1]."""

    def __init__(self, dev, numels):
        self.dev, self.numels, self.n = dev, numels, len(numels)
        self.chunk_start, self.n_chunks = _native.optim_chunks(numels)
        self.table = torch.empty(3 * self.n + 1, dtype=torch.int64, device=dev)
        self.partials = torch.empty(max(1, self.n_chunks), dtype=torch.float32, device=dev)
        self.gptrs = None
        base = self.table.data_ptr()
        self.g, self.numel, self.start = base, base + 8 * self.n, base + 16 * self.n

    def bind(self, gptrs):
        if gptrs != self.gptrs:
            _uploader(self.dev).send(torch.tensor(gptrs + self.numels + self.chunk_start, dtype=torch.int64), self.table)
            self.gptrs = gptrs

    def norm(self, max_norm):
        """sumsq + finish: fp32 [2] = (total norm, clip coefficient)."""
        out = torch.empty(2, dtype=torch.float32, device=self.dev)
        _native.grad_sumsq(self.dev, self.n, self.n_chunks, self.g, self.numel, self.start, self.partials)
        _native.grad_norm_finish(self.dev, self.n_chunks, self.partials, max_norm, out)
        return out


_grad_tables = {}                                            # device -> the tables of the last list of gradients seen there


def _fused_grads(parameters):
    """(grads, device) when the kernels take every gradient of `parameters`, else (None, None)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads or not _enabled():
        return None, None
    dev = grads[0].device
    if not all(_dense_f32_cuda(g) and g.device == dev for g in grads):
        return None, None
    if torch.cuda.is_current_stream_capturing() or not _native.optim_supported(len(grads), 1):
        return None, None
    return grads, dev


def _tables_for(grads, dev):
    numels = [g.numel() for g in grads]
    tables = _grad_tables.get(dev)
    if tables is None or tables.numels != numels:
        tables = _grad_tables[dev] = _GradTables(dev, numels)
    tables.bind([g.data_ptr() for g in grads])
    return tables


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` with the same signature and return value.  With ``norm_type == 2``,
    ``error_if_nonfinite=False``, ``max_norm > 0`` and every gradient a dense fp32 CUDA tensor on one device it is three
    launches (sum of squares per chunk, norm and coefficient, in-place scaling) and returns a 0-d device tensor without a host
    sync; anything else calls torch's function."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    else:
        parameters = list(parameters)
    max_norm = float(max_norm)
    grads, dev = (None, None)
    if float(norm_type) == 2.0 and not error_if_nonfinite and max_norm > 0.0:
        grads, dev = _fused_grads(parameters)
    if grads is None:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    with torch.cuda.device(dev):
        tables = _tables_for(grads, dev)
        if tables.n_chunks == 0:
            return torch.zeros((), dtype=torch.float32, device=dev)
        out = tables.norm(max_norm)
        _native.grad_scale(dev, tables.n, tables.n_chunks, tables.g, tables.numel, tables.start, out.data_ptr() + 4)
    return out[0]


@torch.no_grad()
def grad_norm(parameters):
    """The 2-norm of all gradients as a 0-d tensor and nothing else (util/misc.py get_total_grad_norm): two launches on the
    kernels' route, ``torch.nn.utils.get_total_norm`` otherwise."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    else:
        parameters = list(parameters)
    grads, dev = _fused_grads(parameters)
    if grads is None:
        return torch.nn.utils.get_total_norm([p.grad for p in parameters if p.grad is not None], 2.0)
    with torch.cuda.device(dev):
        tables = _tables_for(grads, dev)
        if tables.n_chunks == 0:
            return torch.zeros((), dtype=torch.float32, device=dev)
        return tables.norm(0.0)[0]


class _Plan:
    """The device tables of one set of parameters with a gradient, in param_groups order."""

    def __init__(self, dev, params, states, gidx, pptrs, global_step):
        n = self.n = len(params)
        self.dev, self.gidx, self.pptrs = dev, gidx, pptrs
        self.steps = [s["step"] for s in states]
        self.state_ids = [id(s["exp_avg"]) for s in states]
        numels = [p.numel() for p in params]
        chunk_start, self.n_chunks = _native.optim_chunks(numels)
        # t of a tensor in the next launch = (global_step + 1) - offset = its own step + 1
        offsets = [global_step - int(s.item()) for s in self.steps]
        rows = pptrs + [s["exp_avg"].data_ptr() for s in states] + [s["exp_avg_sq"].data_ptr() for s in states] + numels \
            + offsets + chunk_start
        groups = torch.zeros(2 * ((n + 1) // 2), dtype=torch.int32)
        groups[:n] = torch.tensor(gidx, dtype=torch.int32)
        host = torch.cat([torch.tensor(rows, dtype=torch.int64), groups.view(torch.int64)])
        self.table = torch.empty(host.numel(), dtype=torch.int64, device=dev)
        _uploader(dev).send(host, self.table)
        base = self.table.data_ptr()
        self.p, self.m, self.v, self.numel, self.offset = (base + 8 * n * k for k in range(5))
        self.start = base + 8 * 5 * n
        self.group = self.start + 8 * (n + 1)
        self.gtable = torch.empty(n, dtype=torch.int64, device=dev)
        self.gptrs = None
        self.partials = torch.empty(max(1, self.n_chunks), dtype=torch.float32, device=dev)

    def bind(self, gptrs):
        if gptrs != self.gptrs:
            _uploader(self.dev).send(torch.tensor(gptrs, dtype=torch.int64), self.gtable)
            self.gptrs = gptrs


class AdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` whose step is one multi-tensor HIP launch (three with the clip folded in).

    A subclass with the same constructor: ``param_groups``, ``state_dict``, ``load_state_dict``, ``add_param_group`` and every
    ``lr_scheduler`` work unchanged, and the state is exactly torch's (``step`` as torch creates it, ``exp_avg``,
    ``exp_avg_sq``), so checkpoints move between this class and ``torch.optim.AdamW`` in both directions.
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._plan = None
        self._global_step = 0
        self.last_grad_norm = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def _collect(self):
        """(device, params, group indices, param addresses, grad addresses) of the parameters with a gradient when the kernels
        take all of them, else None."""
        groups = self.param_groups
        if not _enabled() or not 1 <= len(groups) <= _native.OPTIM_MAX_GROUPS:
            return None
        for g in groups:
            if g["amsgrad"] or g["maximize"] or g["capturable"] or g["differentiable"] or g.get("fused"):
                return None
            scalars = (g["lr"], g["eps"], g["weight_decay"]) + tuple(g["betas"])
            if any(isinstance(x, torch.Tensor) for x in scalars):
                return None
        dev, params, gidx, pptrs, gptrs = None, [], [], [], []
        f32, strided = torch.float32, torch.strided
        for gi, g in enumerate(groups):
            for p in g["params"]:
                grad = p.grad
                if grad is None:
                    continue
                if not (p.layout == strided and grad.layout == strided and p.is_cuda and p.dtype == f32 and grad.dtype == f32
                        and grad.device == p.device and p.is_contiguous() and grad.is_contiguous()):
                    return None
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    return None
                params.append(p)
                gidx.append(gi)
                pptrs.append(p.data_ptr())
                gptrs.append(grad.data_ptr())
        if dev is not None and torch.cuda.is_current_stream_capturing():
            return None
        return dev, params, gidx, pptrs, gptrs

    def _make_plan(self, dev, params, gidx, pptrs):
        states = []
        for p in params:
            state = self.state[p]
            if len(state) == 0:                              # torch's lazy initialisation (Adam._init_group)
                state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v, step = state["exp_avg"], state["exp_avg_sq"], state["step"]
            if not (_dense_f32_cuda(m) and _dense_f32_cuda(v) and m.device == dev and v.device == dev
                    and m.numel() == p.numel() and v.numel() == p.numel() and not step.is_cuda):
                return None
            states.append(state)
        return _Plan(dev, params, states, gidx, pptrs, self._global_step)

    def _torch_step(self, max_norm):
        self._plan = None
        if max_norm is not None:
            params = [p for g in self.param_groups for p in g["params"]]
            if float(max_norm) > 0.0:
                self.last_grad_norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
            else:
                self.last_grad_norm = torch.nn.utils.get_total_norm([p.grad for p in params if p.grad is not None], 2.0)
        step = torch.optim.AdamW.step
        while getattr(step, "hooked", False):                # this class's step already ran the step hooks
            step = step.__wrapped__
        step(self)

    @torch.no_grad()
    def step(self, closure=None, *, max_norm=None):
        """One optimisation step.  ``max_norm`` given: the fused form of ``clip_grad_norm_(parameters, max_norm)`` followed by
        the step.  The clipped gradient exists in registers only: **``.grad`` is left unscaled**, unlike after torch's
        ``clip_grad_norm_``.  ``self.last_grad_norm`` is then the 0-d device tensor of the total norm before clipping (what
        ``metric_logger.update(grad_norm=...)`` logs); ``max_norm <= 0`` computes the norm and clips nothing (the reference's
        ``get_total_grad_norm`` branch).

        torch's own ``clip_grad_norm_`` and ``AdamW.step`` run instead, and the library launches nothing, for ``amsgrad``,
        ``maximize``, ``capturable``, ``differentiable`` or ``fused`` groups, tensor hyperparameters, any parameter with a
        gradient (or gradient, or state) that is not a dense contiguous fp32 CUDA tensor, parameters on more than one device,
        more than 8 groups, an active stream capture and ``MSDA_OPTIM_FUSED=0``."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        got = self._collect()
        if got is None:
            self._torch_step(max_norm)
            return loss
        dev, params, gidx, pptrs, gptrs = got
        if dev is None:                                      # no parameter has a gradient: torch's step does nothing
            if max_norm is not None:
                self.last_grad_norm = torch.tensor(0.0)
            return loss
        with torch.cuda.device(dev):
            plan = self._plan
            if plan is None or plan.pptrs != pptrs or plan.gidx != gidx or plan.dev != dev \
                    or plan.state_ids != [id(self.state[p].get("exp_avg")) for p in params]:
                plan = self._make_plan(dev, params, gidx, pptrs)
                if plan is None:
                    self._torch_step(max_norm)
                    return loss
                self._plan = plan
            plan.bind(gptrs)
            self._global_step += 1
            torch._foreach_add_(plan.steps, 1)
            hyper = [(g["lr"], g["weight_decay"], g["betas"][0], g["betas"][1], g["eps"]) for g in self.param_groups]
            coef = None
            if max_norm is not None:
                if plan.n_chunks == 0:
                    self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
                else:
                    out = torch.empty(2, dtype=torch.float32, device=dev)
                    _native.grad_sumsq(dev, plan.n, plan.n_chunks, plan.gtable.data_ptr(), plan.numel, plan.start, plan.partials)
                    _native.grad_norm_finish(dev, plan.n_chunks, plan.partials, max_norm, out)
                    self.last_grad_norm = out[0]
                    coef = out.data_ptr() + 4
            _native.adamw_step(dev, plan.n, plan.n_chunks, plan.p, plan.gtable.data_ptr(), plan.m, plan.v, plan.numel, plan.start,
                               plan.group, plan.offset, hyper, self._global_step, coef)
        return loss
