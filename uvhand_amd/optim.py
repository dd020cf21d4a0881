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

The device-state form.  ``AdamW(..., capturable=True)`` (torch's own flag, on every group) keeps what changes from step to step on
the device: each parameter's ``step`` is the 0-d fp32 device tensor ``torch.optim.AdamW(capturable=True)`` keeps, and the groups'
hyperparameters are a device table with a host shadow (``AdamW.refresh_hyper``).  The same arithmetic then runs eagerly or
inside a stream capture, so that forward + loss + backward + clip + update replay as one HIP graph::

    graph.replay(); lr_scheduler.step(); optimizer.refresh_hyper()
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

    def __init__(self, dev, params, states, gidx, pptrs, per_tensor):
        """per_tensor: what the update reads for each tensor besides its addresses: the step offset (host steps: t of a tensor in
        the next launch = (global_step + 1) - offset = its own step + 1) or the address of its device step (_DevPlan)."""
        n = self.n = len(params)
        self.dev, self.gidx, self.pptrs = dev, gidx, pptrs
        self.steps = [s["step"] for s in states]             # host steps: advanced through this list; device steps: kept alive
        self.state_ids = [id(s["exp_avg"]) for s in states]
        numels = [p.numel() for p in params]
        chunk_start, self.n_chunks = _native.optim_chunks(numels)
        rows = pptrs + [s["exp_avg"].data_ptr() for s in states] + [s["exp_avg_sq"].data_ptr() for s in states] + numels \
            + list(per_tensor) + chunk_start
        groups = torch.zeros(2 * ((n + 1) // 2), dtype=torch.int32)
        groups[:n] = torch.tensor(gidx, dtype=torch.int32)
        host = torch.cat([torch.tensor(rows, dtype=torch.int64), groups.view(torch.int64)])
        self.table = torch.empty(host.numel(), dtype=torch.int64, device=dev)
        _uploader(dev).send(host, self.table)
        base = self.table.data_ptr()
        self.p, self.m, self.v, self.numel, self.per_tensor = (base + 8 * n * k for k in range(5))
        self.start = base + 8 * 5 * n
        self.group = self.start + 8 * (n + 1)
        self.gtable = torch.empty(n, dtype=torch.int64, device=dev)
        self.gptrs = None
        self.partials = torch.empty(max(1, self.n_chunks), dtype=torch.float32, device=dev)

    def bind(self, gptrs):
        """The gradients' table, re-sent through the ring when the addresses changed.  Returns the table's address."""
        if gptrs != self.gptrs:
            _uploader(self.dev).send(torch.tensor(gptrs, dtype=torch.int64), self.gtable)
            self.gptrs = gptrs
        return self.gtable.data_ptr()


class _DevPlan(_Plan):
    """The plan of the device-state form: per tensor the address of its 0-d device step.  Nothing in its tables changes from
    step to step, and under a capture the gradients' table is the capture's own."""

    def __init__(self, dev, params, states, gidx, pptrs):
        super().__init__(dev, params, states, gidx, pptrs, [s["step"].data_ptr() for s in states])
        # a capture may not allocate pinned memory (that is no stream operation, and the runtime can refuse it while a stream
        # captures), so the buffer its table is copied from exists beforehand; an eager step after a capture makes the next one
        self.spare = self._pinned()
        self.captured = []                                   # (addresses, pinned copy, device table) of every capture

    def _pinned(self):
        return torch.empty(max(1, self.n), dtype=torch.int64, pin_memory=True)

    def bind(self, gptrs):
        if self.spare is None:
            self.spare = self._pinned()
        return super().bind(gptrs)

    def bind_captured(self, gptrs):
        """Under a capture: a table of the capture's own, filled by ONE captured copy out of a pinned buffer that is written
        here, once, and then kept unchanged for the plan's life, so that every replay copies the same addresses again.  The
        eager table and the ring are left alone: a later eager step may rewrite both."""
        for ptrs, pinned, table in self.captured:
            if ptrs == gptrs:
                break
        else:
            if self.spare is None:
                raise RuntimeError("AdamW(capturable=True): a second capture with gradients at other addresses needs an eager "
                                   "step() in between (it prepares the pinned buffer the capture copies their table from)")
            pinned, self.spare = self.spare, None
            pinned[:self.n] = torch.tensor(gptrs, dtype=torch.int64)
            table = torch.empty(max(1, self.n), dtype=torch.int64, device=self.dev)
            self.captured.append((gptrs, pinned, table))
        table.copy_(pinned, non_blocking=True)
        return table.data_ptr()


def _hyper_rows(groups):
    """[(lr, weight_decay, beta1, beta2, eps)] of the groups as Python floats, checked as msda_adamw_step_f32 checks them."""
    rows = [(float(g["lr"]), float(g["weight_decay"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) for g in groups]
    for lr, wd, b1, b2, eps in rows:
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise RuntimeError("AdamW(capturable=True): betas must be in [0, 1)")
        if not all(x == x and abs(x) != float("inf") for x in (lr, wd, eps)):
            raise RuntimeError("AdamW(capturable=True): lr, eps and weight_decay must be finite")
    return rows


class AdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` whose step is one multi-tensor HIP launch (three with the clip folded in).

    A subclass with the same constructor: ``param_groups``, ``state_dict``, ``load_state_dict``, ``add_param_group`` and every
    ``lr_scheduler`` work unchanged, and the state is exactly torch's (``step`` as torch creates it, ``exp_avg``,
    ``exp_avg_sq``), so checkpoints move between this class and ``torch.optim.AdamW`` in both directions.

    ``capturable=True`` on every group selects the device-state form (see the module's head): two launches for a plain step,
    three with the clip, eagerly or inside a stream capture, with the state of ``torch.optim.AdamW(capturable=True)``.  A
    capture needs what torch's graph recipe needs, warm-up steps: the tables and every state must exist from an earlier eager
    step, and the device hyperparameters must equal ``param_groups`` (``refresh_hyper``).  The gradients may live anywhere:
    ``zero_grad(set_to_none=True)`` before the capture and a backward inside it is fine.  ``last_grad_norm`` of a captured
    step is static memory of the graph that every replay refreshes; read or clone it before the next replay.

    A graph holds the addresses it was captured with.  The optimizer keeps the tables and step counts of every captured plan
    alive, but not ``exp_avg`` and ``exp_avg_sq``, and a change of device replaces the hyperparameter table and the skip
    counter: capture again after ``load_state_dict``, ``add_param_group`` or a move to another device, as torch's capturable
    optimizer requires.  A replay of the older graph would write moments the allocator may already have handed out again.
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._plan = None
        self._global_step = 0
        self.last_grad_norm = None
        self._hyper = None                                   # device-state form: (device, fp64 [8, 5] table, host shadow)
        self._status = None                                  # int32 [2] on the device: (the last step was skipped, skipped steps)
        self._kept = []                                      # plans a capture has read: their tables outlive a rebuild

    @property
    def skipped_steps(self):
        """0-d int32 device tensor: the ``step(..., skip_nonfinite=True)`` calls (replays included) whose norm was not finite.
        None before the first step of the device-state form."""
        return None if self._status is None else self._status[1]

    def refresh_hyper(self):
        """Device-state form: compare ``param_groups`` with the host shadow of the device hyperparameter table and, when they
        differ, send the table (a non-blocking copy on the current stream, no synchronisation).  Returns whether it sent
        anything.  Call it after ``lr_scheduler.step()`` between two replays of a captured step; an eager ``step`` does it by
        itself.  False and nothing done on the other routes and before the first step.

        The copy is ordered against ``graph.replay()`` only when both are issued on the same stream: with the replay on a side
        stream, call this under that stream too, otherwise the copy races with the replay's reads of the table."""
        if self._hyper is None or not _enabled() or not all(g["capturable"] for g in self.param_groups):
            return False
        dev, table, shadow = self._hyper
        rows = _hyper_rows(self.param_groups)
        if rows == shadow or len(rows) > _native.OPTIM_MAX_GROUPS:
            return False
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("AdamW.refresh_hyper() inside a stream capture: the copy would replay a buffer that is rewritten "
                               "later; call it between replays")
        with torch.cuda.device(dev):
            flat = torch.tensor([x for row in rows for x in row], dtype=torch.float64)
            _uploader(dev).send(flat.view(torch.int64), table.view(-1)[:flat.numel()].view(torch.int64))
        self._hyper = (dev, table, rows)
        return True

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def _collect(self):
        """(device, params, group indices, param addresses, grad addresses) of the parameters with a gradient when the kernels
        take all of them, else None.  Groups that all have ``capturable=True`` are the device-state form; mixed ones are torch's."""
        groups = self.param_groups
        if not _enabled() or not 1 <= len(groups) <= _native.OPTIM_MAX_GROUPS:
            return None
        capturable = groups[0]["capturable"]
        for g in groups:
            if g["amsgrad"] or g["maximize"] or g["capturable"] != capturable or g["differentiable"] or g.get("fused"):
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
        if dev is not None and not capturable and torch.cuda.is_current_stream_capturing():
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
        return _Plan(dev, params, states, gidx, pptrs, [self._global_step - int(s["step"].item()) for s in states])

    def _make_dev_plan(self, dev, params, gidx, pptrs):
        states = []
        for p in params:
            state = self.state[p]
            if len(state) == 0:                              # as torch's capturable route creates it (Adam._init_group)
                state["step"] = torch.zeros((), dtype=_get_scalar_dtype(), device=p.device)
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v, step = state["exp_avg"], state["exp_avg_sq"], state["step"]
            if not (_dense_f32_cuda(m) and _dense_f32_cuda(v) and m.device == dev and v.device == dev
                    and m.numel() == p.numel() and v.numel() == p.numel()
                    and _dense_f32_cuda(step) and step.device == dev and step.dim() == 0):
                return None
            states.append(state)
        return _DevPlan(dev, params, states, gidx, pptrs)

    def _dev_step(self, dev, params, gidx, pptrs, gptrs, max_norm, skip_nonfinite):
        """The device-state form.  Returns False when a state is not what the kernels take (torch's route then runs)."""
        capturing = torch.cuda.is_current_stream_capturing()
        plan = self._plan
        if type(plan) is not _DevPlan or plan.pptrs != pptrs or plan.gidx != gidx or plan.dev != dev \
                or plan.state_ids != [id(self.state[p].get("exp_avg")) for p in params] \
                or self._hyper is None or self._hyper[0] != dev:
            if capturing:
                raise RuntimeError("AdamW(capturable=True).step() inside a stream capture before its tables and states exist "
                                   "for this set of parameters: warm-up steps are needed, run an eager step() with the same "
                                   "parameters having gradients first (torch's CUDA graph recipe does the same)")
            plan = self._make_dev_plan(dev, params, gidx, pptrs)
            if plan is None:
                return False
            self._plan = plan
            if self._hyper is None or self._hyper[0] != dev:
                self._hyper = (dev, torch.zeros(_native.OPTIM_MAX_GROUPS, 5, dtype=torch.float64, device=dev), None)
                self._status = torch.zeros(2, dtype=torch.int32, device=dev)
        if capturing:
            if _hyper_rows(self.param_groups) != self._hyper[2]:
                raise RuntimeError("AdamW(capturable=True).step() inside a stream capture: param_groups' hyperparameters differ "
                                   "from the device table; call refresh_hyper() before the capture")
            g = plan.bind_captured(gptrs)
            if plan not in self._kept:
                self._kept.append(plan)
        else:
            g = plan.bind(gptrs)
            self.refresh_hyper()
        hyper, status = self._hyper[1].data_ptr(), self._status.data_ptr()
        coef = skip = None
        if max_norm is not None and plan.n_chunks > 0:
            out = torch.empty(2, dtype=torch.float32, device=dev)      # under a capture: the graph's own memory
            _native.grad_sumsq(dev, plan.n, plan.n_chunks, g, plan.numel, plan.start, plan.partials)
            _native.grad_norm_finish_dev(dev, plan.n_chunks, plan.partials, max_norm, out, plan.n, plan.per_tensor, skip_nonfinite,
                                         status)
            self.last_grad_norm = out[0]
            coef = out.data_ptr() + 4
            skip = status if skip_nonfinite else None
        else:
            if max_norm is not None:                         # nothing but empty tensors: their norm is 0, their steps advance
                self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            _native.optim_advance(dev, plan.n, plan.per_tensor)
        _native.adamw_step_dev(dev, plan.n, plan.n_chunks, plan.p, g, plan.m, plan.v, plan.numel, plan.start, plan.group,
                               plan.per_tensor, len(self.param_groups), hyper, coef, skip)
        return True

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
    def step(self, closure=None, *, max_norm=None, skip_nonfinite=False):
        """One optimisation step.  ``max_norm`` given: the fused form of ``clip_grad_norm_(parameters, max_norm)`` followed by
        the step.  The clipped gradient exists in registers only: **``.grad`` is left unscaled**, unlike after torch's
        ``clip_grad_norm_``.  ``self.last_grad_norm`` is then the 0-d device tensor of the total norm before clipping (what
        ``metric_logger.update(grad_norm=...)`` logs); ``max_norm <= 0`` computes the norm and clips nothing (the reference's
        ``get_total_grad_norm`` branch).

        torch's own ``clip_grad_norm_`` and ``AdamW.step`` run instead, and the library launches nothing, for ``amsgrad``,
        ``maximize``, ``differentiable`` or ``fused`` groups, tensor hyperparameters, any parameter with a
        gradient (or gradient, or state) that is not a dense contiguous fp32 CUDA tensor, parameters on more than one device,
        more than 8 groups, ``MSDA_OPTIM_FUSED=0``, groups of which only some are ``capturable`` and, unless every group is
        ``capturable``, an active stream capture.

        ``skip_nonfinite=True`` (device-state form with ``max_norm``, else an error): a step whose total norm is not finite
        leaves every parameter, moment and step count untouched and adds one to ``self.skipped_steps``; inside a graph this
        stands where engine.py:626 leaves the loop on a non-finite loss.  The default lets such a step poison what torch's
        route poisons."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        got = self._collect()
        nothing = got is not None and got[0] is None         # no parameter has a gradient
        device_state = got is not None and not nothing and self.param_groups[0]["capturable"]
        if skip_nonfinite and not nothing and (max_norm is None or not device_state):
            raise RuntimeError("AdamW.step(skip_nonfinite=True) needs max_norm and the device-state form (capturable=True on "
                               "every group, on the kernels' route): no other route can skip without a host synchronisation")
        if got is None:
            self._torch_step(max_norm)
            return loss
        dev, params, gidx, pptrs, gptrs = got
        if nothing:                                          # torch's step does nothing
            if max_norm is not None:
                self.last_grad_norm = torch.tensor(0.0)
            return loss
        if device_state:
            with torch.cuda.device(dev):
                if self._dev_step(dev, params, gidx, pptrs, gptrs, max_norm, skip_nonfinite):
                    return loss
            if skip_nonfinite:
                raise RuntimeError("AdamW.step(skip_nonfinite=True): a state is not what the device-state kernels take")
            self._torch_step(max_norm)
            return loss
        with torch.cuda.device(dev):
            plan = self._plan
            if type(plan) is not _Plan or plan.pptrs != pptrs or plan.gidx != gidx or plan.dev != dev \
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
                               plan.group, plan.per_tensor, hyper, self._global_step, coef)
        return loss
