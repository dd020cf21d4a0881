"""SmoothNet's MotionSmoother (models/smoothnet.py:7-125) over several calls as one autograd node.

``motion_smoothers(calls, modules, training)`` runs ``modules[m](x)`` for every ``(m, x)`` of ``calls`` (x [B, T, C], the
reference's ``view(B, T, -1)``) and returns the outputs [B, O, C].  On CUDA fp32 it is ``_SmootherFunction``: every Smoother
of every module in one HIP launch per MLP depth (9 with the defaults, ``csrc/msda_smoother.hip``) and at most 11 backward
launches, with no host synchronisation; under ``no_grad`` (the reference's ``test_smoothnet``) nothing is saved.  Calls that
share a module (ArcticSmoother's left / right hands) run as one problem, so the shared weights' gradients come out of one
reduction.

Dropout draws its mask from the kernel's own hash of (seed, problem, layer, row, column): the seed comes from torch's
generator (one ``random_()`` on a device scalar: reproducible under ``manual_seed``, capturable in a HIP graph), the stream is
not ``nn.Dropout``'s.  Keep probability and scaling are nn.Dropout's.

Everything else runs ``motion_smoothers_reference``, a torch restatement of the reference's composition: CPU tensors, non-fp32
inputs, autocast, geometries the kernels do not take, and ``MSDA_SMOOTHER_FUSED=0`` (A/B knob)."""
import os

import torch
import torch.nn.functional as F

from .. import _native


def _smoother_reference(sm, x, training):
    """Smoother.forward (models/smoothnet.py:57-66) with SmootherResBlock.forward (:15-25)."""
    enc = sm.encoder[0]
    x = F.leaky_relu(F.linear(x, enc.weight, enc.bias), 0.1)
    for blk in sm.res_blocks:
        identity = x
        p = blk.dropout.p
        y = F.leaky_relu(F.dropout(F.linear(x, blk.linear1.weight, blk.linear1.bias), p, training), 0.2)
        y = F.leaky_relu(F.dropout(F.linear(y, blk.linear2.weight, blk.linear2.bias), p, training), 0.2)
        x = y + identity
    return F.linear(x, sm.decoder.weight, sm.decoder.bias)


def motion_smoother_reference(module, x, training):
    """MotionSmoother.forward (models/smoothnet.py:108-125): x [B, T, C] -> [B, O, C]."""
    x = x.permute(0, 2, 1)
    N, C, T = x.shape
    assert T == module.window_size, (
        'Input sequence length must be equal to the window size. ',
        f'Got x.shape[2]=={T} and window_size=={module.window_size}')
    vel = x[..., 1:] - x[..., :-1]
    acc = vel[..., 1:] - vel[..., :-1]
    y = torch.cat([_smoother_reference(module.pos_smoother, x, training),
                   _smoother_reference(module.vel_smoother, vel, training),
                   _smoother_reference(module.acc_smoother, acc, training)], dim=2)
    return F.linear(y, module.fusion_layer.weight, module.fusion_layer.bias).permute(0, 2, 1)


def motion_smoothers_reference(calls, modules, training):
    """The reference's composition; same arguments and results as ``motion_smoothers``."""
    return [motion_smoother_reference(modules[m], x, training) for m, x in calls]


def _fused_enabled():
    return os.environ.get("MSDA_SMOOTHER_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatement


def smoother_parameters(module):
    """A MotionSmoother's parameters in the kernels' order (its parameters() order): pos, vel, acc Smoothers (encoder, per
    block linear1 and linear2, decoder; weight before bias), then the fusion Linear."""
    out = []
    for sm in (module.pos_smoother, module.vel_smoother, module.acc_smoother):
        lins = [sm.encoder[0]] + [l for blk in sm.res_blocks for l in (blk.linear1, blk.linear2)] + [sm.decoder]
        for lin in lins:
            out += [lin.weight, lin.bias]
    return out + [module.fusion_layer.weight, module.fusion_layer.bias]


def _dims(module):
    sm = module.pos_smoother
    return (module.window_size, module.output_size, sm.hidden_size, sm.res_hidden_size, len(sm.res_blocks))


def _dropout_p(module):
    ps = {blk.dropout.p for sm in (module.pos_smoother, module.vel_smoother, module.acc_smoother) for blk in sm.res_blocks}
    return ps.pop() if len(ps) == 1 else (0.0 if not ps else None)


def _fused_plan(calls, modules, training):
    """(meta, xs, params) for the kernels, or None where the composition runs."""
    if not (_fused_enabled() and calls) or torch.is_autocast_enabled():
        return None
    used = sorted({m for m, _ in calls})
    if len(used) > _native.SMOOTHER_MAX_MODULES or len(calls) > _native.SMOOTHER_MAX_CALLS:
        return None
    if any(sum(1 for m, _ in calls if m == u) > _native.SMOOTHER_MAX_CALLS_PER_MODULE for u in used):
        return None
    mods = [modules[u] for u in used]
    dims = _dims(mods[0])
    if any(_dims(m) != dims for m in mods) or not _native.smoother_supported(*dims):
        return None
    try:
        params = [p for m in mods for p in smoother_parameters(m)]
    except (AttributeError, IndexError, TypeError):
        return None
    ps = {_dropout_p(m) for m in mods}
    p = ps.pop() if len(ps) == 1 else None
    if p is None or not 0.0 <= p < 1.0:
        return None
    T = dims[0]
    xs = [x for _, x in calls]
    dev = xs[0].device
    if any(not x.is_cuda or x.dtype != torch.float32 or x.device != dev or x.dim() != 3 or x.shape[1] != T or x.numel() == 0
           for x in xs):
        return None
    if any(p_ is None or not p_.is_cuda or p_.dtype != torch.float32 or p_.device != dev or not p_.is_contiguous()
           or p_.data_ptr() % 16 for p_ in params):
        return None
    remap = {u: i for i, u in enumerate(used)}
    meta = (dims, len(used), tuple(remap[m] for m, _ in calls), bool(training), float(p) if training else 0.0)
    return meta, xs, params


def _flat_grads(gp, params):
    out, off = [], 0
    for p in params:
        n = p.numel()
        out.append(gp[off:off + n].view(p.shape))
        off += n
    return out


class _SmootherFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, seed, *tensors):
        dims, n_mod, call_mod, training, p = meta
        n_calls = len(call_mod)
        xs = [x.contiguous().view(-1, x.shape[-1]) for x in tensors[:n_calls]]
        params = tensors[n_calls:]
        outs, act = _native.smoother_forward(dims, n_mod, call_mod, xs, params, training, p, seed)
        ctx.meta = meta
        ctx.shapes = [tuple(x.shape) for x in tensors[:n_calls]]
        ctx.save_for_backward(act, *([seed] if seed is not None else []), *xs, *params)
        O = dims[1]
        return tuple(o.view(-1, O, o.shape[-1]) for o in outs)

    @staticmethod
    def backward(ctx, *grads):
        dims, n_mod, call_mod, training, p = ctx.meta
        n_calls = len(call_mod)
        saved = ctx.saved_tensors
        act, rest = saved[0], saved[1:]
        seed = rest[0] if training and p > 0 else None
        if seed is not None:
            rest = rest[1:]
        xs, params = rest[:n_calls], rest[n_calls:]
        O = dims[1]
        g = [gr.contiguous().view(-1, gr.shape[-1]) if gr is not None
             else torch.zeros(s[0] * O, s[2], dtype=torch.float32, device=act.device) for gr, s in zip(grads, ctx.shapes)]
        want_x = ctx.needs_input_grad[2:2 + n_calls]
        gx, gp = _native.smoother_backward(dims, n_mod, call_mod, list(xs), list(params), act, g, want_x, training, p, seed)
        gx = [t.view(s) if t is not None else None for t, s in zip(gx, ctx.shapes)]
        return (None, None) + tuple(gx) + tuple(_flat_grads(gp, params))


def motion_smoothers(calls, modules, training):
    """Every ``modules[m](x)`` of ``calls`` (a sequence of ``(m, x)``, x [B, T, C]) as one node; returns [B, O, C] per call.

    ``training``: dropout on (the modules' ``training`` flag in the drop-ins)."""
    calls = [(int(m), x) for m, x in calls]
    plan = _fused_plan(calls, modules, training)
    if plan is None:
        return motion_smoothers_reference(calls, modules, training)
    meta, xs, params = plan
    _, _, _, train, p = meta
    seed = torch.empty((), dtype=torch.int64, device=xs[0].device).random_().view(1) if train and p > 0 else None
    O = meta[0][1]
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in xs + params):
        x2 = [x.contiguous().view(-1, x.shape[-1]) for x in xs]
        outs, _ = _native.smoother_forward(meta[0], meta[1], meta[2], x2, params, train, p, seed)
        return [o.view(-1, O, o.shape[-1]) for o in outs]
    return list(_SmootherFunction.apply(meta, seed, *xs, *params))
