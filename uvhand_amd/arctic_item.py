"""The SmoothNet stage's per-frame query selection and input masking (UVHand arctic_tools/process.py:20-70,
engine.py:336-344) without host synchronisation.

``get_arctic_item(outputs, cfg, device=None)`` keeps the reference's signature and return structure.  On CUDA fp32 outputs it is
one HIP launch forward and one backward (``csrc/msda_arctic_item.hip``) instead of a per-class loop of boolean-mask
assignments; everything else runs ``get_arctic_item_reference``, a torch restatement: CPU tensors, logits that are not fp32,
sources that are not fp32, any autocast region, ``len(cfg.hand_idx) != 2``.  With ``MSDA_SMALL_LOSS_BF16=1`` (read at call time,
off by default) bf16 sources (all six) and bf16 autocast run the grouped kernels as one set instead; fp16 autocast and mixed
dtypes keep the restatement.  The returned tensors are fresh (not views of the DETR outputs): ``train_smoothnet`` modifies them
in place.

``get_arctic_item_many(outputs_list, cfg, device=None)`` selects for every prediction set of a step in one launch forward and
one backward, as one autograd node: fp32 logits with sources all fp32 or all bf16 (bits read element by element; rows are
only 2-byte aligned), under no autocast or bf16 autocast.  The nine tensors are fp32 either way, for bf16 sources the gathered
values widened exactly, which is what the restatement's ``.to(float32)`` gives; a bf16 source's gradient is the fp32 sum of
its row's gradients (a row both hands picked: left first) rounded to bf16 once.  Sets it does not take (CPU, fp16 autocast,
mixed dtypes, shapes differing between sets, more than ``SMALL_LOSS_MAX_SETS`` sets, ``len(cfg.hand_idx) != 2``) run per-set
``get_arctic_item`` calls.

``perturb_arctic_item(items, p_mask, scale)`` is the masking of ``train_smoothnet``: each element is replaced by
``x + N(0, 1) * scale`` with probability ``p_mask``.  Same distribution, but drawn with ``torch.where`` on device draws
instead of boolean indexing and a host ``randn(...).cuda()`` per parameter, so the random stream is not the reference's."""
import torch

from . import _native
from ._autocast import autocast_refuses, bf16_autocast, no_autocast, small_loss_bf16_enabled

# engine.py:337-338: root (l, r, o), pose, shape, obj (rot, rad)
DEFAULT_SCALE = [[0.1, 0.1, 0.1], 0.1, 0.1, [5, 0.1]]


def _sources(outputs):
    hand_cam, obj_cam = outputs['pred_cams']
    mano_pose, mano_shape = outputs['pred_mano_params']
    out_obj_rad, out_obj_rot = outputs['pred_obj_params']
    return [hand_cam, obj_cam, mano_pose, mano_shape, out_obj_rad, out_obj_rot]


def _structure(t):
    return [t[0], t[1], t[2]], [t[3], t[4]], [t[5], t[6]], [t[7], t[8]]


def get_arctic_item_reference(outputs, cfg, device=None):
    """arctic_tools/process.py:20-70 restated; ``device`` defaults to the logits' device."""
    out_logits = outputs['pred_logits']
    hand_cam, obj_cam, mano_pose, mano_shape, out_obj_rad, out_obj_rot = _sources(outputs)
    device = out_logits.device if device is None else device
    prob = out_logits.sigmoid()
    bs = prob.shape[0]
    best_score = torch.zeros(bs).to(device).to(prob.dtype)
    obj_idx = torch.zeros(bs).to(device).to(torch.long)
    for i in range(1, cfg.hand_idx[0]):
        score, idx = torch.max(prob[:, :, i], dim=-1)
        obj_idx[best_score < score] = idx[best_score < score]
        best_score[best_score < score] = score[best_score < score]
    left_hand_idx, right_hand_idx = [torch.argmax(prob[:, :, i], dim=-1) for i in cfg.hand_idx]

    def take(src, idx, w):
        return torch.gather(src, 1, idx.view(-1, 1, 1).repeat(1, 1, w))[:, 0, :].to(torch.float32)

    return ([take(hand_cam, left_hand_idx, 3), take(hand_cam, right_hand_idx, 3), take(obj_cam, obj_idx, 3)],
            [take(mano_pose, left_hand_idx, 48), take(mano_pose, right_hand_idx, 48)],
            [take(mano_shape, left_hand_idx, 10), take(mano_shape, right_hand_idx, 10)],
            [take(out_obj_rot, obj_idx, 3), take(out_obj_rad, obj_idx, 1)])


class _ArcticItemFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, classes, logits, *sources):
        outs, idx = _native.arctic_item_forward(logits, [s.contiguous() for s in sources], *classes)
        ctx.save_for_backward(idx)
        ctx.Q = logits.shape[1]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        idx, = ctx.saved_tensors
        g = [gr.contiguous() if gr is not None else None for gr in grads]
        gsrc = _native.arctic_item_backward(idx, ctx.Q, g)
        return (None, None) + tuple(gsrc)


class _ArcticItemManyFunction(torch.autograd.Function):
    """Every set's selection as one node: one grouped launch forward, one backward; fp32 or bf16 sources."""

    @staticmethod
    def forward(ctx, classes, n, *flat):
        ctx.set_materialize_grads(False)
        sources = [[s.contiguous() for s in flat[n + 6 * i:n + 6 * i + 6]] for i in range(n)]
        outs, idx = _native.arctic_item_many_forward(list(flat[:n]), sources, *classes)
        ctx.save_for_backward(idx)
        ctx.n, ctx.Q, ctx.dtype = n, flat[0].shape[1], flat[n].dtype
        return tuple(t for grp in outs for t in grp)

    @staticmethod
    def backward(ctx, *grads):
        idx, = ctx.saved_tensors
        g = [gr.contiguous() if gr is not None else None for gr in grads]
        gsrc = _native.arctic_item_many_backward(idx, ctx.Q, g, ctx.dtype)
        return (None, None) + (None,) * ctx.n + tuple(t for grp in gsrc for t in grp)


def _kernel_dtype(logits, sources, cfg):
    """The sources' one dtype (fp32 or bf16) when the kernels take these tensors, whatever autocast says; else None."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3) or len(cfg.hand_idx) != 2:
        return None
    bs, Q, K = logits.shape
    if not (1 <= cfg.hand_idx[0] <= K and all(0 <= int(h) < K for h in cfg.hand_idx)) or bs == 0 or Q == 0:
        return None
    dtype = sources[0].dtype
    if dtype not in (torch.float32, torch.bfloat16):
        return None
    ok = all(s.is_cuda and s.dtype == dtype and s.device == logits.device and tuple(s.shape) == (bs, Q, w)
             for s, w in zip(sources, _native.ARCTIC_ITEM_WIDTHS))
    return dtype if ok else None


def _classes(cfg):
    # the object classes end where the hand classes start: obj_end = hand_idx[0] = the left hand's class
    return (int(cfg.hand_idx[0]), int(cfg.hand_idx[0]), int(cfg.hand_idx[1]))


def _grouped(outputs_list, cfg):
    """The grouped kernels on sets that _kernel_dtype accepted with one dtype and one shape."""
    n = len(outputs_list)
    logits = [o['pred_logits'].contiguous() for o in outputs_list]
    sources = [_sources(o) for o in outputs_list]
    flat = [s for grp in sources for s in grp]
    with no_autocast():
        if torch.is_grad_enabled() and any(s.requires_grad for s in flat):
            outs = _ArcticItemManyFunction.apply(_classes(cfg), n, *logits, *flat)
            outs = [outs[9 * i:9 * i + 9] for i in range(n)]
        else:
            outs, _ = _native.arctic_item_many_forward(logits, [[s.contiguous() for s in grp] for grp in sources], *_classes(cfg))
    return [_structure(list(o)) for o in outs]


def get_arctic_item(outputs, cfg, device=None):
    """One query per hand and object in each frame, and the nine parameters gathered at them:
    ([root_l, root_r, root_o], [mano_pose_l, mano_pose_r], [mano_shape_l, mano_shape_r], [obj_rot, obj_rad]).
    ``device``: accepted for the reference's signature; the results live on the outputs' device."""
    logits = outputs['pred_logits']
    sources = _sources(outputs)
    dtype = _kernel_dtype(logits, sources, cfg)
    if dtype != torch.float32 or torch.is_autocast_enabled():
        # MSDA_SMALL_LOSS_BF16=1: bf16 sources and bf16 autocast go to the grouped entry as one set
        if dtype is not None and small_loss_bf16_enabled() and not autocast_refuses():
            return _grouped([outputs], cfg)[0]
        return get_arctic_item_reference(outputs, cfg, device)
    classes = _classes(cfg)
    logits_c = logits.contiguous()
    if torch.is_grad_enabled() and any(s.requires_grad for s in sources):
        outs = _ArcticItemFunction.apply(classes, logits_c, *sources)
    else:
        outs, _ = _native.arctic_item_forward(logits_c, [s.contiguous() for s in sources], *classes)
    return _structure(list(outs))


def get_arctic_item_many(outputs_list, cfg, device=None):
    """``get_arctic_item`` of every set of ``outputs_list`` (the final and aux outputs of one step), as a list.  CUDA fp32
    logits with sources all fp32 or all bf16, of one shape in every set, under no autocast or bf16 autocast, are one grouped
    launch forward and one backward for at most ``SMALL_LOSS_MAX_SETS`` sets, and one autograd node; anything else is the
    per-set calls."""
    outputs_list = list(outputs_list)
    if 1 <= len(outputs_list) <= _native.SMALL_LOSS_MAX_SETS and (not torch.is_autocast_enabled() or bf16_autocast()):
        first = outputs_list[0]['pred_logits']
        dtypes = [_kernel_dtype(o['pred_logits'], _sources(o), cfg) for o in outputs_list]
        if dtypes[0] is not None and all(d == dtypes[0] for d in dtypes) and all(
                o['pred_logits'].shape == first.shape and o['pred_logits'].device == first.device for o in outputs_list):
            return _grouped(outputs_list, cfg)
    return [get_arctic_item(o, cfg, device) for o in outputs_list]


def perturb_arctic_item(items, p_mask=0.05, scale=None):
    """engine.py:336-344 without host synchronisation: each element of each parameter becomes ``x + randn * s`` with
    probability p_mask (s from ``scale``, the reference's per-group scales by default).  In place; returns ``items``."""
    scale = DEFAULT_SCALE if scale is None else scale
    for idx, out in enumerate(items):
        for p_idx, param in enumerate(out):
            s = scale[idx][p_idx] if isinstance(scale[idx], (list, tuple)) else scale[idx]
            mask = torch.rand(param.shape, device=param.device, dtype=param.dtype) > (1 - p_mask)
            noise = torch.randn(param.shape, device=param.device, dtype=param.dtype) * s
            param.copy_(torch.where(mask, param + noise, param))
    return items
