"""The ARCTIC evaluation step after ``model(samples)``: drop-ins for arctic_tools/process.py ``make_output``,
``post_process_arctic_output``, ``prepare_data`` and ``measure_error``, for src/utils/loss_modules.py ``get_NN`` and for the
per-key means of engine.py ``test_pose`` (784-794) + ``MetricLogger``, without host synchronisation.

Nearest neighbour.  ``get_NN(src [B, N1, 3], trg [B, N2, 3], k=1)`` returns ``(dists [B, N1] squared fp32, idx [B, N1] int64)``
as pytorch3d's ``knn_points`` with K = 1 and full lengths; ``nn_many(pairs)`` runs pairs that share B, N1 and N2 as one
autograd node of one forward and one backward launch (``csrc/msda_arctic_eval.hip``): the lowest index wins a tie, a NaN
distance never wins, the gradient into the targets is summed in source order without atomics.  ``nn_reference`` is chunked
brute force in torch with the same tie rule (any dtype); it runs for CPU tensors, non-fp32 inputs, geometries over
``msda_nn_supported`` and ``MSDA_ARCTIC_EVAL_FUSED=0``.  Pairs of different shapes get launches of their own.  Whenever device
data misses a kernel for a reason other than that knob (a dtype, a size), a warning names the cause once.

Metrics.  ``arctic_metrics(data)`` takes ``prepare_data``'s prefixed dict and returns one ``[6, B]`` fp32 tensor, rows in
``METRIC_KEYS``, NaN where the reference has NaN, in the reference's units: one launch, one workgroup per frame.
``arctic_metrics_reference`` restates the reference's control flow in torch (per-frame loops and host copies included) in
fp32 or as the fp64 yardstick.  ``measure_error(data, metrics)`` is the drop-in returning numpy arrays (one copy);
``ArcticEvaluator.update(data)`` keeps the running per-key means on the device (graph-capturable) and ``compute()`` is the one
synchronising copy.  Validity follows the reference literally: ``(1 - v).long() != 0`` or Python truth of ``v`` marks a frame
invalid, so a fractional validity counts as valid; the contact deviation alone uses ``(1 - v) != 0``.  ``mdev`` and
``acc_err_pose`` are skipped as ``measure_error`` skips them; the field metrics need the field model and are not provided.

Glue.  ``make_output`` / ``post_process_arctic_output`` / ``prepare_data`` keep the reference's signatures plus ``models=``
(a ``pre_process_models``-shaped dict, package or reference modules, converted once); with neither ``models`` nor
``set_default_models`` they raise instead of loading MANO per call as the reference does.  ``prepare_data(flag='device')`` keeps
everything on the device for ``arctic_metrics`` / ``ArcticEvaluator``; ``flag='eval'`` moves to the CPU as the reference."""
import math
import os
import warnings

import numpy as np
import torch

from . import _native
from . import arctic_output as _ao
from .arctic_item import get_arctic_item
from .arctic_output import matrix_to_axis_angle, matrix_to_quaternion, quaternion_to_axis_angle  # noqa: F401  (restated there)
from .mano import mano_many
from .object_tensors import ObjectTensors, objects_many
from .small_loss import _convert, contact_deviation

NN_MAX_PAIRS = _native.NN_MAX_PAIRS
METRIC_KEYS = ("aae", "mpjpe/ra/h", "mrrpe/r/l", "mrrpe/r/o", "success_rate/0.05", "cdev/ho")
DEFAULT_METRICS = ("aae", "mpjpe.ra", "mrrpe", "success_rate", "cdev", "mdev", "acc_err_pose")     # util/settings.py:29
_SKIPPED = ("mdev", "acc_err_pose")                                                                  # process.py:309
_METRIC_ROWS = {"aae": ("aae",), "mpjpe.ra": ("mpjpe/ra/h",), "mrrpe": ("mrrpe/r/l", "mrrpe/r/o"),
                "success_rate": ("success_rate/0.05",), "cdev": ("cdev/ho",)}


def _fused_enabled():
    return os.environ.get("MSDA_ARCTIC_EVAL_FUSED", "1") != "0"     # A/B knob: 0 = the torch restatements


_WARNED = set()


def _warn_restatement(what, why):
    """Once per cause: a CUDA call that the kernels could have served runs the (slower, possibly syncing) torch restatement."""
    if (what, why) not in _WARNED:
        _WARNED.add((what, why))
        warnings.warn("uvhand_amd.arctic_eval.%s: %s; running the torch restatement instead of the HIP kernel" % (what, why))


# ---- container ------------------------------------------------------------------------------------------------------------------
def _to(v, dev):
    if hasattr(v, "to"):
        return v.to(dev)
    if isinstance(v, (list, tuple)):
        return type(v)(_to(x, dev) for x in v)
    if isinstance(v, dict):
        return {k: _to(x, dev) for k, x in v.items()}
    return v


class XDict(dict):
    """What the reference's callers use of common/xdict.py: item assignment refuses an existing key (``overwrite`` replaces),
    ``search`` / ``prefix`` / ``rm`` / ``merge`` / ``to`` / ``to_np``."""

    def __init__(self, d=None):
        super().__init__()
        if d is not None:
            for k, v in d.items():
                dict.__setitem__(self, k, v)

    def __setitem__(self, key, val):
        assert key not in self, "Key already exists %s" % key
        dict.__setitem__(self, key, val)

    def overwrite(self, k, v):
        dict.__setitem__(self, k, v)

    def search(self, keyword, replace_to=None):
        return XDict({(k if replace_to is None else k.replace(keyword, replace_to)): v for k, v in self.items() if keyword in k})

    def rm(self, keyword, keep_list=()):
        return XDict({k: v for k, v in self.items() if keyword not in k or k in keep_list})

    def prefix(self, text):
        return XDict({text + k: v for k, v in self.items()})

    def merge(self, other):
        dup = set(self) & set(other)
        assert not dup, "Merge failed: duplicate keys (%s)" % dup
        self.update(other)

    def to(self, dev):
        return self if dev is None else XDict({k: _to(v, dev) for k, v in self.items()})

    def to_np(self):
        return XDict({k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in self.items()})


# ---- nearest neighbour ----------------------------------------------------------------------------------------------------------
def nn_reference(src_xyz, trg_xyz, k=1):
    """Brute force in torch, in the inputs' dtype: squared distance dx dx + dy dy + dz dz, lowest index on a tie, a NaN
    distance never wins (no finite candidate: +inf, index 0).  Differentiable in both arguments."""
    if k != 1:
        raise ValueError("get_NN: only k = 1 is provided")
    B, N1, _ = src_xyz.shape
    N2 = trg_xyz.shape[1]
    chunk = max(1, (1 << 22) // max(1, B * N2))
    ar = torch.arange(N2, device=src_xyz.device)
    dists, idxs = [], []
    for i0 in range(0, N1, chunk):
        diff = src_xyz[:, i0:i0 + chunk, None, :] - trg_xyz[:, None, :, :]
        d = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        m = d.detach().min(dim=2, keepdim=True).values
        idx = torch.where(d.detach() == m, ar, N2).min(dim=2).values
        dists.append(torch.gather(d, 2, idx[..., None])[..., 0])
        idxs.append(idx)
    return torch.cat(dists, 1), torch.cat(idxs, 1)


class _NNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *flat):
        pairs = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]
        outs = _native.nn_forward(pairs)
        ctx.save_for_backward(*flat, *[o[1] for o in outs])
        ctx.mark_non_differentiable(*[o[1] for o in outs])
        return tuple(t for o in outs for t in o)

    @staticmethod
    def backward(ctx, *grads):
        n = len(ctx.saved_tensors) // 3
        flat, idxs = ctx.saved_tensors[:2 * n], ctx.saved_tensors[2 * n:]
        pairs = [(flat[2 * i], flat[2 * i + 1]) for i in range(n)]
        want = [(ctx.needs_input_grad[2 * i], ctx.needs_input_grad[2 * i + 1]) for i in range(n)]
        gd = [grads[2 * i].contiguous() for i in range(n)]
        res = _native.nn_backward(pairs, list(idxs), gd, want)
        return tuple(g for pair in res for g in pair)


def _nn_why_not(pairs):
    """None when the kernels take these pairs (same shapes), else the reason."""
    s0, t0 = pairs[0]
    dev = s0.device
    if dev.type != "cuda" or not _fused_enabled():
        return "cpu or switched off"                 # the two silent causes
    if torch.is_autocast_enabled():
        return "autocast is on"
    for s, t in pairs:
        if s.dim() != 3 or t.dim() != 3 or s.shape[2] != 3 or t.shape[2] != 3 or s.shape[0] != t.shape[0]:
            return "expected src [B, N1, 3] and trg [B, N2, 3]"
        if any(x.device != dev or x.dtype != torch.float32 for x in (s, t)):
            return "inputs are not all fp32 on one device (got %s, %s)" % (s.dtype, t.dtype)
    if s0.shape[0] == 0 or not _native.nn_supported(s0.shape[0], s0.shape[1], t0.shape[1]):
        return "B = %d, N1 = %d, N2 = %d is outside msda_nn_supported" % (s0.shape[0], s0.shape[1], t0.shape[1])
    return None


def nn_many(pairs, k=1):
    """``[(dists, idx)]`` for pairs ``(src [B, N1, 3], trg [B, N2, 3])``: pairs of equal shapes (the two hands of a step) share
    one launch, at most NN_MAX_PAIRS per launch; pairs of other shapes get launches of their own."""
    if k != 1:
        raise ValueError("get_NN: only k = 1 is provided")
    pairs = [(s, t) for s, t in pairs]
    out = [None] * len(pairs)
    groups = {}
    for i, (s, t) in enumerate(pairs):
        groups.setdefault((tuple(s.shape), tuple(t.shape), s.device, s.dtype, t.dtype), []).append(i)
    for members in groups.values():
        for g0 in range(0, len(members), NN_MAX_PAIRS):
            ids = members[g0:g0 + NN_MAX_PAIRS]
            grp = [pairs[i] for i in ids]
            why = _nn_why_not(grp)
            if why is not None:
                if grp[0][0].is_cuda and _fused_enabled():
                    _warn_restatement("get_NN", why)
                res = [nn_reference(s, t) for s, t in grp]
            else:
                flat = [x.contiguous() for p in grp for x in p]
                if torch.is_grad_enabled() and any(x.requires_grad for x in flat):
                    o = _NNFunction.apply(*flat)
                    res = [(o[2 * i], o[2 * i + 1]) for i in range(len(grp))]
                else:
                    res = _native.nn_forward([(flat[2 * i], flat[2 * i + 1]) for i in range(len(grp))])
            for i, r in zip(ids, res):
                out[i] = r
    return out


def get_NN(src_xyz, trg_xyz, k=1):
    """Drop-in for loss_modules.get_NN: (squared nearest distance [B, N1], its index in trg [B, N1] int64)."""
    return nn_many([(src_xyz, trg_xyz)], k=k)[0]


# ---- glue -----------------------------------------------------------------------------------------------------------------------
_DEFAULT_MODELS = None


def set_default_models(models):
    """The ``pre_process_models``-shaped dict (``mano_l``, ``mano_r``, ``arti_head``) the glue uses when ``models`` is None."""
    global _DEFAULT_MODELS
    _DEFAULT_MODELS = models


def _models(models):
    models = _DEFAULT_MODELS if models is None else models
    if models is None:
        raise RuntimeError("arctic_eval: pass models= (mano_l, mano_r, arti_head) or call set_default_models once; the "
                           "reference builds two MANO heads and ObjectTensors from disk on every call, this package does not")
    if isinstance(models.get("arti_head"), torch.nn.Module) and hasattr(models["arti_head"], "object_tensors") \
            and not isinstance(models["arti_head"], ObjectTensors):
        models = dict(models, arti_head=models["arti_head"].object_tensors)        # the reference's ArtiHead
    return _convert(models)


_unnormalise = _ao.unnormalise


def _make_output(args, root, mano_pose, mano_shape, obj_angle, query_names, K, models=None, obj_idx=None, max_len=None):
    """``make_output`` and, on the device with the kernels switched on, what ``prepare_data`` derives from it and the launches
    have already produced: the pixel-space 2d keys and the axis-angle of ``mano.pose.*`` (else None)."""
    m = _models(models)
    root_l, root_r, root_o = root
    pose_l, pose_r = mano_pose
    shape_l, shape_r = mano_shape
    obj_rot, obj_rad = obj_angle
    img_res = args.img_res
    fused = K.is_cuda and _ao.fused_enabled()
    (mat_r, mat_l), (aa_r, aa_l), cam_ts = _ao.pose_heads((pose_r, pose_l), (root_r, root_l, root_o), K, img_res)
    hands = mano_many([(m["mano_r"], shape_r, aa_r[:, :3], aa_r[:, 3:]), (m["mano_l"], shape_l, aa_l[:, :3], aa_l[:, 3:])])
    obj = m["arti_head"]
    if obj_idx is None:
        obj_idx, max_len = obj.obj_index(query_names)
    elif max_len is None:
        raise ValueError("obj_idx needs a host max_len")
    out = objects_many([(obj, obj_rad.view(-1, 1), obj_rot, None, obj_idx, int(max_len))])[0]
    placed = _ao.place_many([(hands[0].vertices, 0, False), (hands[1].vertices, 1, False), (hands[0].joints, 0, True),
                             (hands[1].joints, 1, True), (out["kp3d"], 2, True), (out["bbox3d"], 2, True), (out["v"], 2, False)],
                            cam_ts, K, img_res, pixels=fused)
    output = XDict()
    extras = {} if fused else None
    for i, (s, hand, cam, shape, mat, aa) in enumerate((("r", hands[0], root_r, shape_r, mat_r, aa_r),
                                                        ("l", hands[1], root_l, shape_l, mat_l, aa_l))):
        for k, v in (("cam_t.wp", cam), ("cam_t", cam_ts[i]), ("joints3d", hand.joints), ("vertices", hand.vertices),
                     ("j3d.cam", placed[2 + i][0]), ("v3d.cam", placed[i][0]), ("j2d.norm", placed[2 + i][1]), ("beta", shape),
                     ("pose", mat)):
            output["mano.%s.%s" % (k, s)] = v
        if fused:
            extras["mano.j2d." + s] = placed[2 + i][2]
            extras["mano.pose." + s] = aa.reshape(-1, 16, 3)
    (kp3d_cam, kp2d, kp_px), (bbox3d_cam, bbox2d, bbox_px) = placed[4], placed[5]
    nk = kp2d.shape[1] // 2
    for k, v in (("rot", obj_rot), ("cam_t.wp", root_o), ("cam_t", cam_ts[2]), ("kp3d", out["kp3d"]), ("bbox3d", out["bbox3d"]),
                 ("bbox3d.cam", bbox3d_cam), ("kp3d.cam", kp3d_cam), ("kp2d.norm", kp2d), ("kp2d.norm.t", kp2d[:, :nk]),
                 ("kp2d.norm.b", kp2d[:, nk:]), ("bbox2d.norm.t", bbox2d[:, :8]), ("bbox2d.norm.b", bbox2d[:, 8:]),
                 ("radian", obj_rad), ("v.cam", placed[6][0]), ("v_len", out["v_len"]), ("f", out["f"]),
                 ("f_len", out["f_len"])):
        output["object." + k] = v
    if fused:
        extras.update({"object.kp2d": kp_px, "object.kp2d.t": kp_px[:, :nk], "object.kp2d.b": kp_px[:, nk:],
                       "object.bbox2d.t": bbox_px[:, :8], "object.bbox2d.b": bbox_px[:, 8:]})
    return output, extras


def make_output(args, root, mano_pose, mano_shape, obj_angle, query_names, K, models=None, obj_idx=None, max_len=None):
    """process.py:107-149: every key of MANOHead.forward (r, then l) and ArtiHead.forward, prefixed, in the reference's
    order.  ``obj_idx`` (int64 device tensor) with a host ``max_len`` replaces ``query_names`` for graph capture.  Device data:
    ``pose_heads``, ``mano_many``, ``objects_many``, ``place_many`` (four launches) and views."""
    return _make_output(args, root, mano_pose, mano_shape, obj_angle, query_names, K, models=models, obj_idx=obj_idx,
                        max_len=max_len)[0]


def _post_process(outputs, meta_info, args, cfg, models=None):
    root, mano_pose, mano_shape, obj_angle = get_arctic_item(outputs, cfg, getattr(args, "device", None))
    return _make_output(args, root, mano_pose, mano_shape, obj_angle, meta_info.get("query_names"), meta_info["intrinsics"],
                        models=models, obj_idx=meta_info.get("obj_idx"), max_len=meta_info.get("max_len"))


def post_process_arctic_output(outputs, meta_info, args, cfg, models=None):
    """process.py:95-105: query selection, then ``make_output``."""
    return _post_process(outputs, meta_info, args, cfg, models=models)[0]


def prepare_data(args, outputs, targets, meta_info, cfg, pred=None, flag='eval', models=None):
    """process.py:249-299.  ``flag``: 'eval' moves the result to the CPU (the reference), 'device' keeps it on the device for
    ``arctic_metrics`` / ``ArcticEvaluator``, 'train' keeps it (and the graph) for the SmoothNet criterion."""
    targets, meta_info = XDict(targets), XDict(meta_info)
    extras = None                                # what make_output's launches already hold of the keys derived below
    if pred is None:
        assert outputs is not None
        pred, extras = _post_process(outputs, meta_info, args, cfg, models=models)
    for key in list(pred.keys()):
        if "2d.norm" in key:
            denorm = key.replace(".norm", "")
            assert key in targets.keys(), "Do not have key %s" % key
            pred[denorm] = extras[denorm] if extras is not None else _unnormalise(pred[key], args.img_res)
            targets[denorm] = _unnormalise(targets[key], args.img_res)
    aa_r, aa_l = (extras["mano.pose.r"], extras["mano.pose.l"]) if extras is not None \
        else _ao.matrix_to_axis_angle_many([pred["mano.pose.r"], pred["mano.pose.l"]])
    pred.overwrite("mano.pose.r", aa_r)
    pred.overwrite("mano.pose.l", aa_l)
    (dr, ir), (dl, il) = nn_many([(pred["object.v.cam"], pred["mano.v3d.cam.r"]), (pred["object.v.cam"], pred["mano.v3d.cam.l"])])
    pred['nn_dist_r'], pred['nn_idx_r'] = dr, ir
    pred['nn_dist_l'], pred['nn_idx_l'] = dl, il
    data = XDict()
    data.merge(pred.prefix("pred."))
    data.merge(targets.prefix("targets."))
    data.merge(meta_info.prefix("meta_info."))
    if flag == 'eval':
        data = data.to("cpu")
    return data


# ---- metrics --------------------------------------------------------------------------------------------------------------------
def _nanmean(v, *args, **kwargs):
    is_nan = torch.isnan(v)
    v = v.masked_fill(is_nan, 0)
    return v.sum(*args, **kwargs) / (~is_nan).to(v.dtype).sum(*args, **kwargs)


def arctic_metrics_reference(data, dtype=torch.float32):
    """The six rows by the reference's control flow (eval_modules.py, metrics.py: per-frame loops and host copies), in
    ``dtype``; returns [6, B] on the data's device."""
    pred, targets, meta = data.search("pred.", ""), data.search("targets.", ""), data.search("meta_info.", "")
    f = lambda t: t.to(dtype)  # noqa: E731
    nan = float("nan")
    is_valid = f(targets["is_valid"])
    left_valid, right_valid = f(targets["left_valid"]) * is_valid, f(targets["right_valid"]) * is_valid
    dev = is_valid.device

    def invalid(v):
        return torch.nonzero((1 - v).long()).view(-1)

    # eval_degree
    aae = torch.abs(f(pred["object.radian"]).view(-1) / math.pi * 180 - f(targets["object.radian"]).view(-1) / math.pi * 180)
    aae[invalid(is_valid)] = nan
    # eval_mpjpe_ra
    jr_g, jl_g = f(targets["mano.j3d.cam.r"]), f(targets["mano.j3d.cam.l"])
    jr_p, jl_p = f(pred["mano.j3d.cam.r"]), f(pred["mano.j3d.cam.l"])
    per_hand = []
    for g, p, valid in ((jr_g, jr_p, right_valid), (jl_g, jl_p, left_valid)):
        dist = (((g - g[:, :1]) - (p - p[:, :1])) ** 2).sum(dim=2).sqrt()
        dist[invalid(valid), :] = nan
        per_hand.append(dist.mean(dim=1))
    mpjpe = _nanmean(torch.stack(per_hand, dim=1), dim=1) * 1000.0
    # object roots (eval_mrrpe, eval_v2v_success)
    v_len = [int(n) for n in targets["object.v_len"]]
    vg = [f(v)[:n] for v, n in zip(targets["object.v.cam"], v_len)]
    vp = [f(v)[:n] for v, n in zip(pred["object.v.cam"], v_len)]
    bottom = [(ids == 2).nonzero().view(-1) for ids in meta["part_ids"]]
    root_g = torch.stack([v[b].mean(dim=0) for v, b in zip(vg, bottom)], dim=0)
    root_p = torch.stack([v[b].mean(dim=0) for v, b in zip(vp, bottom)], dim=0)

    def mrrpe(r_g, l_g, r_p, l_p, valid):
        e = (((l_p - r_p) - (l_g - r_g)) ** 2).sum(dim=1).sqrt()
        e[invalid(valid)] = nan
        return e * 1000.0
    mrrpe_rl = mrrpe(jr_g[:, 0], jl_g[:, 0], jr_p[:, 0], jl_p[:, 0], left_valid * right_valid)
    mrrpe_ro = mrrpe(jr_g[:, 0], root_g, jr_p[:, 0], root_p, right_valid * is_valid)
    # eval_v2v_success
    diameter = f(meta["diameter"])
    rates = []
    for g, p, rg, rp, d, valid in zip(vg, vp, root_g, root_p, diameter, is_valid):
        if bool(valid):
            dist = (((g - rg[None, :]) - (p - rp[None, :])) ** 2).sum(dim=1).sqrt()
            ok = (dist < d * 0.05).to(dtype)
            rates.append(ok.sum() / ok.shape[0])
        else:
            rates.append(torch.tensor(nan, dtype=dtype, device=dev))
    success = torch.stack(rates) * 100.0
    # eval_contact_deviation
    vo = f(pred["object.v.cam"])
    cd_ro = contact_deviation(vo, f(pred["mano.v3d.cam.r"]), f(targets["dist.ro"]), targets["idx.ro"], is_valid, f(targets["right_valid"]))
    cd_lo = contact_deviation(vo, f(pred["mano.v3d.cam.l"]), f(targets["dist.lo"]), targets["idx.lo"], is_valid, f(targets["left_valid"]))
    cdev = _nanmean(torch.stack((cd_ro, cd_lo), dim=1), dim=1) * 1000
    return torch.stack([aae, mpjpe, mrrpe_rl, mrrpe_ro, success, cdev], dim=0)


_FLOAT_KEYS = ("pred.object.radian", "targets.object.radian", "pred.mano.j3d.cam.r", "pred.mano.j3d.cam.l", "targets.mano.j3d.cam.r",
               "targets.mano.j3d.cam.l", "pred.object.v.cam", "targets.object.v.cam", "meta_info.diameter", "targets.is_valid",
               "targets.left_valid", "targets.right_valid", "pred.mano.v3d.cam.r", "pred.mano.v3d.cam.l", "targets.dist.ro",
               "targets.dist.lo")
_LONG_KEYS = ("targets.object.v_len", "meta_info.part_ids", "targets.idx.ro", "targets.idx.lo")


def _metrics_plan(data):
    """(dims, floats, longs) for the kernel, or None where the restatement runs (with a warning, once per cause, when the
    data is on the device and the kernels are not switched off)."""
    fl, lo = [data[k] for k in _FLOAT_KEYS], [data[k] for k in _LONG_KEYS]
    dev = fl[9].device if torch.is_tensor(fl[9]) else torch.device("cpu")
    if not _fused_enabled() or dev.type != "cuda":
        return None
    no = lambda why: _warn_restatement("arctic_metrics", why)  # noqa: E731
    if torch.is_autocast_enabled():
        return no("autocast is on")
    for k, t in zip(_FLOAT_KEYS + _LONG_KEYS, fl + lo):
        want = torch.float32 if k in _FLOAT_KEYS else torch.int64
        if not torch.is_tensor(t) or t.device != dev or t.dtype != want:
            return no("%r must be a %s tensor on %s (got %s)" % (k, want, dev, "%s on %s" % (t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    B = fl[9].shape[0]
    jp, vh, vp, vg, parts = fl[2], fl[12], fl[6], fl[7], lo[1]
    if B == 0 or jp.dim() != 3 or vh.dim() != 3 or vp.dim() != 3 or vg.dim() != 3 or parts.dim() != 2:
        return no("unexpected tensor ranks")
    J, NV = jp.shape[1], vh.shape[1]
    dims = [B, J, NV, vp.shape[1], vg.shape[1], parts.shape[1]]
    shapes = [(B,), (B,), (B, J, 3), (B, J, 3), (B, J, 3), (B, J, 3), (B, dims[3], 3), (B, dims[4], 3), (B,), (B,), (B,), (B,),
              (B, NV, 3), (B, NV, 3), (B, NV), (B, NV), (B,), (B, dims[5]), (B, NV), (B, NV)]
    ts = [t.reshape(-1) if s == (B,) else t for t, s in zip(fl + lo, shapes)]
    if any(tuple(t.shape) != s for t, s in zip(ts, shapes)) or not _native.arctic_metrics_supported(*dims):
        return no("shapes %s are outside msda_arctic_metrics_supported or inconsistent" % (dims,))
    ts = [t.detach().contiguous() for t in ts]
    return dims, ts[:len(fl)], ts[len(fl):]


def arctic_metrics(data, metrics=DEFAULT_METRICS):
    """[6, B] fp32 on the data's device, rows in METRIC_KEYS (every row is computed whatever ``metrics`` asks for)."""
    _rows(metrics)
    plan = _metrics_plan(data)
    if plan is None:
        return arctic_metrics_reference(data).to(torch.float32)
    return _native.arctic_metrics(*plan)


def _rows(metrics):
    keys = []
    for metric in metrics:
        if metric in _SKIPPED:
            continue
        if metric not in _METRIC_ROWS:
            raise NotImplementedError("arctic_eval: metric %r needs the field model's outputs and is not provided" % (metric,))
        keys += _METRIC_ROWS[metric]
    return keys


def arctic_metrics_dict(data, metrics=DEFAULT_METRICS):
    """{key: [B] view} of ``arctic_metrics`` for the requested metrics, in ``measure_error``'s order."""
    vals = arctic_metrics(data, metrics)
    return {k: vals[METRIC_KEYS.index(k)] for k in _rows(metrics)}


def measure_error(data, metrics):
    """Drop-in for process.py:301-314: {key: [B] numpy array} (success_rate in fp64 as the reference's, the rest fp32).  On
    device data: the metric launch and one copy."""
    keys = _rows(metrics)
    vals = arctic_metrics(data, metrics).cpu().numpy()
    out = XDict()
    for k in keys:
        row = vals[METRIC_KEYS.index(k)]
        out[k] = row.astype(np.float64) if k.startswith("success_rate") else row
    return out


class ArcticEvaluator:
    """engine.py:784-794 + MetricLogger: ``update(data)`` adds each key's mean over the step's non-NaN frames to a running
    total (a key that is all NaN in a step is dropped for that step); ``compute()`` returns ``{key: total / count}`` for the
    keys that were ever present (``meter.global_avg``).  On device data ``update`` is two launches and no sync."""

    def __init__(self, metrics=DEFAULT_METRICS):
        self.keys = _rows(metrics)
        self.metrics = tuple(metrics)
        self.total = self.count = None

    def reset(self):
        if self.total is not None:
            self.total.zero_()
            self.count.zero_()

    def update(self, data):
        vals = arctic_metrics(data, self.metrics)
        if self.total is None or self.total.device != vals.device:
            self.total = torch.zeros(len(METRIC_KEYS), dtype=torch.float64, device=vals.device)
            self.count = torch.zeros(len(METRIC_KEYS), dtype=torch.float64, device=vals.device)
        if vals.is_cuda and _fused_enabled():
            _native.arctic_metrics_accumulate(vals.contiguous(), self.total, self.count)
        else:
            ok = ~torch.isnan(vals)
            n = ok.sum(dim=1).to(torch.float64)
            s = vals.to(torch.float64).masked_fill(~ok, 0).sum(dim=1)
            self.total += torch.where(n > 0, s / n.clamp(min=1), torch.zeros_like(s))
            self.count += (n > 0).to(torch.float64)
        return vals

    def compute(self):
        if self.total is None:
            return {}
        tc = torch.stack([self.total, self.count]).cpu()
        return {k: float(tc[0, i] / tc[1, i]) for i, k in enumerate(METRIC_KEYS) if k in self.keys and tc[1, i] > 0}
