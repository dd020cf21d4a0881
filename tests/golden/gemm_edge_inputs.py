"""Edge-shape cases of the two grouped fp32-MFMA GEMM families (csrc/msda_heads.hip, csrc/msda_smoother.hip) and what
tests/test_gemm_edges*.py share about them: seeded builders, the fp64 references, the loss weights, the comparison regions
and the tolerances.  Nothing here needs a GPU; the GPU test runs the same helpers with the HIP entry points.

Every case lies inside the support predicates (msda_heads_supported, msda_smoother_supported) and the Python route checks,
so it takes the fused kernels.  The tile is 64 x 64 with K stages of 32 (csrc/msda_tile.h); the heads' weight gradients are
summed in row chunks of 2048 (kHeadsWgradChunk, csrc/msda_launch.h)."""
import copy
import math

import torch
import torch.nn.functional as F
from torch import nn

from uvhand_amd.functions.heads_func import ARCTIC, ASSEMBLY, detr_heads_reference
from uvhand_amd.functions.smoother_func import motion_smoothers_reference
from uvhand_amd.modules.detr import MLP
from uvhand_amd.modules.smoothnet import MotionSmoother

TILE, STAGE, CHUNK = 64, 32, 2048
SHARED_WIDTHS = (48, 10, 3, 3, 3, 1)          # ARCTIC's six shared Linears (_native.HEADS_SHARED_WIDTHS)

# ---- tolerances -----------------------------------------------------------------------------------------------------------
# The suite's fp32-MFMA bounds (tests/test_detr_gpu.py) for the max-normalised error of a tensor or region.  gfx950's f32
# MFMA rounds like fp32 FMA, so the error of a reduction over n terms grows with n: each of the n accumulations rounds a
# partial sum by at most 2^-24 relative, with independent signs, so the sum's error is about 2^-24 * sqrt(n) * sum|t_k| over
# a result of size ~|sum t_k|.  Normalising by the region's maximum keeps that ratio O(1); c = 16 covers it and the fp32
# error already in the operands (earlier layers).  A bound only rises above ACT / GRAD where 16 * 2^-24 * sqrt(n) does: n
# above ~1100 for outputs, ~11 000 for weight gradients.  No bound exceeds 1e-3.
ACT, GRAD = 2e-5, 1e-4
MARGIN = 10.0                                  # each mutation must miss the reference by this multiple of its tolerance


def bound(base, n):
    return min(1e-3, max(base, 16 * 2.0 ** -24 * math.sqrt(n)))


# ReLU / LeakyReLU kinks: an fp32 pre-activation within rounding of 0 may take the other branch than fp64 and flip one
# term of the backward.  Rows (the heads and smoothers treat every row on its own) with an fp64 pre-activation within 64 times
# the typical fp32 dot-product error, 2^-24 * sum_k |x_k w_k|, get zero loss weight: their gradients are 0 on both sides.
KINK = 64 * 2.0 ** -24

# ---- heads cases ----------------------------------------------------------------------------------------------------------
# name: (kind, levels share their modules, L, B, Q, C, K, R (0: ARCTIC one-stage, no keypoint MLPs), seed)
HEADS_CASES = {
    "arctic_chunked": (ARCTIC, False, 6, 2, 1025, 256, 14, 42, 501),   # M 2050: 2-row tail chunks; 12300 shared rows
    "assembly_one_chunk": (ASSEMBLY, False, 1, 1, 2048, 256, 7, 42, 502),  # M 2048: one full chunk
    "assembly_shared_tail": (ASSEMBLY, True, 3, 1, 683, 256, 7, 2, 503),   # L * M 2049: a 1-row tail chunk
    "c4": (ASSEMBLY, False, 2, 2, 37, 4, 7, 2, 504),
    "c36": (ARCTIC, False, 3, 1, 70, 36, 14, 42, 505),
    "c100": (ASSEMBLY, True, 2, 3, 23, 100, 7, 42, 506),
    "c260": (ARCTIC, True, 2, 2, 45, 260, 14, 42, 507),
    "k1_one_stage": (ARCTIC, False, 2, 1, 50, 256, 1, 0, 508),
    "k65": (ASSEMBLY, False, 2, 1, 130, 128, 65, 2, 519),
    "l8": (ARCTIC, False, 8, 1, 33, 64, 14, 42, 510),
    "b1_q1": (ASSEMBLY, False, 3, 1, 1, 256, 7, 42, 511),
}


def heads_n_mlp(kind, R):
    return 0 if R == 0 else (2 if kind == ARCTIC else 1)


def heads_build(name):
    """(kind, modules (cls, mlps, shared), hs, init, inter, output weights) in fp32 on the CPU."""
    kind, shared, L, B, Q, C, K, R, seed = HEADS_CASES[name]
    torch.manual_seed(seed)
    n = 1 if shared else L
    cls = [nn.Linear(C, K) for _ in range(n)]
    cls = nn.ModuleList(cls * L if shared else cls)
    mlps = []
    for _ in range(heads_n_mlp(kind, R)):
        m = [MLP(C, C, 42 if kind == ARCTIC else 63, 3) for _ in range(n)]
        mlps.append(nn.ModuleList(m * L if shared else m))
    sh = nn.ModuleList(nn.Linear(C, w) for w in SHARED_WIDTHS) if kind == ARCTIC else None
    g = torch.Generator().manual_seed(seed + 1)
    hs = torch.randn(L, B, Q, C, generator=g) * 0.5
    init = inter = None
    if R:
        init = torch.rand(B, Q, R, generator=g) * 2.4 - 1.2
        inter = torch.rand(L, B, Q, R, generator=g) * 2.4 - 1.2
        if kind == ASSEMBLY:
            init = init.abs().clamp(max=1)
    D = 42 if kind == ARCTIC else 63
    widths = [K] + [D] * len(mlps) + (list(SHARED_WIDTHS) if kind == ARCTIC else [])
    weights = [torch.randn(L, B, Q, w, generator=g) for w in widths]
    return kind, (cls, mlps, sh), hs, init, inter, weights


def heads_param_items(mods):
    """[(name, parameter)] of the distinct modules, in a fixed order."""
    cls, mlps, sh = mods
    items, seen = [], set()
    groups = [("cls", list(cls))] + [("mlp%d" % h, list(m)) for h, m in enumerate(mlps)] + [("sh", list(sh or []))]
    for tag, ms in groups:
        for i, m in enumerate(ms):
            if id(m) in seen:
                continue
            seen.add(id(m))
            items += [("%s.%d.%s" % (tag, i, k), p) for k, p in m.named_parameters()]
    return items


def heads_chunk_masks(name):
    """{set name: row mask [L, B, Q]} for the weight-gradient chunks: per-level problems chunk the M rows of each level,
    the problems over every level (shared Linears, shared levels) the L * M flattened rows.  Only where a problem has more
    than one chunk."""
    _, _, L, B, Q, _, _, _, _ = HEADS_CASES[name]
    M = B * Q
    out = {}
    if M > CHUNK:
        idx = torch.arange(M).view(1, B, Q).expand(L, B, Q)
        for c in range((M + CHUNK - 1) // CHUNK):
            out["lvlchunk%d" % c] = (idx // CHUNK) == c
    if L * M > CHUNK:
        idx = torch.arange(L * M).view(L, B, Q)
        for c in range((L * M + CHUNK - 1) // CHUNK):
            out["chunk%d" % c] = (idx // CHUNK) == c
    return out


def heads_problem_rows(name, pname):
    """(chunk family, rows reduced) of the weight-gradient problem behind parameter `pname`."""
    kind, shared, L, B, Q, _, _, _, _ = HEADS_CASES[name]
    over_levels = pname.startswith("sh.") or shared
    return ("chunk" if over_levels else "lvlchunk"), (L * B * Q if over_levels else B * Q)


def heads_results(kind, mods, hs, init, inter, weights, sets, fn, record=False, count=None):
    """Forward once, then one backward per weight set: {set: {key: tensor}} ("out/..." in set "full" only).  `sets` maps a
    set name to a row mask [L, B, Q] (None: every row).  `record`: also the fp64 kink rows and the layer-0 gradients."""
    cls, mlps, sh = mods
    recs, hooks = [], []
    if record:
        def hook(mod, inp, out):
            recs.append((inp[0], out, mod))
        for mlp in mlps:
            for m in {id(x): x for x in mlp}.values():
                hooks += [m.layers[0].register_forward_hook(hook), m.layers[1].register_forward_hook(hook)]
    hs = hs.detach().clone().requires_grad_(True)
    items = heads_param_items(mods)
    n0 = count() if count else 0
    try:
        logits, keys, outs = fn(kind, hs, init, inter, cls, mlps, sh)
    finally:
        for h in hooks:
            h.remove()
    n1 = count() if count else 0
    flat = [logits] + list(keys) + list(outs)
    names = ["logits"] + ["kp%d" % h for h in range(len(keys))] + ["sh%d" % g for g in range(len(outs))]
    res, extra = {}, {}
    res["full"] = {"out/" + k: t.detach() for k, t in zip(names, flat)}
    L = hs.shape[0]
    z0 = [recs[(l * len(mlps) + h) * 2][1] for l in range(L) for h in range(len(mlps))] if record else []
    launches = None
    for sname, mask in sets.items():
        loss = 0
        for t, w in zip(flat, weights):
            w = w.to(t.device, t.dtype)
            if mask is not None:
                w = w * mask.to(t.device, t.dtype)[..., None]
            loss = loss + (t * w).sum()
        grads = torch.autograd.grad(loss, [hs] + [p for _, p in items] + z0, retain_graph=True)
        if launches is None and count:
            launches = (n1 - n0, count() - n1)
        d = res.setdefault(sname, {})
        d["grad/hs"] = grads[0]
        d.update({"grad/" + k: g for (k, _), g in zip(items, grads[1:1 + len(items)])})
        if sname == "full" and record:
            extra["dz0"] = [g.detach() for g in grads[1 + len(items):]]
    if record:
        kink = torch.zeros(hs.shape[:3], dtype=torch.bool)
        for l in range(L):
            for x, z, m in recs[l * 2 * len(mlps):(l + 1) * 2 * len(mlps)]:
                scale = x.detach().abs() @ m.weight.detach().abs().t() + m.bias.detach().abs()
                kink[l] |= (z.detach().abs() < KINK * scale).any(-1)
        extra["kink"] = kink
    return res, extra, launches


def heads_reference(name, sets_extra=True):
    """The fp64 CPU reference of a case: (case objects, loss weights with the kink rows zeroed, weight sets, results,
    extra).  detr_heads_reference on .double() copies of the modules."""
    kind, mods, hs, init, inter, weights = heads_build(name)
    d_mods = copy.deepcopy(mods)
    for m in d_mods:
        for x in (m if isinstance(m, list) else [m]):
            if x is not None:
                x.double()
    d = [t.double() if t is not None else None for t in (hs, init, inter)]
    # the kink rows first (their weights do not matter for the forward)
    _, extra, _ = heads_results(kind, d_mods, *d, [w.double() for w in weights], {}, detr_heads_reference, record=True)
    keep = (~extra["kink"]).to(torch.float32)[..., None]
    weights = [w * keep for w in weights]
    sets = {"full": None}
    if sets_extra:
        sets.update(heads_chunk_masks(name))
    res, extra2, _ = heads_results(kind, d_mods, *d, [w.double() for w in weights], sets, detr_heads_reference,
                                   record=True)
    extra2["kink"] = extra["kink"]
    return (kind, mods, hs, init, inter), d_mods, weights, sets, res, extra2


def heads_tol(name, key):
    kind, _, L, B, Q, C, K, R, _ = HEADS_CASES[name]
    if key.startswith("out/"):
        return bound(ACT, C)
    if key == "grad/hs":
        return bound(GRAD, K + 2 * C + sum(SHARED_WIDTHS))
    return bound(GRAD, heads_problem_rows(name, key[5:])[1])


def _tail(n):
    return slice(TILE * ((n - 1) // TILE), n)


def _mask_slice(shape, axis, sl):
    m = torch.zeros(shape, dtype=torch.bool)
    m[(slice(None),) * axis + (sl,)] = True
    return m


def heads_regions(name, key, shape):
    """{region: bool mask of `shape`}: all, the rows of the last (partial) 64-row tile, the last (partial) 64-column tile.
    Outputs and grad/hs are [L, B, Q, n] (rows per level, or over L * M for the shared Linears); weights [n, C]."""
    _, _, L, B, Q, _, _, _, _ = HEADS_CASES[name]
    regions = {"all": torch.ones(shape, dtype=torch.bool)}
    if key.startswith("out/") or key == "grad/hs":
        M, n = B * Q, shape[-1]
        if key.startswith("out/sh"):
            rows = torch.arange(L * M).view(L, B, Q) >= TILE * ((L * M - 1) // TILE)
        else:
            rows = (torch.arange(M).view(1, B, Q) >= TILE * ((M - 1) // TILE)).expand(L, B, Q)
        regions["tail_rows"] = rows[..., None].expand(shape).clone()
        regions["tail_cols"] = _mask_slice(shape, 3, _tail(n))
    else:
        regions["tail_rows"] = _mask_slice(shape, 0, _tail(shape[0]))
        if len(shape) == 2:
            regions["tail_cols"] = _mask_slice(shape, 1, _tail(shape[1]))
    return regions


# ---- smoother cases -------------------------------------------------------------------------------------------------------
# name: (T, O, H, R, num_blocks, calls [(module, B, C)], dropout p (None: eval), seed)
SMOOTHER_CASES = {
    "minimal": (3, 1, 4, 4, 0, [(0, 2, 3)], None, 601),                       # acc window 1, no residual block
    "o_gt_t": (5, 9, 36, 100, 1, [(0, 3, 7), (0, 1, 2)], None, 602),
    "four_blocks": (6, 6, 260, 68, 4, [(0, 2, 5), (1, 1, 9)], None, 603),
    "t67": (67, 33, 64, 32, 2, [(0, 2, 11)], None, 604),                        # encoder K: 3 stages with tails
    "t1030": (1030, 16, 64, 32, 1, [(0, 1, 3)], None, 605),
    "rows_19k": (8, 8, 64, 32, 2, [(0, 64, 150), (0, 36, 267)], None, 606),    # 9600 + 9612 rows on one module
    "twelve_calls": (12, 12, 64, 32, 1, [(0, 2, 3), (1, 1, 1), (0, 1, 1), (2, 3, 5), (0, 2, 4), (3, 1, 2), (4, 2, 1),
                                         (0, 1, 7), (5, 1, 3), (1, 2, 2), (2, 1, 1), (3, 2, 6)], None, 617),
    "train_four_blocks": (6, 6, 260, 68, 4, [(0, 2, 5), (1, 1, 9)], 0.7, 608),
}


def smoother_build(name):
    """(modules, calls [(m, x [B, T, C])], output weights) in fp32 on the CPU."""
    T, O, H, R, nb, calls, p, seed = SMOOTHER_CASES[name]
    torch.manual_seed(seed)
    n_mod = max(m for m, _, _ in calls) + 1
    mods = [MotionSmoother(T, O, H, R, nb, dropout=0.0 if p is None else p) for _ in range(n_mod)]
    for m in mods:
        m.train(p is not None)
    g = torch.Generator().manual_seed(seed + 1)
    xs = [(m, torch.randn(B, T, C, generator=g)) for m, B, C in calls]
    weights = [torch.randn(B, O, C, generator=g) for _, B, C in calls]
    return mods, xs, weights


def smoother_module_rows(name):
    """[(module, row0, rows)] per call, and rows per module (calls of a module concatenate their B * C rows)."""
    calls = SMOOTHER_CASES[name][5]
    rows, out = {}, []
    for m, B, C in calls:
        out.append((m, rows.get(m, 0), B * C))
        rows[m] = rows.get(m, 0) + B * C
    return out, rows


def smoother_param_items(mods):
    return [("m%d.%s" % (k, n), p) for k, m in enumerate(mods) for n, p in m.named_parameters()]


def _near_kink(z, x, lin_w, lin_b, keep=None):
    scale = x.abs() @ lin_w.abs().t() + lin_b.abs()
    near = z.abs() < KINK * scale
    if keep is not None:
        near = near & (keep > 0)
    return near.any(-1)


def smoother_composition(m, x, masks=None, p=0.0, kink=None):
    """MotionSmoother.forward with dropout = multiplication by masks[(s, layer)] [B, C, n] / (1 - p) (None: eval), in the
    dtype of x; `kink` [B, C] collects the rows with a pre-activation near a LeakyReLU kink."""
    xp = x.permute(0, 2, 1)
    vel = xp[..., 1:] - xp[..., :-1]
    acc = vel[..., 1:] - vel[..., :-1]
    outs = []
    for s, (sm, inp) in enumerate(zip((m.pos_smoother, m.vel_smoother, m.acc_smoother), (xp, vel, acc))):
        enc = sm.encoder[0]
        z = F.linear(inp, enc.weight, enc.bias)
        if kink is not None:
            kink |= _near_kink(z.detach(), inp.detach(), enc.weight.detach(), enc.bias.detach())
        h = F.leaky_relu(z, 0.1)
        for j, blk in enumerate(sm.res_blocks, start=1):
            for layer, lin in ((2 * j - 1, blk.linear1), (2 * j, blk.linear2)):
                src = h if layer % 2 else u
                z = F.linear(src, lin.weight, lin.bias)
                keep = None
                if masks is not None:
                    keep = masks[(s, layer)]
                    z = z * keep * (1.0 / (1.0 - p))
                if kink is not None:
                    sc = 1.0 if masks is None else 1.0 / (1.0 - p)
                    kink |= _near_kink(z.detach(), src.detach() * sc, lin.weight.detach(), lin.bias.detach() * sc, keep)
                if layer % 2:
                    u = F.leaky_relu(z, 0.2)
                else:
                    h = F.leaky_relu(z, 0.2) + h
        outs.append(sm.decoder(h))
    return m.fusion_layer(torch.cat(outs, dim=2)).permute(0, 2, 1)


def smoother_call_masks(name, masks):
    """Per call {(s, layer): mask [B, C, n]} from per-module masks {(m, s, layer): [rows_m, n]}."""
    per_call, _ = smoother_module_rows(name)
    out = []
    for (m, row0, rows), (_, B, C) in zip(per_call, SMOOTHER_CASES[name][5]):
        out.append({(s, l): t[row0:row0 + rows].reshape(B, C, -1) for (mm, s, l), t in masks.items() if mm == m})
    return out


def smoother_mask_shapes(name):
    """{(m, s, layer): (rows_m, n)} of every dropout layer."""
    T, O, H, R, nb, calls, p, _ = SMOOTHER_CASES[name]
    _, rows = smoother_module_rows(name)
    return {(m, s, l): (rows[m], R if l % 2 else H) for m in sorted(rows) for s in range(3) for l in range(1, 2 * nb + 1)}


def smoother_cpu_masks(name, seed=77):
    """Stand-in keep masks for the CPU test of a train-mode case (the GPU test uses the kernels' own)."""
    p = SMOOTHER_CASES[name][6]
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(*shape, generator=g) >= p).double() for k, shape in smoother_mask_shapes(name).items()}


def smoother_results(mods, xs, weights, sets, fn, count=None):
    """Forward once, one backward per weight set: {set: {key: tensor}}.  `sets`: name -> per-call row masks [B, C] (None:
    every row).  fn(calls, modules) -> outputs [B, O, C]."""
    leaves = [(m, x.detach().clone().requires_grad_(True)) for m, x in xs]
    items = smoother_param_items(mods)
    n0 = count() if count else 0
    outs = fn(leaves, mods)
    n1 = count() if count else 0
    res = {"full": {"out/%d" % i: o.detach() for i, o in enumerate(outs)}}
    launches = None
    for sname, rmask in sets.items():
        loss = 0
        for i, (o, w) in enumerate(zip(outs, weights)):
            w = w.to(o.device, o.dtype)
            if rmask is not None:
                w = w * rmask[i].to(o.device, o.dtype)[:, None, :]
            loss = loss + (o * w).sum()
        grads = torch.autograd.grad(loss, [x for _, x in leaves] + [p for _, p in items], retain_graph=True)
        if launches is None and count:
            launches = (n1 - n0, count() - n1)
        d = res.setdefault(sname, {})
        d.update({"grad/x%d" % i: g for i, g in enumerate(grads[:len(leaves)])})
        d.update({"grad/" + k: g for (k, _), g in zip(items, grads[len(leaves):])})
    return res, launches


def smoother_row_sets(name):
    """Weight sets of the CPU mutations: the last call of each module, and the rows of each module's last 32-row stage of
    the weight-gradient reduction."""
    per_call, rows = smoother_module_rows(name)
    calls = SMOOTHER_CASES[name][5]
    last_call = {m: max(i for i, (mm, _, _) in enumerate(per_call) if mm == m) for m in rows}
    lastcall, laststage = [], []
    for i, ((m, row0, r), (_, B, C)) in enumerate(zip(per_call, calls)):
        lastcall.append(torch.full((B, C), float(last_call[m] == i)))
        mrow = row0 + torch.arange(r).view(B, C)
        laststage.append((mrow >= STAGE * ((rows[m] - 1) // STAGE)).double())
    return {"lastcall": lastcall, "laststage": laststage}


def smoother_reference(name, masks=None, extra_sets=False):
    """The fp64 CPU reference of a case: (fp32 case objects, fp64 modules, loss weights with the kink rows zeroed, results).
    Eval: motion_smoothers_reference on .double() copies; train: the masked composition with `masks` {(m, s, layer)}."""
    T, O, H, R, nb, calls, p, _ = SMOOTHER_CASES[name]
    mods, xs, weights = smoother_build(name)
    d_mods = [copy.deepcopy(m).double() for m in mods]
    cm = smoother_call_masks(name, {k: v.double() for k, v in masks.items()}) if p is not None else None
    with torch.no_grad():
        for i, (m, x) in enumerate(xs):
            kink = torch.zeros(x.shape[0], x.shape[2], dtype=torch.bool)
            smoother_composition(d_mods[m], x.double(), cm[i] if cm else None, p or 0.0, kink)
            weights[i] = weights[i] * (~kink).to(torch.float32)[:, None, :]
    if p is None:
        def fn(leaves, ms):
            return motion_smoothers_reference(leaves, ms, False)
    else:
        def fn(leaves, ms):
            return [smoother_composition(ms[m], x, cm[i], p) for i, (m, x) in enumerate(leaves)]
    sets = {"full": None}
    if extra_sets:
        sets.update(smoother_row_sets(name))
    res, _ = smoother_results(d_mods, [(m, x.double()) for m, x in xs], weights, sets, fn)
    return (mods, xs), d_mods, weights, res


def smoother_tol(name, key):
    T, O, H, R, nb, calls, p, _ = SMOOTHER_CASES[name]
    if key.startswith("out/"):
        return bound(ACT, max(T, 3 * O, H, R))
    if key.startswith("grad/x"):
        return bound(GRAD, max(3 * O, H, R, O))
    return bound(GRAD, smoother_module_rows(name)[1][int(key.split(".")[0][len("grad/m"):])])


def smoother_regions(name, key, shape):
    """{region: bool mask}: all, the (b, c) rows of each module's last 64-row tile, the last 64-column tile (O of an output,
    T of an input gradient, the columns of a weight gradient); weight rows: the last 64-row tile of n."""
    regions = {"all": torch.ones(shape, dtype=torch.bool)}
    if key.startswith("out/") or key.startswith("grad/x"):
        i = int(key.split("/")[1].lstrip("x"))
        per_call, rows = smoother_module_rows(name)
        m, row0, _ = per_call[i]
        B, _, C = shape
        mrow = row0 + torch.arange(B * C).view(B, 1, C)
        regions["tail_rows"] = (mrow >= TILE * ((rows[m] - 1) // TILE)).expand(shape).clone()
        regions["tail_cols"] = _mask_slice(shape, 1, _tail(shape[1]))
    else:
        regions["tail_rows"] = _mask_slice(shape, 0, _tail(shape[0]))
        if len(shape) == 2:
            regions["tail_cols"] = _mask_slice(shape, 1, _tail(shape[1]))
    return regions


# ---- comparison -----------------------------------------------------------------------------------------------------------
def region_err(got, ref, mask):
    """max |got - ref| over the region relative to max |ref| over the region."""
    got = got.detach().cpu().double()[mask]
    ref = ref.detach().cpu().double()[mask]
    if ref.numel() == 0:
        return 0.0
    diff = (got - ref).abs().max().item()
    top = ref.abs().max().item()
    if top == 0.0:
        return 0.0 if diff == 0.0 else math.inf
    return diff / top


def compare(got, ref, regions_of, tol_of):
    """{(set, key, region): (err, tol)} over every tensor of the reference results."""
    out = {}
    for sname, tensors in ref.items():
        for key, r in tensors.items():
            tol = tol_of(key)
            for region, mask in regions_of(key, tuple(r.shape)).items():
                out[(sname, key, region)] = (region_err(got[sname][key], r, mask), tol)
    return out
