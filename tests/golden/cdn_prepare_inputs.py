"""Cases, seeded targets and parameters of the denoising-query fixture (cdn_prepare.npz), rebuilt wherever they are needed
instead of being stored: gen_cdn_prepare.py (which ran the reference's prepare_for_cdn on them) and tests/test_cdn_prepare*.py
(which run the product on them) call the same functions.  Test infrastructure, no reference code."""
import numpy as np
import torch
from torch import nn

W = 42                         # keypoint values per target (the reference's padding rows are 42 wide)
NUM_CLASSES = 14               # labels are drawn from [0, NUM_CLASSES); label_enc has one row more, as DINO builds it
QUERIES = 5                    # matching queries behind the denoising rows

# sizes: targets per frame; dn: dn_number as the caller passes it; ratio / box: label_noise_ratio / box_noise_scale;
# torch_seed: manual_seed before the call (cases that draw).  The group-count branches: dn 2 is used as 4 after the doubling;
# 100 with at most 3 targets gives 200 // 6 = 33; 50 with a frame of 60 targets gives 100 // 120 = 0, floored to 1; a step
# without any target has one group and pad_size 0.  No drawing case has an empty frame: there the reference itself raises
# (torch.tensor([]) of :36 is a float tensor, the concatenated labels become float and scatter_ of :78 refuses the int64 draws).
CASES = {
    "one_h8": dict(sizes=(1,), dn=2, ratio=0.0, box=0.0, hidden=8, seed=5101),
    "mixed_h256": dict(sizes=(2, 0, 3), dn=2, ratio=0.0, box=0.4, hidden=256, seed=5102),
    "div33_h8": dict(sizes=(3, 1), dn=100, ratio=0.0, box=0.0, hidden=8, seed=5103),
    "floor1_h8": dict(sizes=(60, 2), dn=50, ratio=0.0, box=1.0, hidden=8, seed=5104),
    "empty_h8": dict(sizes=(0, 0), dn=2, ratio=0.0, box=0.4, hidden=8, seed=5105),
    "flip_one_h8": dict(sizes=(1,), dn=2, ratio=0.5, box=0.0, hidden=8, seed=5106, torch_seed=61),
    "flip_div33_h8": dict(sizes=(3, 1), dn=100, ratio=0.5, box=0.4, hidden=8, seed=5107, torch_seed=62),
    "flip_pair_h256": dict(sizes=(2, 3), dn=2, ratio=0.5, box=0.4, hidden=256, seed=5108, torch_seed=63),
}
SMALL = [k for k, c in CASES.items() if sum(c["sizes"]) <= 8]          # the cases the GPU tests run
EXPECTED_GROUPS = {"one_h8": 4, "mixed_h256": 4, "div33_h8": 33, "floor1_h8": 1, "empty_h8": 1, "flip_one_h8": 4,
                   "flip_div33_h8": 33, "flip_pair_h256": 4}
NEXT_DRAWS = 4                 # torch.rand values taken after the call: the generator's state


def make_targets(sizes, seed, device="cpu", dtype=torch.float32):
    """The reference's target dict: ``labels`` a list of per-frame Python lists, ``keypoints`` a list of [n, W] tensors in
    [0, 1] with exact 0, exact 1 and values inside inverse_sigmoid's eps planted."""
    rs = np.random.RandomState(seed)
    labels, keys = [], []
    for n in sizes:
        labels.append([int(x) for x in rs.randint(0, NUM_CLASSES, size=n)])
        k = rs.uniform(0.02, 0.98, size=(n, W)).astype(np.float32)
        if n:
            k[0, 0], k[0, 1], k[0, 2], k[0, 3] = 0.0, 1.0, 3e-6, 1.0 - 3e-6
        keys.append(torch.from_numpy(k).to(device=device, dtype=dtype))
    return {"labels": labels, "keypoints": keys}


def targets(case, device="cpu", dtype=torch.float32):
    c = CASES[case]
    return make_targets(c["sizes"], c["seed"], device, dtype)


def make_label_enc(hidden, seed, device="cpu", dtype=torch.float32):
    enc = nn.Embedding(NUM_CLASSES + 1, hidden)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        enc.weight.copy_(torch.randn(enc.weight.shape, generator=g))
    return enc.to(device=device, dtype=dtype)


def label_enc(case, device="cpu", dtype=torch.float32):
    return make_label_enc(CASES[case]["hidden"], CASES[case]["seed"] + 1, device, dtype)


def dn_args(case, tg):
    c = CASES[case]
    return (tg, c["dn"], c["ratio"], c["box"])


def output_weights(seed, shapes, device="cpu", dtype=torch.float32):
    """The seeded weighting of the two outputs (the loss is the sum of the weighted outputs)."""
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(device=device, dtype=dtype) for s in shapes]


def loss_of(label, key, seed):
    wl, wk = output_weights(seed, [tuple(label.shape), tuple(key.shape)], label.device, label.dtype)
    return (label * wl).sum() + (key * wk.to(key.dtype)).sum()


def run(fn, case, device="cpu", dtype=torch.float32, **kwargs):
    """One call of ``fn`` (a prepare_for_cdn) on the case and the backward of the weighted sum:
    (label, key, mask, dn_meta, grad_weight or None, the next NEXT_DRAWS values of the CPU generator or None)."""
    c = CASES[case]
    enc = label_enc(case, device, dtype)
    tg = targets(case, device, dtype)
    if "torch_seed" in c:
        torch.manual_seed(c["torch_seed"])
    label, key, mask, meta = fn(dn_args(case, tg), True, QUERIES, NUM_CLASSES, c["hidden"], enc, **kwargs)
    nxt = torch.rand(NEXT_DRAWS) if "torch_seed" in c else None
    grad = None
    if label.requires_grad:
        loss_of(label, key, c["seed"] + 2).backward()
        grad = enc.weight.grad
    return label, key, mask, meta, grad, nxt


def ulp(x):
    import math
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 0.0


def hold(what, ours, t32, r64, ratios=None):
    """The project's accuracy rule: the largest error of `ours` against the fp64 evaluation is at most 4 times that of the torch
    fp32 composition, which counts as at least one fp32 ulp of the tensor's largest value.  Prints the figures, returns the ratio."""
    r64 = r64.double()
    e_ours = float((ours.double() - r64).abs().max()) if r64.numel() else 0.0
    e_torch = float((t32.double() - r64).abs().max()) if r64.numel() else 0.0
    top = float(r64.abs().max()) if r64.numel() else 0.0
    yard = max(e_torch, ulp(top))
    ratio = e_ours / yard if yard else (float("inf") if e_ours else 0.0)
    if ratios is not None:
        ratios[what] = max(ratios.get(what, 0.0), ratio)
    print("%-44s ours %.3e torch %.3e yardstick %.3e ratio %.2f" % (what, e_ours, e_torch, yard, ratio))
    assert e_ours <= 4.0 * yard, (what, e_ours, e_torch, yard)
    return ratio
