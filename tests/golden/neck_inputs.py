"""Seeded inputs of tests/test_neck*.py: per-level conv inputs, Conv2d / GroupNorm tensors, uniforms and loss weights of the
input-projection neck, and the runner that returns outputs and all five gradient families.  Values are drawn in fp32 and
widened, so the fp32 and fp64 evaluations start from the same numbers; the uniforms stay fp32 in both, so that both take the
same mask (float32(0.3) widened would pass a comparison with the double 0.3)."""
import numpy as np
import torch

GROUPS = 32
EPS = 1e-5

# name: (N, hidden, [(C_in, H, W, kernel)], masked, seed); kernel 1 = 1x1, kernel 3 = 3x3 stride 2 padding 1
CASES = {
    # five levels in one call: 28x28 (float4 path), 7x7 and 5x3 (odd sizes), the 3x3 stride-2 level (7x7 -> 4x4), 1x1
    "mixed": (3, 64, [(24, 28, 28, 1), (40, 7, 7, 1), (40, 5, 3, 1), (40, 7, 7, 3), (24, 1, 1, 1)], True, 11),
    # hidden 256 (8 channels per group, two channels per wavefront), one frame, no mask
    "hidden256": (1, 256, [(24, 28, 28, 1), (40, 7, 7, 1), (40, 7, 7, 3)], False, 12),
    "single": (3, 64, [(40, 5, 3, 1)], True, 13),
    # the conv input is a permuted view of an NHWC tensor
    "permuted": (1, 64, [(24, 4, 4, 1), (40, 7, 7, 1)], True, 14),
    # conv bias 1e3 under unit noise: E[x^2] - mean^2 would lose every digit of the variance
    "offset": (1, 256, [(24, 28, 28, 1), (40, 7, 7, 1)], True, 15),
    # group 0 of every level is constant: variance 0, rstd = eps^-1/2
    "constant": (3, 64, [(24, 4, 4, 1), (40, 7, 7, 1)], True, 16),
    # groups of 2 x 4160 and 2 x 4161 floats: past the 8192 floats the forward stages in LDS (float4 and scalar forms)
    "large": (1, 64, [(24, 65, 64, 1), (24, 57, 73, 1)], True, 17),
}


def conv_geometry(kernel):
    return ((2, 2), (1, 1)) if kernel == 3 else ((1, 1), (0, 0))


def build(name, dtype=torch.float32, device="cpu"):
    """(xs, convs, norms, uniforms, weights): convs as (weight, bias, stride, padding, dilation, groups), norms as
    (num_groups, gamma, beta, eps); uniforms None for an unmasked case; weights multiply the outputs in the loss."""
    N, hidden, levels, masked, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    xs, convs, norms, uniforms, weights = [], [], [], [], []
    for cin, H, W, k in levels:
        if name == "permuted":
            x = torch.randn(N, H, W, cin, generator=g).permute(0, 3, 1, 2)
        else:
            x = torch.randn(N, cin, H, W, generator=g)
        w = torch.randn(hidden, cin, k, k, generator=g) / float(np.sqrt(cin * k * k))
        b = torch.randn(hidden, generator=g) * 0.5
        gamma = 1 + 0.3 * torch.randn(hidden, generator=g)
        beta = 0.3 * torch.randn(hidden, generator=g)
        if name == "offset":
            b += 1e3
        if name == "constant":
            cpg = hidden // GROUPS
            w[:cpg] = 0
            b[:cpg] = 0.7
        stride, padding = conv_geometry(k)
        Ho, Wo = (H + 2 * padding[0] - k) // stride[0] + 1, (W + 2 * padding[1] - k) // stride[1] + 1
        u = torch.rand(N, hidden, Ho, Wo, generator=g)
        edge = torch.tensor(np.array([0.3, np.nextafter(np.float32(0.3), np.float32(0)), np.nextafter(np.float32(0.3), np.float32(1)),
                                      0.0, 1 - 2.0 ** -24, 1 - 2.0 ** -23, 0.99999], dtype=np.float32))
        u.view(-1)[:min(7, u.numel())] = edge[:u.numel()]
        if u.numel() > 16:
            u.view(-1)[-7:] = edge
        weights.append(torch.randn(N, hidden, Ho, Wo, generator=g).to(device, dtype))
        xs.append(x.to(device, dtype))
        convs.append((w.to(device, dtype), b.to(device, dtype), stride, padding, (1, 1), 1))
        norms.append((GROUPS, gamma.to(device, dtype), beta.to(device, dtype), EPS))
        uniforms.append(u.to(device))           # always fp32: the mask is the fp32 comparison u > 0.3f in every evaluation
    return xs, convs, norms, (uniforms if masked else None), weights


NAMES = ("out", "grad_x", "grad_weight", "grad_bias", "grad_gamma", "grad_beta")


def run(fn, xs, convs, norms, uniforms, weights):
    """{family: [per-level tensor]} of fn's outputs and of the gradients of sum_l (out_l * weights_l).sum()."""
    L = len(xs)
    xs = [x.detach().requires_grad_(True) for x in xs]
    convs = [(c[0].detach().requires_grad_(True), c[1].detach().requires_grad_(True)) + tuple(c[2:]) for c in convs]
    norms = [(n[0], n[1].detach().requires_grad_(True), n[2].detach().requires_grad_(True), n[3]) for n in norms]
    outs = fn(xs, convs, norms, uniforms)
    loss = sum((o * w).sum() for o, w in zip(outs, weights))
    leaves = xs + [c[0] for c in convs] + [c[1] for c in convs] + [n[1] for n in norms] + [n[2] for n in norms]
    grads = torch.autograd.grad(loss, leaves)
    res = {"out": [o.detach() for o in outs]}
    for i, name in enumerate(NAMES[1:]):
        res[name] = list(grads[i * L:(i + 1) * L])
    return res
