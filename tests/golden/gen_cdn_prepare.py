#!/usr/bin/env python3
"""Denoising-query fixture, made by RUNNING THE REFERENCE'S prepare_for_cdn (models/dino/dn_components.py:20-150) and
inverse_sigmoid (util/misc.py:614-618) unchanged on the seeded targets and embeddings of cdn_prepare_inputs.py:

  cdn_prepare.npz   <case>/label        input_query_label [B, pad, hidden]
                    <case>/key          input_query_key [B, pad, 42]
                    <case>/mask         attn_mask [pad + queries, pad + queries] bool
                    <case>/meta         (pad_size, num_dn_group)
                    <case>/grad_weight  gradient of sum(weight * output) over both outputs w.r.t. label_enc.weight (cases with
                                        at least one target)
                    <case>/next         the next values of torch's CPU generator after the call (cases that draw)

As gen_dino_decoder.py does, the two definitions are taken out of their files with `ast` and executed unchanged.  They run on
the CPU: in this process only, Tensor.cuda is the identity and .to('cuda') goes to the CPU.  Cases with label_noise_ratio 0
are deterministic; the others run under a fixed manual_seed and serve the CPU composition route, which draws from the same
generator in the same order.  The generator asserts the group count every case was chosen for.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_cdn_prepare.py
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import cdn_prepare_inputs as CI  # noqa: E402


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _cpu_only():
    """This process has no GPU: .cuda() is the identity and 'cuda' means the CPU."""
    real_to = torch.Tensor.to

    def to(self, *args, **kwargs):
        args = tuple("cpu" if a == "cuda" else a for a in args)
        if kwargs.get("device") == "cuda":
            kwargs["device"] = "cpu"
        return real_to(self, *args, **kwargs)

    torch.Tensor.to = to
    torch.Tensor.cuda = lambda self, *a, **k: self


def main():
    _cpu_only()
    (inverse_sigmoid,) = _extract(REF + "/util/misc.py", ["inverse_sigmoid"], {"torch": torch})
    (prepare_for_cdn,) = _extract(REF + "/models/dino/dn_components.py", ["prepare_for_cdn"],
                                  {"torch": torch, "inverse_sigmoid": inverse_sigmoid})
    out = {}
    for case, c in CI.CASES.items():
        label, key, mask, meta, grad, nxt = CI.run(prepare_for_cdn, case)
        assert meta["num_dn_group"] == CI.EXPECTED_GROUPS[case], (case, meta)
        assert tuple(label.shape) == (len(c["sizes"]), meta["pad_size"], c["hidden"])
        out[case + "/label"] = label.detach().numpy()
        out[case + "/key"] = key.detach().numpy()
        out[case + "/mask"] = mask.numpy()
        out[case + "/meta"] = np.asarray([meta["pad_size"], meta["num_dn_group"]], dtype=np.int64)
        if grad is not None:
            out[case + "/grad_weight"] = grad.numpy()
        if nxt is not None:
            out[case + "/next"] = nxt.numpy()
        print(case, dict(meta), "grad" if grad is not None else "no grad")
    path = os.path.join(HERE, "cdn_prepare.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
