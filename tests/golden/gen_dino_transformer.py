#!/usr/bin/env python3
"""DINO DeformableTransformer fixture, made by RUNNING THE REFERENCE'S DeformableTransformer, TransformerEncoder,
DeformableTransformerEncoderLayer, TransformerDecoder and DeformableTransformerDecoderLayer
(models/dino/deformable_transformer.py:25-1065) with its gen_encoder_output_proposals, MLP and gen_sineembed_for_position
(models/dino/utils.py) and inverse_sigmoid (util/misc.py) unchanged, on the seeded parameters and inputs of
dino_transformer_inputs.py.  The decoder is the reference's own, not the package's.

  dino_transformer.npz   <case>/hs<i>, ref<i>, hs_enc, ref_enc_obj, ref_enc_hand, init_box_proposal_unsig   the five outputs
                         <case>/topk                the selected rows [N, Q]
                         <case>/grad_src<l>         gradients of the seeded weighted sum w.r.t. every level of srcs
                         <case>/param_names, pgrad_none, pgrad_val, pgrad_sum, pgrad_abssum   seeded samples and fp64 sums of
                                                    every parameter gradient, in sorted name order
                         <case>/state_keys          the state_dict keys of the bare construction, in order
                         <case>/init_sums           per-tensor fp64 sums of the state_dict constructed under
                                                    torch.manual_seed(INIT_SEED)
                         <case>/row_margin, class_margin, dec_margin, codes, proposals_err    the fixture's condition

As gen_dino_decoder.py does, the definitions are taken out of their files with `ast` and executed unchanged (importing the
files needs the reference's CUDA extension).  The package's MSDeformAttn serves the sampling, on the oracle's pure-PyTorch
core.  CPU, fp32, eval mode.

The generator asserts the fixture's condition: among each frame's top Q + 1 row maxima every two neighbours differ by at least
MIN_MARGIN; each selected row's top two class logits differ by at least MIN_MARGIN (in the decoder's layers too); all three
codes occur; and the reference's gen_encoder_output_proposals equals two_stage_func.proposals_composition bit for bit on these
inputs.  No selected row is a padded one: the padded rows of a frame are zeroed before ``enc_output`` and so share one set of
class logits exactly — with more than one of them (any border) a selected padded row would tie with its neighbours, which the
first condition excludes.  tests/test_dino_select_gpu.py covers the +inf rows instead.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dino_transformer.py
"""
import ast
import copy
import math
import os
import random
import sys
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dino_transformer_inputs as TI  # noqa: E402
import uvhand_amd.modules.ms_deform_attn as msda_mod  # noqa: E402
from uvhand_amd.functions import two_stage_func as TS  # noqa: E402
from uvhand_amd.modules import MSDeformAttn  # noqa: E402


class _CpuCore:
    """MSDeformAttnFunction's interface on the oracle's pure-PyTorch core (the library's op refuses CPU tensors)."""

    @staticmethod
    def apply(value, shapes, lsi, loc, attn, im2col_step):
        from oracle.torch_fallback import msda_torch_fallback
        return msda_torch_fallback(value, shapes, loc, attn)


msda_mod.MSDeformAttnFunction = _CpuCore


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _reference():
    (inverse_sigmoid,) = _extract(REF + "/util/misc.py", ["inverse_sigmoid"], {"torch": torch})
    uns = {"torch": torch, "nn": nn, "F": F, "math": math, "Tensor": Tensor}
    MLP, act, sine, props = _extract(REF + "/models/dino/utils.py",
                                     ["MLP", "_get_activation_fn", "gen_sineembed_for_position", "gen_encoder_output_proposals"], uns)
    ns = {"torch": torch, "nn": nn, "Tensor": Tensor, "Optional": Optional, "math": math, "random": random, "copy": copy,
          "inverse_sigmoid": inverse_sigmoid, "MLP": MLP, "_get_activation_fn": act, "gen_sineembed_for_position": sine,
          "gen_encoder_output_proposals": props, "MSDeformAttn": MSDeformAttn}
    (tr,) = _extract(REF + "/models/dino/deformable_transformer.py",
                     ["DeformableTransformer", "TransformerEncoder", "TransformerDecoder", "DeformableTransformerEncoderLayer",
                      "DeformableTransformerDecoderLayer", "_get_clones"], ns)[:1]
    return tr, MLP, props


def _margins(logits, Q):
    """(smallest gap between neighbours of each frame's top Q + 1 row maxima, smallest top-two class gap of the selected rows,
    the codes of the selected rows)."""
    row_max = logits.max(-1)[0]
    top = torch.sort(row_max, dim=1, descending=True)[0][:, :Q + 1]
    row_margin = float((top[:, :-1] - top[:, 1:]).min())
    idx = torch.sort(row_max, dim=1, descending=True)[1][:, :Q]
    sel = torch.gather(logits, 1, idx.unsqueeze(-1).expand(-1, -1, logits.shape[-1]))
    two = torch.topk(sel, 2, dim=-1)[0]
    cl = sel.argmax(-1)
    hand = (cl == 12) | (cl == 13)
    return row_margin, float((two[..., 0] - two[..., 1]).min()), 2 * hand.long() + (~hand & (cl != 0)).long(), idx


def run_case(case, tr_cls, mlp_cls, ref_props):
    """The fixture's entries of one case; AssertionError where the seeded parameters miss the fixture's condition."""
    out = {}
    if True:
        torch.manual_seed(TI.INIT_SEED)
        bare = TI.construct(tr_cls, case)
        out[case + "/state_keys"] = np.array(list(bare.state_dict().keys()))
        out[case + "/init_sums"] = np.asarray([float(v.double().sum()) for v in bare.state_dict().values()], dtype=np.float64)

        tr = TI.build(tr_cls, mlp_cls, case)
        enc_logits, dec_logits = [], []
        hooks = [tr.enc_out_class_embed.register_forward_hook(lambda mod, inp, o: enc_logits.append(o.detach().double()))]
        hooks += [m.register_forward_hook(lambda mod, inp, o: dec_logits.append(o.detach().double())) for m in tr.decoder.class_embed]
        prep = TI.prepare(case)
        outs = TI.step(tr, prep)
        for h in hooks:
            h.remove()

        Q = TI.CFG["queries"]
        row_margin, class_margin, codes, idx = _margins(enc_logits[0], Q)
        assert row_margin >= TI.MIN_MARGIN, "%s: neighbouring row maxima %.3e apart; change the seed" % (case, row_margin)
        assert class_margin >= TI.MIN_MARGIN, "%s: class margin %.3e; change the seed" % (case, class_margin)
        assert set(codes.flatten().tolist()) == {0, 1, 2}, "%s: codes %s; change the seed" % (case, sorted(set(codes.flatten().tolist())))
        dec_margin = []
        for c in dec_logits:
            two = torch.topk(c, 2, dim=-1)[0]
            dec_margin.append(float((two[..., 0] - two[..., 1]).min()))
            assert dec_margin[-1] >= TI.MIN_MARGIN, "%s: decoder class margin %.3e; change the seed" % (case, dec_margin[-1])
        # the reference's selection, read back through its init_box_proposal_unsig: the rows are the sort's
        topk = idx.numpy()
        dead = torch.from_numpy(np.concatenate([m.reshape(m.shape[0], -1) for m in TI.inputs(case)["masks"]], 1))
        assert not torch.gather(dead, 1, idx).any(), "%s: a padded row is selected and ties with the other padded rows" % case

        # DINO's gen_encoder_output_proposals against the composition the package's kernel restates (note learnedxy.sigmoid())
        mem = torch.randn(TI.CFG["N"], TI.n_rows(), TI.CFG["d"], generator=torch.Generator().manual_seed(3))
        wh = tr.two_stage_wh_embedding.weight[0].detach() if TI.CASES[case]["learn_wh"] else None
        shapes = torch.as_tensor(TI.CFG["shapes"], dtype=torch.long)
        m_ref, p_ref = ref_props(mem, dead, shapes, wh)
        m_own, p_own = TS.proposals_composition(mem, dead, TI.CFG["shapes"], wh)
        assert torch.equal(m_ref, m_own) and torch.equal(p_ref, p_own), "%s: the DINO proposals differ from the composition" % case
        out[case + "/proposals_err"] = np.asarray(0.0)

        out[case + "/row_margin"] = np.asarray(row_margin)
        out[case + "/class_margin"] = np.asarray(class_margin)
        out[case + "/dec_margin"] = np.asarray(dec_margin)
        out[case + "/codes"] = codes.numpy().astype(np.uint8)
        out[case + "/topk"] = topk
        for lab, o in zip(TI.labels(), outs):
            out["%s/%s" % (case, lab)] = o.detach().numpy()
        # the selected rows are what the reference gathered: hs_enc is output_memory[topk]
        for lvl, s in enumerate(prep["srcs"]):
            out["%s/grad_src%d" % (case, lvl)] = s.grad.numpy()
        params = sorted(tr.named_parameters(), key=lambda kv: kv[0])
        out[case + "/param_names"] = np.array([k for k, _ in params])
        none, val, sums, abss = [], np.zeros((len(params), TI.PGRAD_SAMPLES), dtype=np.float32), [], []
        for j, (k, p) in enumerate(params):
            none.append(p.grad is None)
            g = (p.grad if p.grad is not None else torch.zeros_like(p)).flatten().double().numpy()
            ix = TI.pgrad_index(case, j, g.size)
            val[j, :ix.size] = g[ix]
            sums.append(g.sum())
            abss.append(np.abs(g).sum())
        out[case + "/pgrad_none"] = np.asarray(none)
        out[case + "/pgrad_val"] = val
        out[case + "/pgrad_sum"] = np.asarray(sums, dtype=np.float64)
        out[case + "/pgrad_abssum"] = np.asarray(abss, dtype=np.float64)
        print(case, "row margin %.3e class margin %.3e decoder margins %s codes %s" % (row_margin, class_margin, dec_margin,
                                                                                      codes.tolist()))
        print(case, "None gradients:", [k for (k, _), n in zip(params, none) if n])
    return out


def main():
    tr_cls, mlp_cls, ref_props = _reference()
    out = {}
    for case in TI.CASES:
        out.update(run_case(case, tr_cls, mlp_cls, ref_props))
    np.savez_compressed(os.path.join(HERE, "dino_transformer.npz"), **out)


if __name__ == "__main__":
    main()
