"""Drop-in DeformableDETR models (uvhand_amd/modules/detr.py) on the CPU, where the heads run the torch restatement:
against fixtures made by running the reference's DeformableDETR (tests/golden/gen_golden_r10.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

sys.path.insert(0, GOLDEN)
import detr_inputs as DI  # noqa: E402
from uvhand_amd.functions.heads_func import ARCTIC, ASSEMBLY, detr_heads, detr_heads_reference  # noqa: E402
from uvhand_amd.modules import ArcticDeformableDETR, AssemblyDeformableDETR  # noqa: E402
from uvhand_amd.modules.detr import NestedTensor  # noqa: E402

CASES = list(DI.CASES)


def _cls(name):
    return ArcticDeformableDETR if DI.CASES[name][0] == "arctic" else AssemblyDeformableDETR


def _fixture(name):
    return load_golden("detr_" + name)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_bit_identical_at_seed(name):
    z = _fixture(name)
    model = DI.build(name, _cls(name), NestedTensor)
    sd = model.state_dict()
    assert sorted("init/" + k for k in sd) == sorted(k for k in z if k.startswith("init/"))
    for k, v in sd.items():
        assert DI.digest(v) == str(z["init/" + k]), k


@pytest.mark.parametrize("name", CASES)
def test_reference_state_dict_loads_strict(name):
    z = _fixture(name)
    ref_sd = {k[len("shape/"):]: torch.full(tuple(int(s) for s in v), 0.25) for k, v in z.items() if k.startswith("shape/")}
    model = DI.build(name, _cls(name), NestedTensor)
    model.load_state_dict(ref_sd, strict=True)
    assert all(bool((p == 0.25).all()) for p in model.parameters())


@pytest.mark.parametrize("name", CASES)
def test_outputs_and_gradients_match_reference(name):
    z = _fixture(name)
    seed = DI.CASES[name][-1]
    model = DI.build(name, _cls(name), NestedTensor)
    DI.perturb(model, seed)
    model.train()
    out = model(DI.samples(name, NestedTensor))
    paths = [p for p, _ in DI.flatten_outputs(out)]
    assert sorted("out" + p for p in paths) == sorted(k for k in z if k.startswith("out/"))
    for path, t in DI.flatten_outputs(out):
        ref = z["out" + path]
        assert tuple(t.shape) == ref.shape and t.dtype == torch.float32, path
        np.testing.assert_allclose(t.detach().numpy(), ref, rtol=1e-5, atol=1e-6, err_msg=path)
    DI.weighted_sum(out, seed + 7).backward()
    assert rel_err(model.transformer.hs.grad.numpy(), z["grad/hs"]) < 1e-5
    got = {k: p.grad for k, p in model.named_parameters()}
    for k, g in got.items():
        if "grad/" + k in z:
            assert rel_err(g.numpy(), z["grad/" + k]) < 1e-5, k
        elif "gradsum0/" + k in z:
            assert rel_err(g.sum(0).numpy(), z["gradsum0/" + k]) < 1e-5, k
            assert rel_err(g.sum(1).numpy(), z["gradsum1/" + k]) < 1e-5, k
        else:
            assert g is None, k


@pytest.mark.parametrize("name", CASES)
def test_decoder_attributes_as_reference(name):
    model_kind, two_stage, refine = DI.CASES[name][:3]
    model = DI.build(name, _cls(name), NestedTensor)
    dec = model.transformer.decoder
    if model_kind == "arctic":
        if refine:
            assert dec.cls_embed is model.cls_embed and dec.key_embed is model.key_embed
            assert dec.obj_key_embed is model.obj_key_embed
            assert len(model.key_embed) == DI.CASES[name][3] + 1
        else:
            assert not hasattr(dec, "cls_embed") and not hasattr(model, "key_embed")
        for name_ in ("mano_pose_embed", "mano_beta_embed", "hand_cam", "obj_cam", "obj_rot", "obj_rad"):
            mods = getattr(model, name_)
            assert all(m is mods[0] for m in mods)
    else:
        if refine:
            assert dec.keypoint_embed is model.keypoint_embed and dec.obj_keypoint_embed is model.obj_keypoint_embed
            assert model.keypoint_embed[0] is not model.keypoint_embed[1]
        else:
            assert dec.keypoint_embed is None and dec.obj_keypoint_embed is None
            assert all(m is model.keypoint_embed[0] for m in model.keypoint_embed)
        assert (getattr(dec, "cls_embed", None) is model.cls_embed) == (two_stage or refine)


def test_output_structure():
    model = DI.build("arctic_one_stage", ArcticDeformableDETR, NestedTensor)
    out = model(DI.samples("arctic_one_stage", NestedTensor))
    assert set(out) == {"pred_logits", "pred_hand_key", "pred_obj_key", "pred_mano_params", "pred_obj_params", "pred_cams",
                        "aux_outputs"}
    assert out["pred_hand_key"].shape == () and float(out["pred_hand_key"]) == 0.0      # torch.zeros(levels)[-1]
    assert len(out["aux_outputs"]) == 1 and len(out["pred_mano_params"]) == 2
    assert out["pred_mano_params"][0].shape[-1] == 48 and out["pred_obj_params"][0].shape[-1] == 1
    model = DI.build("arctic_refine", ArcticDeformableDETR, NestedTensor)
    out = model(DI.samples("arctic_refine", NestedTensor))
    assert set(out["interm_outputs"]) == {"pred_logits", "pred_hand_key", "pred_obj_key"}
    assert len(out["aux_outputs"]) == 2
    model = DI.build("assembly_2d", AssemblyDeformableDETR, NestedTensor)
    out = model(DI.samples("assembly_2d", NestedTensor))
    assert set(out) == {"pred_logits", "pred_keypoints", "aux_outputs", "enc_outputs"}
    assert out["pred_keypoints"].shape[-1] == 63


@pytest.mark.parametrize("name", CASES)
def test_restatement_is_what_the_cpu_runs(name):
    model_kind = DI.CASES[name][0]
    model = DI.build(name, _cls(name), NestedTensor)
    DI.perturb(model, 5)
    tr = model.transformer
    if model_kind == "arctic":
        mlps = [model.key_embed, model.obj_key_embed] if model.two_stage else []
        shared = [model.mano_pose_embed[0], model.mano_beta_embed[0], model.hand_cam[0], model.obj_cam[0],
                  model.obj_rot[0], model.obj_rad[0]]
        args = (ARCTIC, tr.hs, tr.init_reference, tr.inter_references, model.cls_embed, mlps, shared)
    else:
        args = (ASSEMBLY, tr.hs, tr.init_reference, tr.inter_references, model.cls_embed, [model.keypoint_embed])
    a = detr_heads(*args)
    b = detr_heads_reference(*args)
    for x, y in zip([a[0]] + a[1] + a[2], [b[0]] + b[1] + b[2]):
        assert torch.equal(x, y)


def test_inverse_sigmoid_clamps_negative_references():
    from uvhand_amd.functions.heads_func import inverse_sigmoid
    r = inverse_sigmoid(torch.tensor([-0.5, 0.0, 3e-6, 1.0]))
    assert float(r[0]) == float(r[1]) == float(torch.log(torch.tensor(1e-5)))
    assert abs(float(r[2]) - float(r[0])) < 1e-4 and abs(float(r[3]) + float(r[0])) < 1e-5


@pytest.mark.skipif(os.environ.get("MSDA_HEADS_FUSED") == "0", reason="knob set by the caller")
def test_knob_default_on():
    from uvhand_amd.functions import heads_func
    assert heads_func._fused_enabled()
