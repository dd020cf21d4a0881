#!/usr/bin/env python3
"""ARCTIC evaluation fixtures, made by RUNNING THE REFERENCE'S OWN FUNCTIONS unchanged on the seeded inputs of
arctic_eval_inputs.py: arctic_tools/process.py get_arctic_item, post_process_arctic_output, make_output, prepare_data,
measure_error; MANOHead.forward (src/nets/hand_heads/mano_head.py), ArtiHead.forward (src/nets/obj_heads/obj_head.py);
eval_degree, eval_mpjpe_ra, eval_mrrpe, eval_v2v_success, eval_contact_deviation (src/utils/eval_modules.py); common/metrics.py;
contact_deviation (src/utils/loss_modules.py); unpad_vtensor, nanmean (common/torch_utils.py); common/rot.py; common/xdict.py
over common/thing.py; ObjectTensors (common/object_tensors.py) on the synthetic arrays.

  arctic_eval.npz  <case>/mo_keys             make_output's keys in its order;  <case>/mo/mano.pose.{r,l} its rotation matrices
                   <case>/keys                prepare_data's keys in its order
                   <case>/data/<key>          prepare_data(flag='eval') tensors: all of them for case `partial`, those of at
                                              most 3000 elements for the others (file size); never nn_dist_* / nn_idx_*
                   <case>/metric/<key>        measure_error's six rows (fp64 copies of the reference's arrays)
                   <case>/step/<key>          engine.py:784-794's per-key mean of the step (NaN: key dropped for the step)
                   avg/<key>                  MetricLogger's global_avg over arctic_eval_inputs.SEQUENCE

As gen_golden_r14.py does, the definitions are taken out of their files with `ast` and executed unchanged (importing them
needs pytorch3d, smplx, trimesh and the ARCTIC meta files).  Stand-ins, none of them arithmetic of the evaluation:
  * knn_points CANNOT RUN HERE (pytorch3d is absent): get_NN's call is served by the package's nn_reference in fp32, so
    `nn_dist_*` / `nn_idx_*` are NOT reference output and are left out of the file; the nearest-neighbour yardstick is fp64 brute force in the tests.
  * build_mano_aa returns the package's MANO on mano_inputs.py's models (CPU: its torch restatement, pinned to manopth by
    test_mano.py); ObjectTensors() returns the reference class built without __init__ on the synthetic arrays.
  * process.py's matrix_to_axis_angle / axis_angle_to_matrix are pytorch3d's: common/rot.py's copies of them serve.
  * engine.py's per-key loop sits inside test_pose and is restated here line by line.
The generator asserts what the tests rely on: every synthetic object has bottom-part rows below its v_len, and (in fp64) no
vertex lies within 1e-4 relative of its success threshold.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_arctic_eval.py
"""
import ast
import copy
import math
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("UVHAND_REFERENCE", "/root/reference") + "/arctic_tools"

sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import arctic_eval_inputs as EI  # noqa: E402
import small_loss_inputs as SI  # noqa: E402
from uvhand_amd.arctic_eval import nn_reference  # noqa: E402

METRICS = ["aae", "mpjpe.ra", "mrrpe", "success_rate", "cdev", "mdev", "acc_err_pose"]
SMALL = 3000


def _extract(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def _reference():
    S = types.SimpleNamespace
    rot_ns = {"torch": torch, "F": F}
    rot_names = ["_sqrt_positive_part", "quaternion_to_axis_angle", "quaternion_to_matrix", "matrix_to_quaternion",
                 "matrix_to_axis_angle", "axis_angle_to_quaternion", "quaternion_raw_multiply", "quaternion_invert", "quaternion_apply"]
    r = dict(zip(rot_names, _extract(REF + "/common/rot.py", rot_names, rot_ns)))
    thing_names = ["thing2dev", "thing2np", "thing2torch", "thing2list", "detach_thing"]
    thing = S(**dict(zip(thing_names, _extract(REF + "/common/thing.py", thing_names, {"torch": torch, "np": np}))))
    (xdict,) = _extract(REF + "/common/xdict.py", ["xdict"], {"torch": torch, "np": np, "thing": thing})
    nanmean, unpad_vtensor = _extract(REF + "/common/torch_utils.py", ["nanmean", "unpad_vtensor"], {"torch": torch})
    torch_utils = S(nanmean=nanmean, unpad_vtensor=unpad_vtensor)
    (wp2p,) = _extract(REF + "/common/camera.py", ["weak_perspective_to_perspective_torch"], {"torch": torch})
    to_xy, project2d = _extract(REF + "/common/transforms.py", ["to_xy_batch", "project2d_batch"], {"torch": torch})
    normalize_kp2d, unormalize_kp2d = _extract(REF + "/common/data_utils.py", ["normalize_kp2d", "unormalize_kp2d"], {"torch": torch})
    (prefix_dict,) = _extract(REF + "/common/ld_utils.py", ["prefix_dict"], {})
    m_names = ["compute_v2v_dist_no_reduce", "compute_joint3d_error", "compute_mrrpe", "compute_arti_deg_error"]
    metrics = S(**dict(zip(m_names, _extract(REF + "/common/metrics.py", m_names, {"torch": torch, "np": np, "math": math}))))
    (contact_deviation,) = _extract(REF + "/src/utils/loss_modules.py", ["contact_deviation"], {"torch": torch, "torch_utils": torch_utils})
    e_names = ["eval_degree", "eval_mpjpe_ra", "eval_mrrpe", "eval_v2v_success", "eval_contact_deviation"]
    ev = _extract(REF + "/src/utils/eval_modules.py", e_names,
                  {"torch": torch, "np": np, "copy": copy, "metrics": metrics, "unpad_vtensor": unpad_vtensor,
                   "torch_utils": torch_utils, "xdict": xdict, "contact_deviation": contact_deviation})
    eval_fn_dict = dict(zip(["aae", "mpjpe.ra", "mrrpe", "success_rate", "cdev"], ev))
    ot_ns = {"torch": torch, "np": np, "nn": nn, "xdict": xdict, "thing": thing, "axis_angle_to_quaternion": r["axis_angle_to_quaternion"],
             "quaternion_apply": r["quaternion_apply"]}
    (ObjectTensors,) = _extract(REF + "/common/object_tensors.py", ["ObjectTensors"], ot_ns)

    def object_tensors():
        obj = ObjectTensors.__new__(ObjectTensors)
        nn.Module.__init__(obj)
        obj.obj_tensors = SI.obj_arrays()
        obj.dev = None
        return obj
    manos = EI.mano_models()
    head_ns = {"nn": nn, "camera": S(weak_perspective_to_perspective_torch=wp2p), "tf": S(project2d_batch=project2d),
               "data_utils": S(normalize_kp2d=normalize_kp2d, unormalize_kp2d=unormalize_kp2d), "rot": S(**r), "xdict": xdict,
               "build_mano_aa": lambda is_rhand: manos["mano_r" if is_rhand else "mano_l"], "ObjectTensors": object_tensors}
    (MANOHead,) = _extract(REF + "/src/nets/hand_heads/mano_head.py", ["MANOHead"], head_ns)
    (ArtiHead,) = _extract(REF + "/src/nets/obj_heads/obj_head.py", ["ArtiHead"], head_ns)
    p_ns = {"torch": torch, "xdict": xdict, "MANOHead": MANOHead, "ArtiHead": ArtiHead, "ld_utils": S(prefix_dict=prefix_dict),
            "data_utils": head_ns["data_utils"], "matrix_to_axis_angle": r["matrix_to_axis_angle"],
            "axis_angle_to_matrix": lambda a: r["quaternion_to_matrix"](r["axis_angle_to_quaternion"](a)),
            "get_NN": lambda s, t: nn_reference(s.float(), t.float()), "eval_fn_dict": eval_fn_dict}
    names = ["get_arctic_item", "post_process_arctic_output", "make_output", "prepare_data", "measure_error"]
    return dict(zip(names, _extract(REF + "/process.py", names, p_ns))), xdict


def _check_inputs(targets, meta):
    for ids, n in zip(meta["part_ids"], targets["object.v_len"]):
        assert (ids[:int(n)] == 2).any(), "an object without bottom-part rows below v_len"
        assert not (ids[int(n):] == 2).any()


def _check_thresholds(data):
    """fp64: no vertex within 1e-4 relative of its success threshold."""
    for b in range(len(data["targets.is_valid"])):
        n = int(data["targets.object.v_len"][b])
        g, p = data["targets.object.v.cam"][b, :n].double(), data["pred.object.v.cam"][b, :n].double()
        bot = data["meta_info.part_ids"][b, :n] == 2
        d = ((g - g[bot].mean(0)) - (p - p[bot].mean(0))).norm(dim=1)
        thr = float(data["meta_info.diameter"][b]) * 0.05
        assert ((d - thr).abs() > 1e-4 * thr).all(), "a vertex on its success threshold"


def main():
    warnings.filterwarnings("ignore")
    fn, xdict = _reference()
    args = EI.args()
    out, total, count = {}, {}, {}
    steps = {}
    for case in EI.CASES:
        outputs, targets, meta = EI.case_inputs(case)
        _check_inputs(targets, meta)
        with torch.no_grad():
            mo = fn["post_process_arctic_output"](outputs, xdict(meta), args, EI.CFG)
            data = fn["prepare_data"](args, outputs, targets, meta, EI.CFG, flag='eval')
            _check_thresholds(data)
            stats = fn["measure_error"](data, METRICS)
        out[case + "/mo_keys"] = np.array(list(mo.keys()))
        out[case + "/mo/mano.pose.r"], out[case + "/mo/mano.pose.l"] = mo["mano.pose.r"].numpy(), mo["mano.pose.l"].numpy()
        out[case + "/keys"] = np.array(list(data.keys()))
        for k, v in data.items():
            if "pred.nn_" in k:                     # nn_reference's output, not the reference's: not a fixture
                continue
            if torch.is_tensor(v) and (case == "partial" or v.numel() <= SMALL):
                out["%s/data/%s" % (case, k)] = v.numpy()
        for k, v in stats.items():
            out["%s/metric/%s" % (case, k)] = np.asarray(v, dtype=np.float64)
        # engine.py:784-794
        for k, v in stats.items():
            not_non_idx = ~np.isnan(stats[k])
            replace_value = float(stats[k][not_non_idx].mean())
            if replace_value != replace_value:
                stats = stats.rm(k)
            else:
                stats.overwrite(k, replace_value)
        steps[case] = dict(stats)
        for k in [k.split("/metric/")[1] for k in out if k.startswith(case + "/metric/")]:
            out["%s/step/%s" % (case, k)] = np.float64(steps[case].get(k, float("nan")))
    for case in EI.SEQUENCE:                        # MetricLogger.update(**stats): total += value, count += 1
        for k, v in steps[case].items():
            total[k] = total.get(k, 0.0) + v
            count[k] = count.get(k, 0) + 1
    for k in total:
        out["avg/" + k] = np.float64(total[k] / count[k])
    np.savez_compressed(os.path.join(HERE, "arctic_eval.npz"), **out)
    for case in EI.CASES:
        print(case, {k: np.round(out["%s/metric/%s" % (case, k)], 3) for k in ("success_rate/0.05", "cdev/ho", "aae")})
    print({k: float(out[k]) for k in out if k.startswith("avg/")})


if __name__ == "__main__":
    main()
