"""uvhand_amd — MI355X-native multi-scale deformable attention for UVHand.

Drop-in for the reference's ``models/ops`` package surface:

    from uvhand_amd.modules import MSDeformAttn              # models/ops/modules/ms_deform_attn.py
    from uvhand_amd.functions import MSDeformAttnFunction    # models/ops/functions/ms_deform_attn_func.py

Python host code on PyTorch-ROCm, hand-written HIP kernels (``csrc/``) behind the C ABI
declared in ``include/msda.h``.  There is no CPU or pure-PyTorch implementation in this
package: without the built HIP library every call raises.
"""
from ._native import set_exact_nonfinite
from .functions import MSDeformAttnFunction
from .graphs import graphed
from .modules import MSDeformAttn

# the ARCTIC evaluation step (uvhand_amd/arctic_eval.py), resolved on first use so that importing the op stays light
_ARCTIC_EVAL = ("get_NN", "nn_many", "make_output", "post_process_arctic_output", "prepare_data", "measure_error",
                "arctic_metrics", "ArcticEvaluator")
# the SmoothNet criterion's losses (uvhand_amd/smooth_loss.py), resolved the same way
_SMOOTH_LOSS = ("compute_smoothnet_loss", "smooth_loss_reference", "eval_acc_pose", "compute_error_accel")
# the step's first call, arctic_pre_process (uvhand_amd/pre_process.py), resolved the same way
_PRE_PROCESS = ("arctic_pre_process", "fit_targets", "distance_fields")
# the tail of the step, clip_grad_norm_ and AdamW (uvhand_amd/optim.py), resolved the same way
_OPTIM = ("AdamW", "clip_grad_norm_", "grad_norm")
__all__ = ["MSDeformAttn", "MSDeformAttnFunction", "graphed", "set_exact_nonfinite"] + list(_ARCTIC_EVAL) + list(_SMOOTH_LOSS) \
    + ["SmoothCriterion"] + list(_PRE_PROCESS) + list(_OPTIM)


def __getattr__(name):
    if name in _ARCTIC_EVAL:
        from . import arctic_eval
        return getattr(arctic_eval, name)
    if name in _SMOOTH_LOSS:
        from . import smooth_loss
        return getattr(smooth_loss, name)
    if name in _PRE_PROCESS:
        from . import pre_process
        return getattr(pre_process, name)
    if name in _OPTIM:
        from . import optim
        return getattr(optim, name)
    if name == "SmoothCriterion":
        from .modules import SmoothCriterion
        return SmoothCriterion
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
__version__ = "0.1.0"
