"""ctypes binding of ``libmsda_hip.so`` (C ABI: ``include/msda.h``).

This is the only route from Python to the HIP kernels, and there is no other
implementation behind it: if the library is missing or a call fails, this module
raises — it never falls back to PyTorch ops or to anything under ``oracle/``.

It stands where the reference's pybind module ``MultiScaleDeformableAttention``
stands (UVHand models/ops/src/vision.cpp:13-16, imported as ``MSDA`` at
models/ops/functions/ms_deform_attn_func.py:18) and reproduces the host-side
checks of models/ops/src/cuda/ms_deform_attn_cuda.cu:28-52, 93-117 and the
CPU-tensor error of models/ops/src/ms_deform_attn.h:38,60.
"""
import ctypes
import os
import warnings

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libmsda_hip.so")

_lib = None

# Every function of include/msda.h: "<return> <arguments>", one letter per C type (spaces only group them for the eye).
# tests/test_abi.py holds this table against the header, name by name and position by position.
_CTYPE = {"v": None, "i": ctypes.c_int, "u": ctypes.c_uint, "l": ctypes.c_longlong, "U": ctypes.c_ulonglong,
          "f": ctypes.c_float, "d": ctypes.c_double, "p": ctypes.c_void_p,      # p: any pointer, msda_stream_t included
          "s": ctypes.c_char_p, "q": ctypes.POINTER(ctypes.c_ulonglong)}          # the two pointers ctypes converts itself
SIGNATURES = {
    # the op
    "msda_forward_f32": "i ppppp iiiiiii pp",
    "msda_backward_f32": "i pppppp iiiiiii pppp",
    "msda_forward_f64": "i ppppp iiiiiii pp",
    "msda_backward_f64": "i pppppp iiiiiii pppp",
    "msda_forward_bf16": "i ppppp iiiiiii pp",
    "msda_backward_bf16": "i pppppp iiiiiii pppp",
    "msda_backward_bf16_gv32": "i pppppp iiiiiii pppp",
    "msda_backward_passes": "i ii",
    # backward with flags and caller-provided scratch
    "msda_backward_workspace_bytes": "U iiiiiii u",
    "msda_deterministic_supported": "i iiiiiiii",
    "msda_backward_ws_f32": "i pppppp iiiiiii pppp U u p",
    "msda_backward_ws_f64": "i pppppp iiiiiii pppp U u p",
    "msda_backward_ws_bf16": "i pppppp iiiiiii pppp U u p",
    "msda_backward_ws_bf16_gv32": "i pppppp iiiiiii pppp U u p",
    # forward that prepares its backward
    "msda_forward_workspace_bytes": "U iiiiiii u",
    "msda_forward_ws_f32": "i ppppp iiiiiii pp U p",
    "msda_forward_ws_bf16": "i ppppp iiiiiii pp U p",
    # fused module prologue
    "msda_prologue_supported": "i iiiiiii",
    "msda_forward_prologue_f32": "i pppppp iiiiiii ll pppp",
    "msda_backward_prologue_f32": "i pppppp iiiiiii ll ppppp",
    "msda_forward_prologue_ws_f32": "i pppppp iiiiiii ll pppp U p",
    "msda_backward_prologue_ws_f32": "i pppppp iiiiiii ll ppppp U u p",
    "msda_forward_prologue_bf16": "i pppppp iiiiiii ll pppp",
    "msda_forward_prologue_ws_bf16": "i pppppp iiiiiii ll pppp U p",
    "msda_backward_prologue_bf16_gv32": "i pppppp iiiiiii ll ppppp U u p",
    # bracketing projections
    "msda_linear_wgrad_workspace_bytes": "U iii",
    "msda_linear_wgrad_f32": "i pp iii pppp",
    "msda_linear_wgrad_masked_f32": "i ppp iii pppp",
    "msda_linear_wgrad_masked_bf16": "i ppp iii pppp",
    "msda_linear_wgrad_multi": "i i pppp ppp pppp",
    "msda_linear_wgrad_multi_f32": "i i ppp ppp pppp",
    "msda_zero_masked_rows_f32": "i pp l i p",
    "msda_cast_bf16_multi_f32": "i i pppp",
    "msda_linear_forward_f32": "i pppp l ii pp",
    "msda_linear_dgrad_f32": "i ppp l ii pp",
    # residual add + LayerNorm, FFN
    "msda_add_layernorm_workspace_bytes": "U l i",
    "msda_add_layernorm_forward_f32": "i pppp l i f pppp",
    "msda_add_layernorm_backward_f32": "i pppppp l i ppppp",
    "msda_add_layernorm_forward_f32_bf16res": "i pppp l i f pppp",
    "msda_add_layernorm_backward_f32_bf16res": "i pppppp l i pppppp",
    "msda_relu_dropout_backward_f32": "i pp f l p",
    # decoder self-attention core
    "msda_attn32_supported": "i iii",
    "msda_attn32_forward_f32": "i pll pll pll iiii ff p pll pp",
    "msda_attn32_backward_f32": "i pll pll pll pll p pll iiii ff p pll pll pll p",
    "msda_attn32_forward_bf16": "i pll pll pll iiii ff p pll pp",
    "msda_attn32_backward_bf16": "i pll pll pll pll p pll iiii ff p pll pll pll p",
    "msda_attn32x_supported": "i iii",
    "msda_attn32x_forward_f32": "i pll pll pll iiii ff p pl pll pp",
    "msda_attn32x_backward_f32": "i pll pll pll pll p pll iiii ff p pl pll pll pll p",
    "msda_attn32x_forward_bf16": "i pll pll pll iiii ff p pl pll pp",
    "msda_attn32x_backward_bf16": "i pll pll pll pll p pll iiii ff p pl pll pll pll p",
    # transformer input assembly
    "msda_flatten_levels_f32": "i i ppppp ii ppp",
    "msda_unflatten_levels_f32": "i i pppp ii ppppp",
    "msda_unflatten_workspace_bytes": "U i pp ii",
    "msda_last_error": "s",
    # two-stage query selection
    "msda_two_stage_proposals_f32": "i pp iiii ppppppp",
    "msda_two_stage_select_supported": "i iii",
    "msda_two_stage_select_f32": "i pppp iiiiii pppp",
    "msda_proposal_pos_embed_f32": "i pp l pp",
    "msda_proposal_pos_linear_relu_f32": "i pppp l i pp",
    # the AssemblyHands transformer
    "msda_assembly_refine_f32": "i p i p i p l pp",
    "msda_assembly_proposals_f32": "i p l p l iiii pppp",
    "msda_assembly_select_f32": "i ppp iiiiiii ppp",
    # the DINO decoder's query positions and refinement
    "msda_dino_sine_embed_f32": "i p i p i l pp p",
    "msda_dino_query_pos_supported": "i ii l ii",
    "msda_dino_query_pos_forward_f32": "i p i p i l ppppp pp p",
    "msda_dino_refine_forward_f32": "i pp i pp ii l pp p",
    "msda_dino_refine_backward_f32": "i ppp l pp p",
    # DINO's two-stage query selection for any number of rows per frame
    "msda_dino_select_supported": "i iiii",
    "msda_dino_select_workspace_bytes": "U ii",
    "msda_dino_select_forward_f32": "i ppp iiiiiii ppppp p p",
    "msda_dino_select_backward_f32": "i pp iiii p p",
    # DINO's contrastive-denoising queries
    "msda_cdn_supported": "i ii ll",
    "msda_cdn_prepare_forward_f32": "i ppppp i l ii l iii u f pppp p",
    "msda_cdn_prepare_backward_f32": "i pp l i l p p",
    # the Hungarian matchers
    "msda_match_arctic_f32": "i ppp iiiii ppp l p i ff ppp",
    "msda_match_assembly_f32": "i pp iiiii ppp l i ff ppp",
    "msda_lsap_f32": "i p iii pp",
    # the set criteria's matched losses
    "msda_criterion_fwd_f32": "i i ppp iiiii p i ppp l pp U p f ppp",
    "msda_criterion_bwd_f32": "i i ppp iiiii p i ppp l pp U p f pppppp",
    # the DINO criterion's matched and denoising losses
    "msda_criterion_dino_fwd_f32": "i ppp pp iiiiii p ii ppp l p U p f p U pp p",
    "msda_criterion_dino_bwd_f32": "i ppp pp iiiiii p ii ppp l p U p f pp ppp p",
    # the DeformableDETR prediction heads
    "msda_heads_supported": "i i",
    "msda_heads_workspace_bytes": "U ii l iii u",
    "msda_heads_forward_f32": "i ii l iiii u ppppppppp pppppp",
    "msda_heads_backward_f32": "i ii l iiii u ppppppppp ppppp pppppppp U p",
    "msda_heads_ref_backward_f32": "i i l ii pppp pp p",
    "msda_heads_bf16_supported": "i i",
    "msda_heads_bf16_workspace_bytes": "U ii l iii u",
    "msda_ffn_bf16_supported": "i ii",
    "msda_ffn_bf16_workspace_bytes": "U l ii",
    "msda_ffn_forward_bf16": "i l ii p i pppp d p ppp p",
    "msda_ffn_backward_bf16": "i l ii ppppp d p i pppp p U p",
    "msda_heads_forward_bf16": "i ii l iiii u ppppppppp pppppp",
    "msda_heads_backward_bf16": "i ii l iiii u ppppppppp ppppp pppppppp U p",
    # SmoothNet and get_arctic_item's selection
    "msda_smoother_supported": "i iiiii",
    "msda_smoother_workspace_bytes": "U iiiiiii ppp i",
    "msda_smoother_forward_f32": "i iiiiiii ppp pppp U i f pp",
    "msda_smoother_backward_f32": "i iiiiiii ppp ppp U ppp i f pp U p",
    "msda_smoother_dropout_mask_f32": "i p iiii f pp",
    "msda_arctic_item_forward_f32": "i iiiiii ppppp",
    "msda_arctic_item_backward_f32": "i ii pppp",
    "msda_arctic_item_many_forward": "i iiiiiiii ppppp",
    "msda_arctic_item_many_backward": "i iiii pppp",
    # Swin window attention
    "msda_swin_attn_supported": "i iiiiiii",
    "msda_swin_attn_workspace_bytes": "U iiiiiiii",
    "msda_swin_attn_forward_f32": "i iiiiiii ppppp U p",
    "msda_swin_attn_backward_f32": "i iiiiiii ppppp U ppppp U p",
    "msda_swin_attn_forward_bf16": "i iiiiiii ppppp U p",
    "msda_swin_attn_backward_bf16": "i iiiiiii ppppp U ppppp U p",
    # the Swin blocks' residual / drop-path / LayerNorm glue and PatchMerging's gather + norm
    "msda_swin_glue_supported": "i i",
    "msda_swin_glue_workspace_bytes": "U l i",
    "msda_swin_glue_norm_forward_f32": "i ppp l i f ppp p",
    "msda_swin_glue_norm_forward_bf16": "i ppp l i f ppp p",
    "msda_swin_glue_norm_backward_f32": "i ppppp l i pppp U p",
    "msda_swin_glue_norm_backward_bf16": "i ppppp l i pppp U p",
    "msda_swin_glue_add_norm_forward_f32": "i ppp ll i pp f pppp p",
    "msda_swin_glue_add_norm_forward_bf16": "i ppp ll i pp f pppp p",
    "msda_swin_glue_add_norm_backward_f32": "i ppppppp ll i ppppp U p",
    "msda_swin_glue_add_norm_backward_bf16": "i ppppppp ll i ppppp U p",
    "msda_swin_glue_add_forward_f32": "i ppp ll i p p",
    "msda_swin_glue_add_forward_bf16": "i ppp ll i p p",
    "msda_swin_glue_add_backward_f32": "i pp ll i p p",
    "msda_swin_glue_add_backward_bf16": "i pp ll i p p",
    "msda_swin_glue_merge_norm_forward_f32": "i p iiii pp f ppp p",
    "msda_swin_glue_merge_norm_forward_bf16": "i p iiii pp f ppp p",
    "msda_swin_glue_merge_norm_backward_f32": "i ppppp iiii pppp U p",
    "msda_swin_glue_merge_norm_backward_bf16": "i ppppp iiii pppp U p",
    "msda_swin_glue_norm_forward_f32_sbf16": "i ppp l i f ppp p",
    "msda_swin_glue_norm_forward_bf16_sbf16": "i ppp l i f ppp p",
    "msda_swin_glue_norm_backward_f32_sbf16": "i ppppp l i pppp U p",
    "msda_swin_glue_norm_backward_bf16_sbf16": "i ppppp l i pppp U p",
    "msda_swin_glue_add_norm_forward_bf16_sbf16": "i ppp ll i pp f pppp p",
    "msda_swin_glue_add_norm_backward_bf16_sbf16": "i ppppppp ll i ppppp U p",
    "msda_swin_glue_add_forward_bf16_sbf16": "i ppp ll i p p",
    "msda_swin_glue_add_backward_bf16_sbf16": "i pp ll i p p",
    "msda_swin_glue_merge_norm_forward_bf16_sbf16": "i p iiii pp f ppp p",
    "msda_swin_glue_merge_norm_backward_bf16_sbf16": "i ppppp iiii pppp U p",
    # MANO hand layer
    "msda_mano_supported": "i iii",
    "msda_mano_workspace_bytes": "U iiii p",
    "msda_mano_forward_f32": "i iiii pp i ppp ppp",
    "msda_mano_backward_f32": "i iiii pp i ppp pppp U p",
    # ARCTIC object layer and small losses
    "msda_object_supported": "i iiiiiii",
    "msda_object_forward_f32": "i pp i ppp pp",
    "msda_object_backward_f32": "i pp i ppp ppp",
    "msda_small_loss_supported": "i iiiiiii",
    "msda_small_loss_workspace_bytes": "U iiiiiii",
    "msda_small_loss_forward_f32": "i p f pp pp U p",
    "msda_small_loss_backward_f32": "i p f pp ppp U p",
    # ARCTIC evaluation: nearest neighbour and metrics
    "msda_nn_supported": "i iii",
    "msda_nn_forward_f32": "i iiii pppp p",
    "msda_nn_backward_f32": "i iiii pppppp p",
    "msda_arctic_metrics_supported": "i iiiiii",
    "msda_arctic_metrics_f32": "i ppp p p",
    "msda_arctic_metrics_accumulate_f32": "i p i pp p",
    # the input-projection neck: conv bias + GroupNorm + feature mask
    "msda_neck_supported": "i iiii pp",
    "msda_neck_workspace_bytes": "U iii",
    "msda_neck_forward_f32": "i i ppppp pp iii f pppp p",
    "msda_neck_backward_f32": "i i ppppppp pp iii pppp p U p",
    # make_output's pose, camera and projection glue
    "msda_arctic_pose_supported": "i iii",
    "msda_arctic_pose_forward_f32": "i iiif ppp ppp p",
    "msda_arctic_pose_backward_f32": "i iiif ppp ppp pp p",
    "msda_arctic_m2aa_forward_f32": "i ii pp p",
    "msda_arctic_m2aa_backward_f32": "i ii ppp p",
    "msda_arctic_place_supported": "i iii",
    "msda_arctic_place_forward_f32": "i iif ppp ppp ppp p",
    "msda_arctic_place_backward_f32": "i iif ppp ppp ppp pp p",
    # the SmoothNet criterion: contact deviation and acceleration errors
    "msda_smooth_loss_supported": "i iiii",
    "msda_smooth_loss_workspace_bytes": "U iiii",
    "msda_smooth_loss_forward_f32": "i p f pp pp p U p",
    "msda_smooth_loss_backward_f32": "i p f pp p i p p U p",
    # ARCTIC target preparation: rigid fit, camera translation and distance fields
    "msda_pre_fit_supported": "i iii",
    "msda_pre_fit_f32": "i iii f pp p p",
    "msda_dist_fields_supported": "i iii",
    "msda_dist_fields_f32": "i iii pppp ff pp p",
    # the tail of the step: gradient norm, clip and AdamW as multi-tensor launches
    "msda_optim_supported": "i li",
    "msda_optim_chunk_elems": "i",
    "msda_optim_chunks": "l ipp",
    "msda_grad_sumsq_f32": "i il ppp p p",
    "msda_grad_norm_finish_f32": "i l p f p p",
    "msda_grad_scale_f32": "i il ppp p p",
    "msda_adamw_step_f32": "i il pppp pp pp i ppppp l p p",
    "msda_optim_advance_f32": "i ip p",
    "msda_grad_norm_finish_dev_f32": "i l p f p ip ip p",
    "msda_adamw_step_dev_f32": "i il pppp pp pp i p pp p",
    # introspection and test hooks
    "msda_version": "i",
    "msda_path_for": "i iiiii",
    "msda_describe_plan": "i iiiiiiiii u i s i",
    "msda_probe_row_gather": "i p U iii p q p",
    "msda_launch_count": "U",
    "msda_force_path": "v i",
}


def signature(name):
    """(restype, argtypes) of one C function, as ctypes types."""
    ret, _, args = SIGNATURES[name].partition(" ")
    return _CTYPE[ret], [_CTYPE[c] for c in args.replace(" ", "")]


def declare(lib):
    """Set restype and argtypes of every function of the table on a ctypes handle of the library; returns the handle."""
    for name in SIGNATURES:
        if not hasattr(lib, name):
            raise RuntimeError("uvhand_amd: %s does not export %s (stale build?)" % (LIB_PATH, name))
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = signature(name)
    return lib


def load():
    """Load (once) and return the ctypes handle; raise if the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "uvhand_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C uvhand_amd/csrc`). There is no non-HIP fallback for this op." % LIB_PATH)
    _lib = declare(ctypes.CDLL(LIB_PATH))
    return _lib


def _suffix(dtype):
    if dtype == torch.float32:
        return "f32"
    if dtype == torch.float64:
        return "f64"
    if dtype == torch.bfloat16:
        return "bf16"
    raise RuntimeError('"ms_deform_attn" not implemented for \'%s\'' % str(dtype).replace("torch.", ""))


def _check_inputs(named):
    # order and wording follow ms_deform_attn_cuda.cu:28-38 / :93-105
    value = named[0][1]
    if not value.is_cuda:
        raise RuntimeError("Not implemented on the CPU")          # ms_deform_attn.h:38,60
    dev = value.device
    ok = True
    for _, t in named:
        if not (t.is_contiguous() and t.is_cuda and t.device == dev):
            ok = False
            break
    if ok:
        return
    for name, t in named:
        if not t.is_contiguous():
            raise RuntimeError("%s tensor has to be contiguous" % name)
    for name, t in named:
        if not t.is_cuda:
            raise RuntimeError("%s must be a CUDA tensor" % name)
    for name, t in named:
        if t.device != dev:
            raise RuntimeError("%s must be on the same device as value (%s vs %s)" % (name, t.device, dev))


def _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step):
    if value.dim() != 4 or sampling_loc.dim() != 6 or attn_weight.dim() != 5:
        raise RuntimeError("ms_deform_attn: expected value[N,S,M,D], sampling_loc[N,Lq,M,L,P,2], "
                           "attn_weight[N,Lq,M,L,P]")
    N, S, M, D = value.shape
    L = spatial_shapes.shape[0]
    Lq, P = sampling_loc.shape[1], sampling_loc.shape[4]
    if tuple(sampling_loc.shape) != (N, Lq, M, L, P, 2) or tuple(attn_weight.shape) != (N, Lq, M, L, P):
        raise RuntimeError("ms_deform_attn: sampling_loc %s / attn_weight %s do not match value %s and %d levels"
                           % (tuple(sampling_loc.shape), tuple(attn_weight.shape), tuple(value.shape), L))
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("expected scalar type Long for spatial_shapes / level_start_index")
    if tuple(spatial_shapes.shape) != (L, 2) or tuple(level_start_index.shape) != (L,):
        raise RuntimeError("ms_deform_attn: spatial_shapes must be [L,2] and level_start_index [L]")
    step = min(N, int(im2col_step))                                # ms_deform_attn_cuda.cu:50-52
    if N > 0 and (step <= 0 or N % step != 0):
        raise RuntimeError("batch(%d) must divide im2col_step(%d)" % (N, step))
    return N, S, M, D, L, Lq, P


def _compute_dtypes(value, sampling_loc, attn_weight):
    """value-like tensors' dtype T and location-like tensors' dtype TL (include/msda.h)."""
    if sampling_loc.dtype != attn_weight.dtype:
        raise RuntimeError("expected sampling_loc and attn_weight to have the same dtype, got %s and %s"
                           % (sampling_loc.dtype, attn_weight.dtype))
    suf = _suffix(value.dtype)
    want_tl = torch.float32 if suf == "bf16" else value.dtype
    if sampling_loc.dtype != want_tl:
        raise RuntimeError("expected scalar type %s but found %s"
                           % (str(want_tl).replace("torch.", "").capitalize(),
                              str(sampling_loc.dtype).replace("torch.", "").capitalize()))
    return suf


# Test hook (tests/test_parity_gpu.py): msda_force_path() is THREAD-LOCAL in the library, so that no caller can flip the
# kernel family under another thread's launch.  A setting made through force_path() below is applied around each native
# call on whichever thread performs it (autograd runs backward on its own device thread) and withdrawn right after, so no
# thread keeps a stale override; a process that never forces a path pays one comparison per call.
_forced_path = -1


class _ForcedPathScope:
    __slots__ = ("lib", "active")

    def __init__(self, lib):
        self.lib, self.active = lib, _forced_path != -1

    def __enter__(self):
        if self.active:
            self.lib.msda_force_path(_forced_path)
        return self

    def __exit__(self, *exc):
        if self.active:
            self.lib.msda_force_path(-1)
        return False


def _raise(lib, rc, what):
    msg = lib.msda_last_error()
    raise RuntimeError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else "?"))


_VP = ctypes.c_void_p
FLAG_DETERMINISTIC = 1                                # MSDA_FLAG_DETERMINISTIC (include/msda.h)
FLAG_PROLOGUE = 2                                     # MSDA_FLAG_PROLOGUE
FLAG_FORWARD_TABLE = 4                                # MSDA_FLAG_FORWARD_TABLE
FLAG_EXACT_NONFINITE = 8                              # MSDA_FLAG_EXACT_NONFINITE

_extra_flags = 0


def set_exact_nonfinite(on=True):
    """Process-wide: every backward of the D = 32 family keeps the coarse levels on the sort + gather kernels instead of the
    dense matrix-core product (MSDA_FLAG_EXACT_NONFINITE, include/msda.h), so that a non-finite grad_output row makes exactly
    the grad_value rows non-finite that the reference's atomicAdd would (ms_deform_im2col_cuda.cuh:125-152) — the dense product
    spreads it over the whole level of that (batch, head).  Costs the dense levels' speed-up on large problems."""
    global _extra_flags
    _extra_flags = FLAG_EXACT_NONFINITE if on else 0
    from . import _ext
    ext = _ext.get()
    if ext is not None and hasattr(ext, "set_exact_nonfinite"):
        ext.set_exact_nonfinite(bool(on))


def deterministic_requested():
    """True when grad_value should be bitwise reproducible: torch.use_deterministic_algorithms(True) (the reference
    sets cudnn.deterministic, main.py:65-66, which does not cover its atomicAdd scatter) or MSDA_DETERMINISTIC=1."""
    return torch.are_deterministic_algorithms_enabled() or os.environ.get("MSDA_DETERMINISTIC", "0") not in ("", "0")

def _deterministic_for(lib, det, elem_bytes, N, S, M, D, L, Lq, P):
    """The deterministic flag of a backward call: `det`, unless the geometry has no deterministic kernel within the library's
    work bound (msda_deterministic_supported: outside the D = 32 family above 2^36 point tests) AND torch runs with
    use_deterministic_algorithms(True, warn_only=True) — then a warning and the default kernels, as torch does for its own
    ops without a deterministic form.  Without warn_only the library's refusal is raised."""
    if det and torch.is_deterministic_algorithms_warn_only_enabled():
        if not lib.msda_deterministic_supported(elem_bytes, N, S, M, D, L, Lq, P):
            warnings.warn("ms_deform_attn_backward: no deterministic grad_value kernel for this geometry within the work bound "
                          "(include/msda.h, MSDA_FLAG_DETERMINISTIC); running the default (atomic) kernel [warn_only]")
            return False
    return det


def _raw_stream(device):
    """hipStream_t of PyTorch's current stream on `device` (launch there: ms_deform_attn_cuda.cu:65,135)."""
    try:
        return torch._C._cuda_getCurrentRawStream(device.index)
    except AttributeError:                                   # older/newer torch without the private hook
        return torch.cuda.current_stream(device).cuda_stream


class _DeviceGuard:
    """No reference counterpart (it relies on torch.cuda.set_device(rank), util/misc.py:550): switch to
    the tensors' device only when it is not already current."""
    __slots__ = ("prev",)

    def __init__(self, device):
        cur = torch.cuda.current_device()
        self.prev = cur if cur != device.index else None
        if self.prev is not None:
            torch.cuda.set_device(device.index)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


def _launch(dev, name, what, *args):
    """The launch a wrapper ends in: on the tensors' device, msda.h's `name` with PyTorch's current stream there as the
    last argument; a non-zero status raises with the library's message.  The deformable-attention op's own four wrappers
    keep this sequence inline: they also hold _ForcedPathScope, and the extra frame showed in the backward's host time
    (profiles/native_signatures_host_time.md)."""
    lib = _lib or load()
    with _DeviceGuard(dev):
        rc = getattr(lib, name)(*args, _raw_stream(dev))
    if rc != 0:
        _raise(lib, rc, what)


def _forward_table(lib, N, S, M, D, L, Lq, P, device, prologue=False):
    """The buffer a forward of this geometry can fill with its point table for the backward of the same autograd node
    (msda_forward_workspace_bytes, include/msda.h: the point table of small problems, the per-range point lists of large
    ones); None where the backward's plan reads none."""
    flags = FLAG_PROLOGUE if prologue else 0
    nbytes = int(lib.msda_forward_workspace_bytes(N, S, M, D, L, Lq, P, flags))
    if not nbytes:
        return None
    # the same buffer goes to the backward with MSDA_FLAG_FORWARD_TABLE: the table first, that call's scratch behind it
    nbytes = max(nbytes, int(lib.msda_backward_workspace_bytes(N, S, M, D, L, Lq, P, flags | FLAG_FORWARD_TABLE)))
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step, with_table=None):
    """Replaces MSDA.ms_deform_attn_forward (vision.cpp:14). Returns out[N, Lq, M*D].
    with_table=True / False (the autograd Functions): returns (out, table) — with True the forward also leaves its per-point
    table (msda_forward_ws_*; None where the geometry's backward reads none) to be handed to ms_deform_attn_backward."""
    lib = _lib or load()
    _check_inputs((("value", value), ("spatial_shapes", spatial_shapes),
                   ("level_start_index", level_start_index), ("sampling_loc", sampling_loc),
                   ("attn_weight", attn_weight)))
    N, S, M, D, L, Lq, P = _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)
    suf = _compute_dtypes(value, sampling_loc, attn_weight)
    table = None
    with _DeviceGuard(value.device), _ForcedPathScope(lib):
        out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
        if with_table and suf != "f64":
            table = _forward_table(lib, N, S, M, D, L, Lq, P, value.device)
        if table is not None:
            rc = getattr(lib, "msda_forward_ws_" + suf)(
                value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(),
                attn_weight.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(), table.data_ptr(), table.numel(),
                _raw_stream(value.device))
        else:
            rc = getattr(lib, "msda_forward_" + suf)(
                value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), sampling_loc.data_ptr(),
                attn_weight.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(), _raw_stream(value.device))
    if rc != 0:
        _raise(lib, rc, "ms_deform_attn_forward")
    return out if with_table is None else (out, table)


def _backward_workspace(lib, N, S, M, D, L, Lq, P, device, flags=FLAG_DETERMINISTIC):
    """Scratch a backward call with these flags can use (msda_backward_workspace_bytes, include/msda.h): a stream-ordered
    torch buffer, or (None, 0) when the call needs none.  The caller keeps it alive until the launch is queued;
    the caching allocator only hands the block out again to work queued later on the same stream."""
    nbytes = int(lib.msda_backward_workspace_bytes(N, S, M, D, L, Lq, P, flags))
    if nbytes == 0:
        return None, 0
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), nbytes


def backward_passes(Lq, P):
    """Query chunks the D = 32 backward takes for Lq*P sampling points per (batch, head, level); 1 = single pass."""
    return int((_lib or load()).msda_backward_passes(Lq, P))


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                            im2col_step, fp32_grad_value=False, deterministic=None, table=None):
    """Replaces MSDA.ms_deform_attn_backward (vision.cpp:15).
    Returns (grad_value, grad_sampling_loc, grad_attn_weight).  fp32_grad_value (bf16 rows only): grad_value
    comes back in float32 (msda_backward_bf16_gv32, include/msda.h; the only bf16 backward outside D = 32).  deterministic (None = deterministic_requested()):
    bitwise reproducible grad_value (MSDA_FLAG_DETERMINISTIC; every kernel family and dtype)."""
    lib = _lib or load()
    _check_inputs((("value", value), ("spatial_shapes", spatial_shapes),
                   ("level_start_index", level_start_index), ("sampling_loc", sampling_loc),
                   ("attn_weight", attn_weight), ("grad_output", grad_output)))
    N, S, M, D, L, Lq, P = _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)
    suf = _compute_dtypes(value, sampling_loc, attn_weight)
    if grad_output.dtype != value.dtype or grad_output.numel() != N * Lq * M * D:
        raise RuntimeError("ms_deform_attn_backward: grad_output must be %s[%d,%d,%d]"
                           % (value.dtype, N, Lq, M * D))
    if fp32_grad_value and suf != "bf16":
        raise RuntimeError("fp32_grad_value applies to bfloat16 rows only")
    with _DeviceGuard(value.device), _ForcedPathScope(lib):
        grad_value = torch.empty_like(value, dtype=torch.float32) if fp32_grad_value else torch.empty_like(value)
        grad_loc = torch.empty_like(sampling_loc)
        grad_attn = torch.empty_like(attn_weight)
        det = deterministic_requested() if deterministic is None else bool(deterministic)
        det = _deterministic_for(lib, det, 8 if suf == "f64" else 4, N, S, M, D, L, Lq, P)
        # always through the entry with flags and scratch (msda_backward_workspace_bytes says how much a call can use: 0 for
        # most shapes); the deterministic flag reaches every kernel family and dtype
        flags = (FLAG_DETERMINISTIC if det else 0) | _extra_flags
        if table is not None:                                # the forward's table of this very call (with_table=True), scratch behind it
            ws, nbytes, flags = table, table.numel(), flags | FLAG_FORWARD_TABLE
        else:
            ws, nbytes = _backward_workspace(lib, N, S, M, D, L, Lq, P, value.device, flags)
        rc = getattr(lib, "msda_backward_ws_" + suf + ("_gv32" if fp32_grad_value else ""))(
            grad_output.data_ptr(), value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
            sampling_loc.data_ptr(), attn_weight.data_ptr(), N, S, M, D, L, Lq, P,
            grad_value.data_ptr(), grad_loc.data_ptr(), grad_attn.data_ptr(),
            ws.data_ptr() if ws is not None else None, nbytes, flags, _raw_stream(value.device))
    if rc != 0:
        _raise(lib, rc, "ms_deform_attn_backward")
    return grad_value, grad_loc, grad_attn


def linear_wgrad_supported(grad_out, inp):
    """fp32 (or both bfloat16), contiguous 2-D views [M, N] / [M, K] on one GPU, N and K multiples of 4."""
    return (grad_out.is_cuda and inp.is_cuda and grad_out.dtype == inp.dtype
            and grad_out.dtype in (torch.float32, torch.bfloat16)
            and grad_out.dim() == 2 and inp.dim() == 2 and grad_out.shape[0] == inp.shape[0]
            and grad_out.is_contiguous() and inp.is_contiguous() and grad_out.device == inp.device
            and grad_out.shape[1] % 4 == 0 and inp.shape[1] % 4 == 0 and inp.shape[0] < (1 << 30)
            and grad_out.data_ptr() % 16 == 0 and inp.data_ptr() % 16 == 0)


def _row_mask_ptr(row_mask, rows, device):
    if row_mask is None:
        return None
    if not (row_mask.dtype == torch.bool and row_mask.is_contiguous() and row_mask.numel() == rows
            and row_mask.device == device):
        raise RuntimeError("row_mask must be a contiguous bool tensor with one entry per row, on the same device")
    return row_mask.data_ptr()


def zero_masked_rows_(x, row_mask):
    """In place: x[r, :] = 0 where row_mask[r] (x: contiguous fp32 [rows, cols], cols % 4 == 0) — include/msda.h."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and x.shape[1] % 4 == 0):
        raise RuntimeError("zero_masked_rows_: expected a contiguous fp32 CUDA matrix with cols % 4 == 0")
    _launch(x.device, "msda_zero_masked_rows_f32", "zero_masked_rows_", x.data_ptr(),
            _row_mask_ptr(row_mask, x.shape[0], x.device), x.shape[0], x.shape[1])
    return x


def linear_wgrad(grad_out, inp, want_bias=True, row_mask=None):
    """(grad_weight[N,K], grad_bias[N] or None) = (grad_out^T @ inp, grad_out.sum(0)) — include/msda.h; float32 results
    also for bfloat16 operands.  Rows of grad_out with row_mask[r] True count as zero."""
    lib = _lib or load()
    if not linear_wgrad_supported(grad_out, inp):
        raise RuntimeError("linear_wgrad: expected contiguous fp32 (or both bf16) CUDA matrices [M,N] and [M,K] with N, K % 4 == 0")
    M, N = grad_out.shape
    K = inp.shape[1]
    gw = torch.empty((N, K), dtype=torch.float32, device=inp.device)
    gb = torch.empty((N,), dtype=torch.float32, device=inp.device) if want_bias else None
    nbytes = lib.msda_linear_wgrad_workspace_bytes(M, N, K)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=inp.device) if nbytes else None
    _launch(inp.device, "msda_linear_wgrad_masked_" + ("bf16" if grad_out.dtype == torch.bfloat16 else "f32"),
            "linear_wgrad", grad_out.data_ptr(), inp.data_ptr(), _row_mask_ptr(row_mask, M, inp.device), M, N, K,
            gw.data_ptr(), gb.data_ptr() if want_bias else None, ws.data_ptr() if ws is not None else None)
    return gw, gb


def linear_rows_supported(a, weight, reduce_dim):
    """fp32 contiguous [rows, reduce] matrix and [out, in] weight on one GPU, both feature counts multiples of 4, 16-byte aligned."""
    return (a.is_cuda and weight.is_cuda and a.device == weight.device and a.dtype == torch.float32 and weight.dtype == torch.float32
            and a.dim() == 2 and weight.dim() == 2 and a.is_contiguous() and weight.is_contiguous()
            and a.shape[1] == weight.shape[reduce_dim] and weight.shape[0] % 4 == 0 and weight.shape[1] % 4 == 0
            and a.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0)


def linear_forward(inp, weight, bias=None, row_mask=None):
    """inp[rows, in] @ weight[out, in].T + bias, rows with row_mask[r] True written as zeros — include/msda.h
    (msda_linear_forward_f32): one fp32-MFMA launch, fixed summation order."""
    if not linear_rows_supported(inp, weight, 1) or (bias is not None and not (
            bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == weight.shape[0]
            and bias.device == inp.device and bias.data_ptr() % 16 == 0)):
        raise RuntimeError("linear_forward: expected contiguous fp32 CUDA [rows, in] and [out, in] (+ [out]) with in, out % 4 == 0")
    rows, out_f, in_f = inp.shape[0], weight.shape[0], weight.shape[1]
    y = torch.empty((rows, out_f), dtype=torch.float32, device=inp.device)
    _launch(inp.device, "msda_linear_forward_f32", "linear_forward", inp.data_ptr(), weight.data_ptr(),
            bias.data_ptr() if bias is not None else None, _row_mask_ptr(row_mask, rows, inp.device), rows, out_f, in_f,
            y.data_ptr())
    return y


def linear_dgrad(grad_out, weight, row_mask=None):
    """grad_out[rows, out] @ weight[out, in], rows with row_mask[r] True written as zeros — include/msda.h (msda_linear_dgrad_f32)."""
    if not linear_rows_supported(grad_out, weight, 0):
        raise RuntimeError("linear_dgrad: expected contiguous fp32 CUDA [rows, out] and [out, in] with in, out % 4 == 0")
    rows, out_f, in_f = grad_out.shape[0], weight.shape[0], weight.shape[1]
    gx = torch.empty((rows, in_f), dtype=torch.float32, device=grad_out.device)
    _launch(grad_out.device, "msda_linear_dgrad_f32", "linear_dgrad", grad_out.data_ptr(), weight.data_ptr(),
            _row_mask_ptr(row_mask, rows, grad_out.device), rows, out_f, in_f, gx.data_ptr())
    return gx


def prologue_supported(value, reference_points, sampling_offsets, attn_logits):
    """True when the fused-prologue entry points (include/msda.h) can take these tensors."""
    if not (value.is_cuda and value.dtype == torch.float32 and sampling_offsets.dtype == torch.float32
            and attn_logits.dtype == torch.float32 and reference_points.dtype == torch.float32):
        return False
    if value.dim() != 4 or sampling_offsets.dim() != 6 or reference_points.dim() != 4 or reference_points.shape[-1] != 2:
        return False
    N, S, M, D = value.shape
    Lq, L, P = sampling_offsets.shape[1], sampling_offsets.shape[3], sampling_offsets.shape[4]
    lib = _lib or load()
    with _ForcedPathScope(lib):
        return bool(lib.msda_prologue_supported(N, S, M, D, L, Lq, P))


def _row_stride(t, name):
    """Floats between consecutive (batch, query) rows of `t` [N, Lq, ...]: the trailing dimensions must be
    dense and the batch stride Lq rows — i.e. `t` is a column block of a row-major [N*Lq, ld] matrix."""
    inner = 1
    for size, stride in zip(reversed(t.shape[2:]), reversed(t.stride()[2:])):
        if size != 1 and stride != inner:
            raise RuntimeError("%s tensor has to be contiguous within a query row" % name)
        inner *= size
    if t.shape[1] > 1:
        ld = t.stride(1)
    elif t.shape[0] > 1:
        ld = t.stride(0)                       # one query per batch element: the rows are the batch elements
    else:
        ld = inner
    if ld < inner or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * ld):
        raise RuntimeError("%s tensor has to be contiguous or a column block of a row-major matrix" % name)
    return ld


def prologue_geometry_supported(N, S, M, D, L, Lq, P):
    """msda_prologue_supported (include/msda.h) for fp32 tensors of these sizes."""
    lib = _lib or load()
    with _ForcedPathScope(lib):
        return bool(lib.msda_prologue_supported(N, S, M, D, L, Lq, P))


def _check_prologue_dtypes(spatial_shapes, level_start_index, **floats):
    """The fused-prologue entry points exist for float32 only (include/msda.h); index tensors are int64."""
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("expected scalar type Long for spatial_shapes / level_start_index")
    for name, t in floats.items():
        if t.dtype != torch.float32:
            raise RuntimeError("expected scalar type Float for %s but found %s"
                               % (name, str(t.dtype).replace("torch.", "").capitalize()))


def ms_deform_attn_forward_prologue(value, spatial_shapes, level_start_index, reference_points, sampling_offsets,
                                    attn_logits, im2col_step, with_table=None):
    """Fused-prologue forward (include/msda.h).  Returns (out, sampling_loc, attn_weight); the last two are
    what the reference's Python would have computed and are what the backward consumes.  `sampling_offsets`
    [N,Lq,M,L,P,2] and `attn_logits` [N,Lq,M,L*P] may be column blocks of one wider projection output."""
    lib = _lib or load()
    _check_inputs((("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                   ("reference_points", reference_points)))
    for name, t in (("sampling_offsets", sampling_offsets), ("attn_logits", attn_logits)):
        if not t.is_cuda or t.device != value.device:
            raise RuntimeError("%s must be a CUDA tensor on the device of value" % name)
    if value.dim() != 4 or sampling_offsets.dim() != 6:
        raise RuntimeError("ms_deform_attn_forward_prologue: expected value[N,S,M,D] and sampling_offsets[N,Lq,M,L,P,2]")
    N, S, M, D = value.shape
    Lq, L, P = sampling_offsets.shape[1], sampling_offsets.shape[3], sampling_offsets.shape[4]
    if (tuple(sampling_offsets.shape) != (N, Lq, M, L, P, 2) or tuple(attn_logits.shape) != (N, Lq, M, L * P)
            or tuple(reference_points.shape) != (N, Lq, L, 2) or tuple(spatial_shapes.shape) != (L, 2)
            or tuple(level_start_index.shape) != (L,)):
        raise RuntimeError("ms_deform_attn_forward_prologue: inconsistent shapes")
    bf16 = value.dtype == torch.bfloat16
    _check_prologue_dtypes(spatial_shapes, level_start_index, reference_points=reference_points,
                           sampling_offsets=sampling_offsets, attn_logits=attn_logits, **({} if bf16 else {"value": value}))
    ld_off, ld_log = _row_stride(sampling_offsets, "sampling_offsets"), _row_stride(attn_logits, "attn_logits")
    if reference_points.data_ptr() % 8:                      # a contiguous view at an odd element offset
        reference_points = reference_points.clone()
    step = min(N, int(im2col_step))
    if N > 0 and (step <= 0 or N % step != 0):
        raise RuntimeError("batch(%d) must divide im2col_step(%d)" % (N, step))
    with _DeviceGuard(value.device), _ForcedPathScope(lib):
        out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
        loc = torch.empty((N, Lq, M, L, P, 2), dtype=torch.float32, device=value.device)
        attn = torch.empty((N, Lq, M, L, P), dtype=torch.float32, device=value.device)
        table = _forward_table(lib, N, S, M, D, L, Lq, P, value.device, prologue=True) if with_table else None
        rc = getattr(lib, "msda_forward_prologue_ws_" + ("bf16" if bf16 else "f32"))(
            value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(), reference_points.data_ptr(),
            sampling_offsets.data_ptr(), attn_logits.data_ptr(), N, S, M, D, L, Lq, P, ld_off, ld_log, out.data_ptr(),
            loc.data_ptr(), attn.data_ptr(), table.data_ptr() if table is not None else None,
            table.numel() if table is not None else 0, _raw_stream(value.device))
    if rc != 0:
        _raise(lib, rc, "ms_deform_attn_forward_prologue")
    return (out, loc, attn) if with_table is None else (out, loc, attn, table)


def ms_deform_attn_backward_prologue(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output,
                                     merged=False, deterministic=None, use_workspace=True, table=None):
    """Returns (grad_value (float32, also for bf16 rows), grad_sampling_offsets, grad_attn_logits[N,Lq,M,L*P],
    grad_reference_points[N,Lq,L,2]).
    merged=True: the two raw gradients are the column blocks [0, 2*M*L*P) and [2*M*L*P, 3*M*L*P) of ONE
    [N, Lq, 3*M*L*P] tensor — the gradient of a merged offsets+logits projection — returned as a fifth value."""
    lib = _lib or load()
    _check_inputs((("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                   ("sampling_loc", sampling_loc), ("attn_weight", attn_weight), ("grad_output", grad_output)))
    # same checks as the plain backward (the kernels reinterpret device memory: a wrong dtype is silent garbage)
    N, S, M, D, L, Lq, P = _dims(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, max(1, value.shape[0]))
    bf16 = value.dtype == torch.bfloat16
    _check_prologue_dtypes(spatial_shapes, level_start_index, sampling_loc=sampling_loc, attn_weight=attn_weight,
                           **({} if bf16 else {"value": value, "grad_output": grad_output}))
    if bf16 and grad_output.dtype != torch.bfloat16:
        raise RuntimeError("expected scalar type BFloat16 for grad_output (bf16 rows)")
    if grad_output.numel() != N * Lq * M * D:
        raise RuntimeError("ms_deform_attn_backward_prologue: grad_output must be float32[%d,%d,%d]" % (N, Lq, M * D))
    mlp = M * L * P
    with _DeviceGuard(value.device), _ForcedPathScope(lib):
        gv = torch.empty_like(value, dtype=torch.float32)          # fp32 also for bf16 rows (msda_backward_prologue_bf16_gv32)
        if merged:
            both = torch.empty((N, Lq, 3 * mlp), dtype=torch.float32, device=value.device)
            goff, glog = both[..., :2 * mlp].view(N, Lq, M, L, P, 2), both[..., 2 * mlp:].view(N, Lq, M, L * P)
            ld_off = ld_log = 3 * mlp
        else:
            both = None
            goff = torch.empty_like(sampling_loc)
            glog = torch.empty((N, Lq, M, L * P), dtype=torch.float32, device=value.device)
            ld_off = ld_log = 0
        gref = torch.empty((N, Lq, L, 2), dtype=torch.float32, device=value.device)
        det = deterministic_requested() if deterministic is None else bool(deterministic)
        # use_workspace=False (tests): the call a caller without scratch makes — the library then runs the kernels that need none
        flags = (FLAG_DETERMINISTIC if det else 0) | _extra_flags
        if table is not None:                                # the forward's table (with_table=True of the forward), scratch behind it
            ws, flags = table, flags | FLAG_FORWARD_TABLE
            nbytes = table.numel() if use_workspace else min(table.numel(), int(lib.msda_forward_workspace_bytes(N, S, M, D, L, Lq, P, FLAG_PROLOGUE)))
        else:
            ws, nbytes = _backward_workspace(lib, N, S, M, D, L, Lq, P, value.device,
                                             FLAG_PROLOGUE | (FLAG_DETERMINISTIC if det else 0)) if use_workspace else (None, 0)
        rc = getattr(lib, "msda_backward_prologue_bf16_gv32" if bf16 else "msda_backward_prologue_ws_f32")(
            grad_output.data_ptr(), value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
            sampling_loc.data_ptr(), attn_weight.data_ptr(), N, S, M, D, L, Lq, P, ld_off, ld_log, gv.data_ptr(),
            goff.data_ptr(), glog.data_ptr(), gref.data_ptr(), ws.data_ptr() if ws is not None else None, nbytes,
            flags, _raw_stream(value.device))
    if rc != 0:
        _raise(lib, rc, "ms_deform_attn_backward_prologue")
    return (gv, goff, glog, gref, both) if merged else (gv, goff, glog, gref)


def relu_dropout_backward_(grad, act, scale):
    """grad *= scale * (act > 0), in place (msda_relu_dropout_backward_f32, include/msda.h): the backward of
    dropout(relu(h)) from act = dropout(relu(h)).  fp32 CUDA tensors of the same size, contiguous, 16-byte aligned."""
    n = grad.numel()
    if not (grad.is_cuda and act.is_cuda and grad.dtype == act.dtype == torch.float32 and act.numel() == n
            and grad.is_contiguous() and act.is_contiguous()):
        raise RuntimeError("relu_dropout_backward_: expected two contiguous float32 CUDA tensors of one size")
    _launch(grad.device, "msda_relu_dropout_backward_f32", "relu_dropout_backward_", grad.data_ptr(), act.data_ptr(),
            float(scale), n)
    return grad


def _attn_view(t, name, heads, dtype=torch.float32):
    """[L, N, heads*32] float32 (bfloat16) CUDA view with the last dimension contiguous -> (pointer, batch stride, sequence stride)."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 3 and t.shape[2] == heads * 32
            and t.stride(2) == 1):
        raise RuntimeError("attn32: %s must be a %s CUDA tensor [L, N, heads*32] with a contiguous last dimension"
                           % (name, str(dtype).replace("torch.", "")))
    return t.data_ptr(), t.stride(1), t.stride(0)


def _attn_dtype(q):
    """The core's operand type: bfloat16 -> the msda_attn32_*_bf16 entries, anything else -> the fp32 ones (which check it)."""
    return torch.bfloat16 if torch.is_tensor(q) and q.dtype == torch.bfloat16 else torch.float32


def attn32_supported(Lq, Lk, head_dim):
    lib = _lib or load()
    return bool(lib.msda_attn32_supported(int(Lq), int(Lk), int(head_dim)))


def attn32x_supported(Lq, Lk, head_dim):
    lib = _lib or load()
    return bool(lib.msda_attn32x_supported(int(Lq), int(Lk), int(head_dim)))


def _attn_mask_bytes(mask, Lq, Lk, who):
    """A 2-D bool (or uint8) CUDA mask [Lq, Lk], True = hidden -> (its bytes, row stride); no copy when its last dimension is
    contiguous.  The returned tensor keeps the bytes alive for the call."""
    if mask is None:
        return None, None, 0
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.dtype in (torch.bool, torch.uint8) and tuple(mask.shape) == (Lq, Lk)):
        raise RuntimeError("%s: mask must be a bool CUDA tensor [Lq, Lk] = [%d, %d]" % (who, Lq, Lk))
    if mask.stride(1) != 1 or (Lq > 1 and mask.stride(0) < Lk):
        mask = mask.contiguous()
    mbytes = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return mbytes, mbytes.data_ptr(), (mbytes.stride(0) if Lq > 1 else max(Lk, mbytes.stride(0)))


def _attn_entry(family, who, dt, Lq, Lk, dropout_p, seed, mask):
    """The C entry of a family ("attn32": resident, "attn32x": streaming, with a mask) and operand type, and its seed (and mask)
    arguments after the seed check; the last item keeps the mask's bytes alive for the call."""
    if dropout_p > 0 and not (torch.is_tensor(seed) and seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1):
        raise RuntimeError("%s: dropout needs a one-element int64 CUDA seed tensor" % who)
    tail, mkeep = [seed.data_ptr() if dropout_p > 0 else None], None
    if family == "attn32x":
        mkeep, mptr, msq = _attn_mask_bytes(mask, Lq, Lk, who)
        tail += [mptr, msq]
    return "msda_%s_%s" % (who, "bf16" if dt == torch.bfloat16 else "f32"), tail, mkeep


def _attn_forward(family, q, k, v, heads, scale, dropout_p, seed, mask=None):
    who = family + "_forward"
    Lq, N, Lk = q.shape[0], q.shape[1], k.shape[0]
    dt = _attn_dtype(q)
    qv, kv, vv = _attn_view(q, "q", heads, dt), _attn_view(k, "k", heads, dt), _attn_view(v, "v", heads, dt)
    entry, tail, mkeep = _attn_entry(family, who, dt, Lq, Lk, dropout_p, seed, mask)
    out = torch.empty((Lq, N, heads * 32), dtype=dt, device=q.device)
    lse = torch.empty((N * heads, Lq), dtype=torch.float32, device=q.device)
    ov = _attn_view(out, "out", heads, dt)
    _launch(q.device, entry, who, *qv, *kv, *vv, N, heads, Lq, Lk, float(scale), float(dropout_p), *tail, *ov, lse.data_ptr())
    return out, lse


def _attn_backward(family, q, k, v, out, lse, grad_out, heads, scale, dropout_p, seed, mask, grad_q, grad_k, grad_v):
    who = family + "_backward"
    Lq, N, Lk = q.shape[0], q.shape[1], k.shape[0]
    dt = _attn_dtype(q)
    grad_q = torch.empty((Lq, N, heads * 32), dtype=dt, device=q.device) if grad_q is None else grad_q
    grad_k = torch.empty((Lk, N, heads * 32), dtype=dt, device=q.device) if grad_k is None else grad_k
    grad_v = torch.empty((Lk, N, heads * 32), dtype=dt, device=q.device) if grad_v is None else grad_v
    if grad_out.stride(2) != 1:
        grad_out = grad_out.contiguous()
    views = [_attn_view(t, nm, heads, dt) for t, nm in ((q, "q"), (k, "k"), (v, "v"), (out, "out"))]
    gov = _attn_view(grad_out, "grad_out", heads, dt)
    gviews = [_attn_view(t, nm, heads, dt) for t, nm in ((grad_q, "grad_q"), (grad_k, "grad_k"), (grad_v, "grad_v"))]
    entry, tail, mkeep = _attn_entry(family, who, dt, Lq, Lk, dropout_p, seed, mask)
    _launch(q.device, entry, who, *views[0], *views[1], *views[2], *views[3], lse.data_ptr(), *gov, N, heads, Lq, Lk, float(scale),
            float(dropout_p), *tail, *gviews[0], *gviews[1], *gviews[2])
    return grad_q, grad_k, grad_v


def attn32_forward(q, k, v, heads, scale, dropout_p=0.0, seed=None):
    """msda_attn32_forward_f32 (include/msda.h): dropout(softmax(q k^T * scale)) v per (batch, head), head_dim 32.
    q [Lq, N, E], k / v [Lk, N, E] (sequence first, as nn.MultiheadAttention projects them; column-block views allowed);
    seed: a one-element int64 CUDA tensor (required when dropout_p > 0).  Returns (out [Lq, N, E], lse [N*heads, Lq]).
    bfloat16 q, k, v take msda_attn32_forward_bf16 (out bfloat16, lse float32; the same dropout mask for the same seed)."""
    return _attn_forward("attn32", q, k, v, heads, scale, dropout_p, seed)


def attn32_backward(q, k, v, out, lse, grad_out, heads, scale, dropout_p=0.0, seed=None, grad_q=None, grad_k=None, grad_v=None):
    """msda_attn32_backward_f32: gradients of q, k, v (written into grad_q / grad_k / grad_v when given — views like the inputs,
    e.g. the two column blocks of one packed [L, N, 2E] tensor — else into new contiguous tensors).  bfloat16 q takes
    msda_attn32_backward_bf16: every tensor but lse bfloat16, gradients included."""
    return _attn_backward("attn32", q, k, v, out, lse, grad_out, heads, scale, dropout_p, seed, None, grad_q, grad_k, grad_v)


def attn32x_forward(q, k, v, heads, scale, dropout_p=0.0, seed=None, mask=None):
    """msda_attn32x_forward_f32 (include/msda.h): dropout(softmax(q k^T * scale + M)) v per (batch, head), head_dim 32, float32,
    1 <= Lq, Lk <= 2048.  Arguments as attn32_forward; mask: a 2-D bool CUDA tensor [Lq, Lk] shared by every batch entry and
    head, True = the key is hidden (passed as its bytes), or None.  Returns (out [Lq, N, E], lse [N*heads, Lq]).
    bfloat16 q, k, v take msda_attn32x_forward_bf16 (out bfloat16, lse float32; the same dropout mask for the same seed)."""
    return _attn_forward("attn32x", q, k, v, heads, scale, dropout_p, seed, mask)


def attn32x_backward(q, k, v, out, lse, grad_out, heads, scale, dropout_p=0.0, seed=None, mask=None, grad_q=None, grad_k=None,
                     grad_v=None):
    """msda_attn32x_backward_f32: gradients of q, k, v under the forward's mask and seed (written into grad_q / grad_k / grad_v
    when given — views like the inputs — else into new contiguous tensors).  bfloat16 q takes msda_attn32x_backward_bf16: every
    tensor but lse bfloat16, gradients included."""
    return _attn_backward("attn32x", q, k, v, out, lse, grad_out, heads, scale, dropout_p, seed, mask, grad_q, grad_k, grad_v)


def add_layernorm_supported(x, residual, weight, bias):
    """fp32 CUDA rows of a width the kernels take (multiple of 4, <= 1024), contiguous, 16-byte aligned."""
    d = x.shape[-1] if x.dim() else 0
    ts = [x, weight, bias] + ([residual] if residual is not None else [])
    return (x.dim() >= 1 and d % 4 == 0 and 0 < d <= 1024 and weight is not None and bias is not None
            and tuple(weight.shape) == (d,) and tuple(bias.shape) == (d,)
            and (residual is None or residual.shape == x.shape)
            and all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
                    and t.device == x.device for t in ts))


def add_layernorm_bf16res_supported(x, residual, weight, bias):
    """fp32 x (and parameters) as add_layernorm_supported, residual a bfloat16 tensor of x's shape, contiguous, 8-byte aligned."""
    return (torch.is_tensor(residual) and residual.dtype == torch.bfloat16 and residual.is_cuda and residual.is_contiguous()
            and residual.shape == x.shape and residual.device == x.device and residual.data_ptr() % 8 == 0
            and add_layernorm_supported(x, None, weight, bias))


def add_layernorm_forward_bf16res(x, residual, weight, bias, eps):
    """(y, mean, rstd) = LayerNorm(x + residual) for fp32 x and bfloat16 residual — msda_add_layernorm_forward_f32_bf16res."""
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _launch(x.device, "msda_add_layernorm_forward_f32_bf16res", "add_layernorm_forward_bf16res", x.data_ptr(),
            residual.data_ptr(), weight.data_ptr(), bias.data_ptr(), rows, d, float(eps), y.data_ptr(), mean.data_ptr(),
            rstd.data_ptr())
    return y, mean, rstd


def add_layernorm_backward_bf16res(grad_y, x, residual, weight, mean, rstd):
    """(grad_x fp32, grad_residual bf16 = grad_x rounded, grad_weight, grad_bias) — msda_add_layernorm_backward_f32_bf16res."""
    lib = _lib or load()
    d = x.shape[-1]
    rows = x.numel() // d
    gx = torch.empty_like(x)
    gr = torch.empty_like(residual)
    gw = torch.empty((d,), dtype=torch.float32, device=x.device)
    gb = torch.empty((d,), dtype=torch.float32, device=x.device)
    nbytes = max(16, int(lib.msda_add_layernorm_workspace_bytes(rows, d)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    _launch(x.device, "msda_add_layernorm_backward_f32_bf16res", "add_layernorm_backward_bf16res", grad_y.data_ptr(),
            x.data_ptr(), residual.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, d, gx.data_ptr(),
            gr.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr())
    return gx, gr, gw, gb


def add_layernorm_forward(x, residual, weight, bias, eps):
    """(y, mean, rstd) = LayerNorm(x + residual) — msda_add_layernorm_forward_f32 (include/msda.h)."""
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty_like(x)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _launch(x.device, "msda_add_layernorm_forward_f32", "add_layernorm_forward", x.data_ptr(),
            residual.data_ptr() if residual is not None else None, weight.data_ptr(), bias.data_ptr(), rows, d, float(eps),
            y.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    return y, mean, rstd


def add_layernorm_backward(grad_y, x, residual, weight, mean, rstd):
    """(grad_sum, grad_weight, grad_bias) — msda_add_layernorm_backward_f32; grad_sum is d/dx and d/dresidual."""
    lib = _lib or load()
    d = x.shape[-1]
    rows = x.numel() // d
    gs = torch.empty_like(x)
    gw = torch.empty((d,), dtype=torch.float32, device=x.device)
    gb = torch.empty((d,), dtype=torch.float32, device=x.device)
    nbytes = max(16, int(lib.msda_add_layernorm_workspace_bytes(rows, d)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    _launch(x.device, "msda_add_layernorm_backward_f32", "add_layernorm_backward", grad_y.data_ptr(), x.data_ptr(),
            residual.data_ptr() if residual is not None else None, weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows,
            d, gs.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr())
    return gs, gw, gb


def flatten_levels_supported(srcs, poss, level_embed):
    """fp32 contiguous NCHW CUDA feature maps of one batch size / channel count (a multiple of 4), at most 16 levels."""
    ts = list(srcs) + list(poss)
    if not ts or len(srcs) != len(poss) or len(srcs) > 16:
        return False
    n, c = ts[0].shape[0], ts[0].shape[1]
    return (c % 4 == 0 and all(t.dim() == 4 and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                               and t.shape[0] == n and t.shape[1] == c and t.device == ts[0].device for t in ts)
            and all(s.shape == p.shape for s, p in zip(srcs, poss))
            and level_embed.is_cuda and level_embed.dtype == torch.float32 and level_embed.is_contiguous()
            and tuple(level_embed.shape) == (len(srcs), c) and level_embed.data_ptr() % 16 == 0)


def _level_arrays(tensors):
    L = len(tensors)
    ptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in tensors])
    hs = (ctypes.c_int * L)(*[t.shape[2] for t in tensors])
    ws = (ctypes.c_int * L)(*[t.shape[3] for t in tensors])
    return ptrs, hs, ws


def flatten_levels(srcs, poss, level_embed):
    """(src_flatten[N,S,C], lvl_pos_embed_flatten[N,S,C]) — msda_flatten_levels_f32 (include/msda.h)."""
    L, (N, C) = len(srcs), srcs[0].shape[:2]
    S = sum(t.shape[2] * t.shape[3] for t in srcs)
    sp, hs, ws = _level_arrays(srcs)
    pp, _, _ = _level_arrays(poss)
    src_flat = torch.empty((N, S, C), dtype=torch.float32, device=srcs[0].device)
    pos_flat = torch.empty((N, S, C), dtype=torch.float32, device=srcs[0].device)
    _launch(srcs[0].device, "msda_flatten_levels_f32", "flatten_levels", L, sp, pp, level_embed.data_ptr(), hs, ws, N, C,
            src_flat.data_ptr(), pos_flat.data_ptr())
    return src_flat, pos_flat


def unflatten_levels(grad_src_flat, grad_pos_flat, shapes_nchw, want_level_embed=False):
    """Per-level NCHW gradients from the flattened ones (either may be None) and, on request, the level-embedding
    gradient [L, C] — msda_unflatten_levels_f32."""
    lib = _lib or load()
    ref = grad_src_flat if grad_src_flat is not None else grad_pos_flat
    N, S, C = ref.shape
    L = len(shapes_nchw)
    gs = [torch.empty(sh, dtype=torch.float32, device=ref.device) for sh in shapes_nchw] if grad_src_flat is not None else None
    gp = [torch.empty(sh, dtype=torch.float32, device=ref.device) for sh in shapes_nchw] if grad_pos_flat is not None else None
    hs = (ctypes.c_int * L)(*[sh[2] for sh in shapes_nchw])
    ws_ = (ctypes.c_int * L)(*[sh[3] for sh in shapes_nchw])
    sp = _level_arrays(gs)[0] if gs is not None else None
    pp = _level_arrays(gp)[0] if gp is not None else None
    gembed = ws = None
    if want_level_embed and grad_pos_flat is not None:
        gembed = torch.empty((L, C), dtype=torch.float32, device=ref.device)
        nbytes = max(16, int(lib.msda_unflatten_workspace_bytes(L, hs, ws_, N, C)))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=ref.device)
    _launch(ref.device, "msda_unflatten_levels_f32", "unflatten_levels", L, sp, pp, hs, ws_, N, C,
            grad_src_flat.data_ptr() if grad_src_flat is not None else None,
            grad_pos_flat.data_ptr() if grad_pos_flat is not None else None,
            gembed.data_ptr() if gembed is not None else None, ws.data_ptr() if ws is not None else None)
    return gs, gp, gembed


NECK_MAX_LEVELS = 8                     # kNeckMaxLevels (csrc/msda_launch.h)


def _ptr_table(tensors):
    """A host array of device pointers (None entries stay NULL), or None for no table."""
    if tensors is None:
        return None
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def neck_supported(ys, groups):
    """msda_neck_supported for per-level conv outputs [N, C, H_l, W_l] of one batch size and channel count."""
    L = len(ys)
    if not 1 <= L <= NECK_MAX_LEVELS:
        return False
    N, C = ys[0].shape[:2]
    hs = (ctypes.c_int * L)(*[t.shape[2] for t in ys])
    ws = (ctypes.c_int * L)(*[t.shape[3] for t in ys])
    return bool((_lib or load()).msda_neck_supported(L, N, C, groups, hs, ws))


def neck_forward(ys, biases, gammas, betas, uniforms, groups, eps):
    """(outs, means, rstds, masks) — msda_neck_forward_f32 (include/msda.h): one launch for all levels.  ys: contiguous fp32
    conv outputs without bias; biases: per-level tensors or None entries; uniforms: None or one tensor per level (masks is then
    a list of uint8 tensors, else None)."""
    L, (N, C) = len(ys), ys[0].shape[:2]
    dev = ys[0].device
    _, hs, ws = _level_arrays(ys)
    outs = [torch.empty_like(y) for y in ys]
    means = [torch.empty((N, groups), dtype=torch.float32, device=dev) for _ in ys]
    rstds = [torch.empty((N, groups), dtype=torch.float32, device=dev) for _ in ys]
    masks = [torch.empty(y.shape, dtype=torch.uint8, device=dev) for y in ys] if uniforms is not None else None
    _launch(dev, "msda_neck_forward_f32", "neck_forward", L, _ptr_table(ys), _ptr_table(biases), _ptr_table(gammas),
            _ptr_table(betas), _ptr_table(uniforms), hs, ws, N, C, groups, float(eps), _ptr_table(outs), _ptr_table(means),
            _ptr_table(rstds), _ptr_table(masks))
    return outs, means, rstds, masks


def neck_backward(grad_outs, ys, biases, gammas, means, rstds, masks, groups):
    """(grad_ys, grad_gammas, grad_betas, grad_biases) — msda_neck_backward_f32: two launches for all levels.  grad_biases has
    None where the level's conv has no bias."""
    lib = _lib or load()
    L, (N, C) = len(ys), ys[0].shape[:2]
    dev = ys[0].device
    _, hs, ws = _level_arrays(ys)
    gys = [torch.empty_like(y) for y in ys]
    ggs = [torch.empty((C,), dtype=torch.float32, device=dev) for _ in ys]
    gbs = [torch.empty((C,), dtype=torch.float32, device=dev) for _ in ys]
    gcs = [torch.empty((C,), dtype=torch.float32, device=dev) if b is not None else None for b in biases]
    nbytes = max(16, int(lib.msda_neck_workspace_bytes(L, N, C)))
    wsp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _launch(dev, "msda_neck_backward_f32", "neck_backward", L, _ptr_table(grad_outs), _ptr_table(ys), _ptr_table(biases),
            _ptr_table(gammas), _ptr_table(means), _ptr_table(rstds), _ptr_table(masks), hs, ws, N, C, groups, _ptr_table(gys),
            _ptr_table(ggs), _ptr_table(gbs), _ptr_table(gcs), wsp.data_ptr(), nbytes)
    return gys, ggs, gbs, gcs


PATH_GENERIC, PATH_D32 = 0, 1          # MSDA_PATH_* (include/msda.h)


def path_for(elem_bytes, M, D, L, P):
    with _ForcedPathScope(load()):
        return int(load().msda_path_for(elem_bytes, M, D, L, P))


def describe_plan(N, S, M, D, L, Lq, P, row_bytes=4, grad_value_bytes=None, prologue=False, deterministic=False,
                  has_workspace=True, exact_nonfinite=False):
    """msda_describe_plan (include/msda.h): which kernels / launch plan a call of this geometry takes, as text."""
    lib = _lib or load()
    buf = ctypes.create_string_buffer(512)
    flags = ((FLAG_PROLOGUE if prologue else 0) | (FLAG_DETERMINISTIC if deterministic else 0)
             | (FLAG_EXACT_NONFINITE if exact_nonfinite else 0))
    with _ForcedPathScope(lib):
        lib.msda_describe_plan(row_bytes, grad_value_bytes or row_bytes, N, S, M, D, L, Lq, P, flags, 1 if has_workspace else 0,
                               buf, len(buf))
    return buf.value.decode()


def probe_row_gather(table_bytes, device, row_bytes=128, blocks=4096, iters=16, repeats=5):
    """msda_probe_row_gather (include/msda.h): row requests per second the vector memory path of `device` serves on a table
    of `table_bytes` bytes with the sampling kernels' access pattern (measurement helper for bench.py)."""
    lib = _lib or load()
    table = torch.ones((max(int(table_bytes), row_bytes) // 4,), dtype=torch.float32, device=device)
    sink = torch.zeros((1,), dtype=torch.float32, device=device)
    rows = ctypes.c_ulonglong(0)
    fn = lib.msda_probe_row_gather
    with _DeviceGuard(device):
        stream = torch.cuda.current_stream(device)
        call = lambda: fn(table.data_ptr(), table.numel() * 4, row_bytes, blocks, iters, sink.data_ptr(), ctypes.byref(rows),
                          _raw_stream(device))
        for _ in range(2):
            if call() != 0:
                _raise(lib, 1, "msda_probe_row_gather")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(repeats):
            call()
        e1.record(stream)
        e1.synchronize()
    return rows.value * repeats / (e0.elapsed_time(e1) * 1e-3)


def launch_count():
    """msda_launch_count (include/msda.h): launches enqueued through the library by this process so far."""
    return int((_lib or load()).msda_launch_count())


def force_path(path):
    """Test hook: -1 = automatic selection, PATH_GENERIC = the generic kernels for every call made through this module."""
    global _forced_path
    load()
    _forced_path = int(path)


# ---- two-stage query selection of the transformer (csrc/msda_two_stage.hip) ----------------------------------------------
PE_WIDTH = 5376                                       # 42 coordinates x 128 sin / cos features (get_proposal_pos_embed)


def _f32_cuda(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def _check_f32(what, dev, tensors):
    """Every tensor (None entries skipped) contiguous fp32 on `dev`."""
    if not all(t is None or (_f32_cuda(t) and t.device == dev) for t in tensors):
        raise RuntimeError("%s: expected contiguous fp32 CUDA tensors on one device" % what)


def two_stage_proposals(memory, padding_mask, level_hw, learnedxy=None):
    """(proposals [N,S,42], memory_out [N,S,C], row_mask [N,S] bool) — msda_two_stage_proposals_f32: the forward of
    gen_encoder_output_proposals with `level_hw` the levels' (H, W) as Python ints."""
    if not (_f32_cuda(memory) and memory.dim() == 3 and padding_mask.dtype == torch.bool and padding_mask.is_contiguous()
            and padding_mask.device == memory.device and tuple(padding_mask.shape) == tuple(memory.shape[:2])
            and (learnedxy is None or (_f32_cuda(learnedxy) and learnedxy.numel() == 40 and learnedxy.device == memory.device))):
        raise RuntimeError("two_stage_proposals: expected contiguous fp32 CUDA memory [N,S,C], a bool mask [N,S] and learnedxy [40] or None")
    N, S, C = memory.shape
    L = len(level_hw)
    hs = (ctypes.c_int * max(1, L))(*[int(h) for h, _ in level_hw])
    ws = (ctypes.c_int * max(1, L))(*[int(w) for _, w in level_hw])
    props = torch.empty((N, S, 42), dtype=torch.float32, device=memory.device)
    mem_out = torch.empty_like(memory)
    row_mask = torch.empty((N, S), dtype=torch.bool, device=memory.device)
    _launch(memory.device, "msda_two_stage_proposals_f32", "two_stage_proposals", memory.data_ptr(), padding_mask.data_ptr(),
            N, S, C, L, ctypes.cast(hs, _VP), ctypes.cast(ws, _VP), learnedxy.data_ptr() if learnedxy is not None else None,
            props.data_ptr(), mem_out.data_ptr(), row_mask.data_ptr())
    return props, mem_out, row_mask


def two_stage_select_supported(S, K, Q):
    """Whether msda_two_stage_select_f32 takes a frame of S rows, K classes and Q queries (S <= 8192, Q <= S)."""
    return bool((_lib or load()).msda_two_stage_select_supported(int(S), int(K), int(Q)))


def two_stage_select(cls, hand, obj, proposals, num_queries, hand_classes=(12, 13)):
    """(topk [N,Q] int64, refpoint_unsig [N,Q,42], reference_points [N,Q,42]) — msda_two_stage_select_f32: one launch, no
    host synchronisation.  Raises RuntimeError when Q exceeds the rows per frame (as torch.topk does)."""
    ts = (cls, hand, obj, proposals)
    if not (all(_f32_cuda(t) and t.dim() == 3 and t.device == cls.device for t in ts)
            and all(tuple(t.shape) == tuple(cls.shape[:2]) + (42,) for t in ts[1:])):
        raise RuntimeError("two_stage_select: expected contiguous fp32 CUDA cls [N,S,K] and hand / obj / proposals [N,S,42]")
    N, S, K = cls.shape
    Q = int(num_queries)
    if Q > S:
        raise RuntimeError("selected index k out of range")
    topk = torch.empty((N, Q), dtype=torch.int64, device=cls.device)
    unsig = torch.empty((N, Q, 42), dtype=torch.float32, device=cls.device)
    refp = torch.empty((N, Q, 42), dtype=torch.float32, device=cls.device)
    _launch(cls.device, "msda_two_stage_select_f32", "two_stage_select", cls.data_ptr(), hand.data_ptr(), obj.data_ptr(),
            proposals.data_ptr(), N, S, K, Q, int(hand_classes[0]), int(hand_classes[1]), topk.data_ptr(), unsig.data_ptr(),
            refp.data_ptr())
    return topk, unsig, refp


def _check_pe_inputs(r2, dim_t):
    if not (_f32_cuda(r2) and r2.dim() == 2 and r2.shape[1] == 42 and _f32_cuda(dim_t) and dim_t.numel() == 64
            and dim_t.device == r2.device):
        raise RuntimeError("proposal_pos_embed: expected contiguous fp32 CUDA refpoints [M,42] and dim_t [64]")


def proposal_pos_embed(r2, dim_t):
    """PE [M, 5376] of refpoint_unsig [M, 42] — msda_proposal_pos_embed_f32 (dim_t: torch's table at even indices)."""
    _check_pe_inputs(r2, dim_t)
    pe = torch.empty((r2.shape[0], PE_WIDTH), dtype=torch.float32, device=r2.device)
    _launch(r2.device, "msda_proposal_pos_embed_f32", "proposal_pos_embed", r2.data_ptr(), dim_t.data_ptr(), r2.shape[0],
            pe.data_ptr())
    return pe


def proposal_pos_linear_relu(r2, dim_t, weight, bias):
    """relu(PE(r2) @ weight^T + bias) [M, out] without the PE table in memory — msda_proposal_pos_linear_relu_f32."""
    _check_pe_inputs(r2, dim_t)
    if not (_f32_cuda(weight) and weight.dim() == 2 and weight.shape[1] == PE_WIDTH and weight.shape[0] % 4 == 0
            and weight.device == r2.device and weight.data_ptr() % 16 == 0
            and (bias is None or (_f32_cuda(bias) and bias.numel() == weight.shape[0] and bias.device == r2.device))):
        raise RuntimeError("proposal_pos_linear_relu: expected contiguous fp32 CUDA weight [out, 5376] (out % 4 == 0) and bias [out]")
    y = torch.empty((r2.shape[0], weight.shape[0]), dtype=torch.float32, device=r2.device)
    _launch(r2.device, "msda_proposal_pos_linear_relu_f32", "proposal_pos_linear_relu", r2.data_ptr(), dim_t.data_ptr(),
            weight.data_ptr(), bias.data_ptr() if bias is not None else None, r2.shape[0], weight.shape[0], y.data_ptr())
    return y


# ---- the AssemblyHands transformer's refinement and two-stage block (csrc/msda_assembly.hip) ------------------------------
def assembly_refine(reference_points, cls, keypoints):
    """next reference_points [..., 42] — msda_assembly_refine_f32: reference_points [..., 2 | 42], the layer's class logits
    [..., K] and keypoint head output [..., 63], all contiguous fp32 CUDA with the same leading shape.  One launch."""
    lead = tuple(reference_points.shape[:-1])
    if not (all(_f32_cuda(t) and t.device == reference_points.device for t in (reference_points, cls, keypoints))
            and reference_points.shape[-1] in (2, 42) and tuple(cls.shape[:-1]) == lead
            and tuple(keypoints.shape) == lead + (63,) and cls.shape[-1] > 0):
        raise RuntimeError("assembly_refine: expected contiguous fp32 CUDA reference_points [..., 2|42], cls [..., K] and "
                           "keypoints [..., 63] with the same leading shape")
    M = reference_points.numel() // reference_points.shape[-1]
    out = torch.empty(lead + (42,), dtype=torch.float32, device=reference_points.device)
    _launch(reference_points.device, "msda_assembly_refine_f32", "assembly_refine", reference_points.data_ptr(),
            reference_points.shape[-1], cls.data_ptr(), cls.shape[-1], keypoints.data_ptr(), M, out.data_ptr())
    return out


def assembly_proposals(memory, padding_mask, hw):
    """(proposals [N,H*W,2], memory_out [N,H*W,C], row_mask [N,H*W] bool) — msda_assembly_proposals_f32 for one level of
    hw = (H, W) rows: memory [N, H*W, C] fp32 and padding_mask [N, H*W] bool may be slices of the full flattened tensors
    (rows contiguous inside a frame, any frame stride)."""
    H, W = int(hw[0]), int(hw[1])
    if not (memory.is_cuda and memory.dtype == torch.float32 and memory.dim() == 3 and memory.shape[1] == H * W
            and memory.stride(2) == 1 and memory.stride(1) == memory.shape[2] and padding_mask.dtype == torch.bool
            and padding_mask.device == memory.device and tuple(padding_mask.shape) == tuple(memory.shape[:2])
            and padding_mask.stride(1) == 1):
        raise RuntimeError("assembly_proposals: expected fp32 CUDA memory [N,H*W,C] and a bool mask [N,H*W], rows contiguous")
    N, S, C = memory.shape
    props = torch.empty((N, S, 2), dtype=torch.float32, device=memory.device)
    mem_out = torch.empty((N, S, C), dtype=torch.float32, device=memory.device)
    row_mask = torch.empty((N, S), dtype=torch.bool, device=memory.device)
    _launch(memory.device, "msda_assembly_proposals_f32", "assembly_proposals", memory.data_ptr(), memory.stride(0),
            padding_mask.data_ptr(), padding_mask.stride(0), N, H, W, C, props.data_ptr(), mem_out.data_ptr(),
            row_mask.data_ptr())
    return props, mem_out, row_mask


def assembly_select(cls, hand, obj, obj_classes=(1, 8), left=9, right=10):
    """(indices [N,3] int64 (left, right, object), reference_points [N,3,2]) — msda_assembly_select_f32: one launch, no host
    synchronisation.  Raises IndexError when a class index is not below K, as the reference's column indexing does."""
    ts = (cls, hand, obj)
    if not (all(_f32_cuda(t) and t.dim() == 3 and t.device == cls.device for t in ts)
            and all(tuple(t.shape) == tuple(cls.shape[:2]) + (63,) for t in ts[1:])):
        raise RuntimeError("assembly_select: expected contiguous fp32 CUDA cls [N,S,K] and hand / obj [N,S,63]")
    N, S, K = cls.shape
    top = max(int(obj_classes[1]), int(left), int(right))
    if top >= K:
        raise IndexError("index %d is out of bounds for dimension 2 with size %d" % (top, K))
    idx = torch.empty((N, 3), dtype=torch.int64, device=cls.device)
    refp = torch.empty((N, 3, 2), dtype=torch.float32, device=cls.device)
    _launch(cls.device, "msda_assembly_select_f32", "assembly_select", cls.data_ptr(), hand.data_ptr(), obj.data_ptr(), N, S,
            K, int(obj_classes[0]), int(obj_classes[1]), int(left), int(right), idx.data_ptr(), refp.data_ptr())
    return idx, refp


# ---- the DINO decoder's query positions and refinement (csrc/msda_dino.hip) -----------------------------------------------
DINO_PE_WIDTH = 256                                   # gen_sineembed_for_position's columns = ref_point_head's in / hidden / out


def _check_dino_rows(what, ref2, valid_xy, n_frames, dim_t):
    if not (_f32_cuda(ref2) and ref2.dim() == 2 and ref2.shape[1] in (2, 42) and n_frames > 0 and ref2.shape[0] % n_frames == 0
            and _f32_cuda(dim_t) and dim_t.numel() == 64 and dim_t.device == ref2.device
            and (valid_xy is None or (_f32_cuda(valid_xy) and tuple(valid_xy.shape) == (n_frames, 2)
                                      and valid_xy.device == ref2.device))):
        raise RuntimeError("%s: expected contiguous fp32 CUDA ref [L * N, 2 | 42] (sequence-first rows), valid_xy [N, 2] or None "
                           "and dim_t [64]" % what)


def dino_sine_embed(ref2, valid_xy, n_frames, dim_t):
    """pe [M, 256] of sequence-first rows ref2 [M, 2 | 42] (row m in frame m % n_frames) — msda_dino_sine_embed_f32."""
    _check_dino_rows("dino_sine_embed", ref2, valid_xy, n_frames, dim_t)
    M, W = ref2.shape
    pe = torch.empty((M, DINO_PE_WIDTH), dtype=torch.float32, device=ref2.device)
    _launch(ref2.device, "msda_dino_sine_embed_f32", "dino_sine_embed", ref2.data_ptr(), W,
            valid_xy.data_ptr() if valid_xy is not None else None, int(n_frames), M, dim_t.data_ptr(), pe.data_ptr())
    return pe


def dino_query_pos_supported(width, n_frames, rows, hidden, out_features):
    """Whether msda_dino_query_pos_forward_f32 takes this geometry (width 2 | 42, rows % frames == 0, hidden = out = 256)."""
    return bool((_lib or load()).msda_dino_query_pos_supported(int(width), int(n_frames), int(rows), int(hidden), int(out_features)))


def dino_query_pos_forward(ref2, valid_xy, n_frames, dim_t, w1, b1, w2, b2):
    """(h, y) [M, 256] each: h = relu(pe(ref2) @ w1^T + b1), y = h @ w2^T + b2 — msda_dino_query_pos_forward_f32, one launch."""
    _check_dino_rows("dino_query_pos_forward", ref2, valid_xy, n_frames, dim_t)
    ws, bs = (w1, w2), (b1, b2)
    if not (all(_f32_cuda(w) and tuple(w.shape) == (DINO_PE_WIDTH, DINO_PE_WIDTH) and w.device == ref2.device
                and w.data_ptr() % 16 == 0 for w in ws)
            and all(_f32_cuda(b) and b.numel() == DINO_PE_WIDTH and b.device == ref2.device for b in bs)):
        raise RuntimeError("dino_query_pos_forward: expected contiguous fp32 CUDA weights [256, 256] (16-byte aligned) and biases [256]")
    M, W = ref2.shape
    h = torch.empty((M, DINO_PE_WIDTH), dtype=torch.float32, device=ref2.device)
    y = torch.empty((M, DINO_PE_WIDTH), dtype=torch.float32, device=ref2.device)
    _launch(ref2.device, "msda_dino_query_pos_forward_f32", "dino_query_pos_forward", ref2.data_ptr(), W,
            valid_xy.data_ptr() if valid_xy is not None else None, int(n_frames), M, dim_t.data_ptr(), w1.data_ptr(), b1.data_ptr(),
            w2.data_ptr(), b2.data_ptr(), h.data_ptr(), y.data_ptr())
    return h, y


def dino_refine_forward(ref, cls, delta_key, delta_obj, hand_classes=(12, 13)):
    """(out [..., 42], code [...] uint8) — msda_dino_refine_forward_f32: ref / delta_key / delta_obj [..., 42] and cls [..., K],
    contiguous fp32 CUDA with the same leading shape.  One launch, no host synchronisation."""
    lead = tuple(ref.shape[:-1])
    ts = (ref, cls, delta_key, delta_obj)
    if not (all(_f32_cuda(t) and t.device == ref.device for t in ts) and ref.shape[-1] == 42 and cls.dim() == ref.dim()
            and tuple(cls.shape[:-1]) == lead and cls.shape[-1] > 0
            and tuple(delta_key.shape) == tuple(ref.shape) and tuple(delta_obj.shape) == tuple(ref.shape)):
        raise RuntimeError("dino_refine_forward: expected contiguous fp32 CUDA ref / delta_key / delta_obj [..., 42] and cls [..., K] "
                           "with the same leading shape")
    M = ref.numel() // 42
    out = torch.empty_like(ref)
    code = torch.empty(lead, dtype=torch.uint8, device=ref.device)
    _launch(ref.device, "msda_dino_refine_forward_f32", "dino_refine_forward", ref.data_ptr(), cls.data_ptr(), cls.shape[-1],
            delta_key.data_ptr(), delta_obj.data_ptr(), int(hand_classes[0]), int(hand_classes[1]), M, out.data_ptr(), code.data_ptr())
    return out, code


def dino_refine_backward(grad_out, out, code, want_key=True, want_obj=True):
    """(grad_key, grad_obj) [..., 42] (None where not wanted) — msda_dino_refine_backward_f32."""
    if not (_f32_cuda(grad_out) and _f32_cuda(out) and tuple(grad_out.shape) == tuple(out.shape) and out.shape[-1] == 42
            and code.is_cuda and code.dtype == torch.uint8 and code.is_contiguous() and code.numel() * 42 == out.numel()
            and grad_out.device == out.device == code.device):
        raise RuntimeError("dino_refine_backward: expected contiguous fp32 CUDA grad_out / out [..., 42] and uint8 code [...]")
    gk = torch.empty_like(out) if want_key else None
    go = torch.empty_like(out) if want_obj else None
    _launch(out.device, "msda_dino_refine_backward_f32", "dino_refine_backward", grad_out.data_ptr(), out.data_ptr(), code.data_ptr(),
            code.numel(), gk.data_ptr() if want_key else None, go.data_ptr() if want_obj else None)
    return gk, go


# ---- DINO's two-stage query selection (csrc/msda_dino_select.hip) ------------------------------------------------------------
DINO_SELECT_MAX_FRAMES = 65535                        # frames per call (a grid dimension)


def dino_select_supported(S, K, Q, C):
    """msda_dino_select_supported: 1 <= Q <= min(S, 2048), S <= 2^20, 1 <= K <= 256, C a multiple of 4 in 4..2048."""
    return bool((_lib or load()).msda_dino_select_supported(int(S), int(K), int(Q), int(C)))


def dino_select_workspace_bytes(N, S):
    """msda_dino_select_workspace_bytes: the bytes of scratch one forward of N frames of S rows needs."""
    return int((_lib or load()).msda_dino_select_workspace_bytes(int(N), int(S)))


def dino_select_forward(cls, memory, proposals, num_queries, hand_classes=(12, 13)):
    """(topk [N,Q] int64, slot [N,S] int32, tgt [N,Q,C], prop_sel [N,Q,42], code [N,Q] uint8) — msda_dino_select_forward_f32:
    two launches, no host synchronisation.  Raises RuntimeError when Q exceeds the rows per frame (as torch.topk does)."""
    ts = (cls, memory, proposals)
    if not (all(_f32_cuda(t) and t.dim() == 3 and t.device == cls.device and tuple(t.shape[:2]) == tuple(cls.shape[:2]) for t in ts)
            and proposals.shape[-1] == 42):
        raise RuntimeError("dino_select_forward: expected contiguous fp32 CUDA cls [N,S,K], memory [N,S,C] and proposals [N,S,42]")
    N, S, K = cls.shape
    C, Q = memory.shape[-1], int(num_queries)
    if Q > S:
        raise RuntimeError("selected index k out of range")
    dev = cls.device
    topk = torch.empty((N, Q), dtype=torch.int64, device=dev)
    slot = torch.empty((N, S), dtype=torch.int32, device=dev)
    tgt = torch.empty((N, Q, C), dtype=torch.float32, device=dev)
    prop_sel = torch.empty((N, Q, 42), dtype=torch.float32, device=dev)
    code = torch.empty((N, Q), dtype=torch.uint8, device=dev)
    workspace = torch.empty((max(16, dino_select_workspace_bytes(N, S)),), dtype=torch.uint8, device=dev)
    _launch(dev, "msda_dino_select_forward_f32", "dino_select_forward", cls.data_ptr(), memory.data_ptr(), proposals.data_ptr(),
            N, S, K, Q, C, int(hand_classes[0]), int(hand_classes[1]), topk.data_ptr(), slot.data_ptr(), tgt.data_ptr(),
            prop_sel.data_ptr(), code.data_ptr(), workspace.data_ptr())
    return topk, slot, tgt, prop_sel, code


def dino_select_backward(slot, grad_tgt, out=None):
    """grad_memory [N,S,C] — msda_dino_select_backward_f32: every element written by the one launch (``out``: a buffer to fill)."""
    if not (slot.is_cuda and slot.dtype == torch.int32 and slot.is_contiguous() and slot.dim() == 2 and _f32_cuda(grad_tgt)
            and grad_tgt.dim() == 3 and grad_tgt.shape[0] == slot.shape[0] and grad_tgt.device == slot.device):
        raise RuntimeError("dino_select_backward: expected contiguous CUDA int32 slot [N,S] and fp32 grad_tgt [N,Q,C]")
    N, S = slot.shape
    Q, C = grad_tgt.shape[1], grad_tgt.shape[2]
    if out is None:
        out = torch.empty((N, S, C), dtype=torch.float32, device=slot.device)
    elif not (_f32_cuda(out) and tuple(out.shape) == (N, S, C) and out.device == slot.device):
        raise RuntimeError("dino_select_backward: out must be contiguous fp32 CUDA [N,S,C]")
    _launch(slot.device, "msda_dino_select_backward_f32", "dino_select_backward", slot.data_ptr(), grad_tgt.data_ptr(), N, S, Q, C,
            out.data_ptr())
    return out


# ---- DINO's contrastive-denoising queries (csrc/msda_cdn.hip) --------------------------------------------------------------
def cdn_supported(hidden, width, rows_book, E):
    """msda_cdn_supported: hidden a multiple of 4 in 4..1024, width 1..64, every draw counter of E flat elements below 2^32."""
    return bool((_lib or load()).msda_cdn_supported(int(hidden), int(width), int(rows_book), int(E)))


def cdn_flip_threshold(label_noise_ratio):
    """The 32-bit threshold of the label draw: a label is replaced iff its hash is below min(2^32 - 1, floor(ratio * 0.5 * 2^32))
    (dn_components.py:76, ``p < label_noise_ratio * 0.5``); 0 = nothing is drawn."""
    return int(min(4294967295.0, max(0.0, float(label_noise_ratio) * 0.5 * 4294967296.0)))


def cdn_prepare_forward(labels, offsets, keypoints, weight, seed, single_pad, groups, num_classes, flip_threshold=0,
                        key_noise_scale=0.0, key_debug=False):
    """(input_query_label [B, pad, H], input_query_key [B, pad, W], noised_labels [B, pad] int32[, key' [B, pad, W]]) —
    msda_cdn_prepare_forward_f32, one launch (none when pad == 0): labels [T] / offsets [B + 1] int64, keypoints [T, W] and
    weight [rows, H] contiguous fp32 CUDA, seed a one-element int64 CUDA tensor or None when nothing is drawn; single_pad, groups
    (after the reference's division) and num_classes host ints.  ``key_debug``: also the noised, clamped keys before
    inverse_sigmoid (tests)."""
    dev = weight.device
    if not (_f32_cuda(weight) and weight.dim() == 2 and _f32_cuda(keypoints) and keypoints.dim() == 2 and keypoints.device == dev
            and all(t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 1 and t.device == dev
                    for t in (labels, offsets))
            and labels.shape[0] == keypoints.shape[0] and offsets.shape[0] >= 1
            and (seed is None or (seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1 and seed.device == dev))):
        raise RuntimeError("cdn_prepare_forward: expected int64 CUDA labels [T] / offsets [B + 1], contiguous fp32 CUDA keypoints "
                           "[T, W] and weight [rows, H], and a one-element int64 CUDA seed or None, on one device")
    B, T, W = offsets.shape[0] - 1, labels.shape[0], keypoints.shape[1]
    rows_book, H = weight.shape
    pad = 2 * int(single_pad) * int(groups)
    out_l = torch.empty((B, pad, H), dtype=torch.float32, device=dev)
    out_k = torch.empty((B, pad, W), dtype=torch.float32, device=dev)
    noised = torch.empty((B, pad), dtype=torch.int32, device=dev)
    dbg = torch.empty((B, pad, W), dtype=torch.float32, device=dev) if key_debug else None
    _launch(dev, "msda_cdn_prepare_forward_f32", "cdn_prepare_forward", labels.data_ptr(), offsets.data_ptr(), keypoints.data_ptr(),
            weight.data_ptr(), seed.data_ptr() if seed is not None else None, B, T, W, H, rows_book, int(single_pad), int(groups),
            int(num_classes), int(flip_threshold), float(key_noise_scale), out_l.data_ptr(), out_k.data_ptr(), noised.data_ptr(),
            dbg.data_ptr() if key_debug else None)
    return (out_l, out_k, noised, dbg) if key_debug else (out_l, out_k, noised)


def cdn_prepare_backward(grad_label, noised, rows_book):
    """grad_weight [rows_book, H] of the label embedding — msda_cdn_prepare_backward_f32: one launch, fixed summation order."""
    if not (_f32_cuda(grad_label) and grad_label.dim() == 3 and noised.is_cuda and noised.dtype == torch.int32
            and noised.is_contiguous() and tuple(noised.shape) == tuple(grad_label.shape[:2]) and noised.device == grad_label.device):
        raise RuntimeError("cdn_prepare_backward: expected contiguous fp32 CUDA grad_label [B, pad, H] and int32 noised_labels [B, pad]")
    H = grad_label.shape[2]
    gw = torch.empty((int(rows_book), H), dtype=torch.float32, device=grad_label.device)
    _launch(grad_label.device, "msda_cdn_prepare_backward_f32", "cdn_prepare_backward", grad_label.data_ptr(), noised.data_ptr(),
            noised.numel(), H, int(rows_book), gw.data_ptr())
    return gw


# ---- the Hungarian matchers (csrc/msda_matcher.hip) ----------------------------------------------------------------------
MATCH_MAX_QUERIES, MATCH_MAX_TARGETS, MATCH_MAX_SETS, MATCH_MAX_DIM = 1024, 16, 16, 64
MATCH_OK, MATCH_INVALID, MATCH_INFEASIBLE, MATCH_BAD_LABEL, MATCH_BAD_TARGETS = 0, 1, 2, 3, 4


def _ptr_array(ts):
    return (_VP * len(ts))(*[t.data_ptr() for t in ts])


def match_layout(sets, bs, t_max):
    """(numel, slices) of the matchers' int64 result (include/msda.h; MatchView in csrc/msda_set_args.h): the slices of
    query_idx and target_idx [sets, bs, t_max], count and status [sets, bs] and the valid-frame count [1]."""
    n, W = sets * bs, int(t_max)
    t, c, s, v = n * W, 2 * n * W, 2 * n * W + n, 2 * n * W + 2 * n
    return v + 1, (slice(0, t), slice(t, c), slice(c, s), slice(s, v), slice(v, v + 1))


def match_views(buffer, sets, bs, t_max):
    """(query_idx, target_idx, count, status, num_valid []) views of a result buffer, shaped as ``match_layout`` says."""
    q, t, count, status, nvalid = match_layout(sets, bs, t_max)[1]
    return (buffer[q].view(sets, bs, t_max), buffer[t].view(sets, bs, t_max), buffer[count].view(sets, bs),
            buffer[status].view(sets, bs), buffer[nvalid.start])


def _pred_sets_check(what, logits, heads, D, per_set_q=False, sets_ok=True):
    """Per-set lists of fp32 CUDA pred_logits [bs, Q, K] and, per keypoint head of ``heads``, [bs, Q, D] on one device;
    ``per_set_q`` (DINO): the sets may differ in Q.  Returns (dev, bs, the sets' Q, K)."""
    sets = len(logits)
    if not (0 < sets <= MATCH_MAX_SETS and all(len(h) == sets for h in heads) and sets_ok):
        raise RuntimeError("%s: 1 to %d prediction sets%s" % (what, MATCH_MAX_SETS,
                                                              ", one match_set entry each" if per_set_q else ""))
    dev, shapes, q = logits[0].device, [tuple(t.shape) for t in logits], "Q_s" if per_set_q else "Q"
    first = shapes[0] if len(shapes[0]) == 3 else None
    if first is None or not all(_f32_cuda(t) and t.device == dev
                                and (s == first or (per_set_q and len(s) == 3 and s[::2] == first[::2]))
                                for t, s in zip(logits, shapes)):
        raise RuntimeError("%s: expected contiguous fp32 CUDA pred_logits [bs, %s, K]%s in every set"
                           % (what, q, "" if per_set_q else " of one shape"))
    want = [s[:2] + (D,) for s in shapes]
    for h in heads:
        if not all(_f32_cuda(t) and t.device == dev and tuple(t.shape) == w for t, w in zip(h, want)):
            raise RuntimeError("%s: expected contiguous fp32 CUDA keypoint heads [bs, %s, %d]" % (what, q, D))
    return dev, first[0], [s[1] for s in shapes], first[2]


def _set_targets_check(what, dev, bs, labels, keypoints, offsets, t_max=None):
    """One step's targets on ``dev``; ``t_max`` for the callers that bound it here (is_valid: ``_is_valid_check``)."""
    if not (labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous() and labels.dim() == 1
            and offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous()
            and tuple(offsets.shape) == (bs + 1,) and labels.device == dev and offsets.device == dev):
        raise RuntimeError("%s: expected int64 CUDA labels [n] and offsets [bs + 1]" % what)
    if keypoints is not None and not (_f32_cuda(keypoints) and keypoints.dim() == 2 and keypoints.device == dev
                                      and keypoints.shape[0] == labels.shape[0]):
        raise RuntimeError("%s: expected contiguous fp32 CUDA target keypoints [n, D]" % what)
    if t_max is not None and not 0 <= int(t_max) <= MATCH_MAX_TARGETS:
        raise RuntimeError("%s: at most %d targets per frame" % (what, MATCH_MAX_TARGETS))


def _is_valid_check(what, dev, bs, is_valid):
    if not (torch.is_tensor(is_valid) and is_valid.is_cuda and is_valid.dtype == torch.int32 and is_valid.is_contiguous()
            and tuple(is_valid.shape) == (bs,) and is_valid.device == dev):
        raise RuntimeError("%s: expected int32 CUDA is_valid [bs]" % what)


def _match_buffer_check(what, dev, match, sets, bs, t_max):
    if not (match is not None and match.is_cuda and match.dtype == torch.int64 and match.is_contiguous()
            and match.device == dev and 0 <= int(t_max) <= MATCH_MAX_TARGETS
            and match.numel() == match_layout(sets, bs, t_max)[0]):
        raise RuntimeError("%s: expected the matcher's int64 CUDA result for %d sets" % (what, sets))


def _num_boxes_check(what, dev, num_boxes):
    if not (_f32_cuda(num_boxes) and num_boxes.numel() == 1 and num_boxes.device == dev):
        raise RuntimeError("%s: expected an fp32 CUDA num_boxes scalar" % what)


def _match_out(dev, sets, bs, t_max, Q, cost_debug):
    out = torch.empty(match_layout(sets, bs, t_max)[0], dtype=torch.int64, device=dev)
    if cost_debug is not None and not (_f32_cuda(cost_debug) and cost_debug.device == dev
                                       and tuple(cost_debug.shape) == (sets, bs, Q, t_max)):
        raise RuntimeError("match: cost_debug must be contiguous fp32 CUDA [sets, bs, Q, t_max]")
    return out


def match_arctic(logits, hand, obj, labels, keypoints, offsets, is_valid, t_max, cost_class, cost_keypoint, cost_debug=None):
    """The int64 result buffer of msda_match_arctic_f32 (include/msda.h): lists of per-set pred_logits [bs, Q, K] and (with
    target keypoints) pred_hand_key / pred_obj_key [bs, Q, D]; labels [n] / offsets [bs + 1] int64, keypoints [n, D] fp32 or
    None, is_valid [bs] int32 on the same device.  One launch, no host synchronisation."""
    heads = (hand, obj) if keypoints is not None else ()
    D = keypoints.shape[1] if keypoints is not None else 0
    dev, bs, (Q, *_), K = _pred_sets_check("match_arctic", logits, heads, D)
    _set_targets_check("match_arctic", dev, bs, labels, keypoints, offsets, t_max)
    _is_valid_check("match_arctic", dev, bs, is_valid)
    sets = len(logits)
    out = _match_out(dev, sets, bs, t_max, Q, cost_debug)
    _launch(dev, "msda_match_arctic_f32", "match_arctic", _ptr_array(logits), _ptr_array(hand) if heads else None,
            _ptr_array(obj) if heads else None, sets, bs, Q, K, D, labels.data_ptr(),
            keypoints.data_ptr() if keypoints is not None else None, offsets.data_ptr(), labels.shape[0],
            is_valid.data_ptr(), int(t_max), float(cost_class), float(cost_keypoint), out.data_ptr(),
            cost_debug.data_ptr() if cost_debug is not None else None)
    return out


def match_assembly(logits, pred_keypoints, labels, keypoints, offsets, t_max, cost_class, cost_keypoint, cost_debug=None):
    """The int64 result buffer of msda_match_assembly_f32: as match_arctic with one keypoint head per set and no is_valid."""
    D = keypoints.shape[1]
    dev, bs, (Q, *_), K = _pred_sets_check("match_assembly", logits, (pred_keypoints,), D)
    _set_targets_check("match_assembly", dev, bs, labels, keypoints, offsets, t_max)
    sets = len(logits)
    out = _match_out(dev, sets, bs, t_max, Q, cost_debug)
    _launch(dev, "msda_match_assembly_f32", "match_assembly", _ptr_array(logits), _ptr_array(pred_keypoints), sets, bs, Q, K,
            D, labels.data_ptr(), keypoints.data_ptr(), offsets.data_ptr(), labels.shape[0], int(t_max), float(cost_class),
            float(cost_keypoint), out.data_ptr(), cost_debug.data_ptr() if cost_debug is not None else None)
    return out


def lsap(cost):
    """(query_idx [B, W], target_idx [B, W], count [B], status [B]) int64 — msda_lsap_f32: scipy's linear_sum_assignment of
    each [Q, T] block of a contiguous fp32 CUDA cost [B, Q, T] (min(Q, T) <= 16, max(Q, T) <= 1024), W = min(Q, T)."""
    if not (_f32_cuda(cost) and cost.dim() == 3):
        raise RuntimeError("lsap: expected a contiguous fp32 CUDA cost [B, Q, T]")
    B, Q, T = cost.shape
    W = min(Q, T)
    numel, slices = match_layout(B, 1, W)                 # B one-frame sets, without the trailing valid-frame count
    out = torch.empty(numel - 1, dtype=torch.int64, device=cost.device)
    _launch(cost.device, "msda_lsap_f32", "lsap", cost.data_ptr(), B, Q, T, out.data_ptr())
    qi, ti, count, status = (out[sl] for sl in slices[:4])
    return qi.view(B, W), ti.view(B, W), count, status


# ---- the set criteria's matched losses (csrc/msda_criterion.hip) ---------------------------------------------------------
CRIT_ARCTIC, CRIT_ASSEMBLY = 0, 1
CRIT_TERMS = 4
CRIT_BAD_LABEL, CRIT_BAD_TARGETS, CRIT_MASK_MISMATCH, CRIT_MATCH_STATUS = 1, 2, 4, 8


def _crit_common(kind, logits, hand, obj, match, t_max, labels, keypoints, offsets, is_valid, joint_valid, hand_mask,
                 num_boxes, focal_alpha):
    """Checks shared by criterion_fwd / criterion_bwd; returns the C arguments in order and (dev, bs, Q, K, D)."""
    arctic = kind == CRIT_ARCTIC
    heads = ((hand, obj) if arctic else (hand,)) if keypoints is not None else ()
    D = keypoints.shape[1] if keypoints is not None else 0
    dev, bs, (Q, *_), K = _pred_sets_check("criterion", logits, heads, D)
    _set_targets_check("criterion", dev, bs, labels, keypoints, offsets, t_max)
    sets = len(logits)
    _match_buffer_check("criterion", dev, match, sets, bs, t_max)
    if arctic:
        _is_valid_check("criterion", dev, bs, is_valid)
    jv_needed = not arctic and keypoints is not None
    if jv_needed and not (joint_valid is not None and joint_valid.is_cuda and joint_valid.dtype == torch.uint8
                          and joint_valid.is_contiguous() and tuple(joint_valid.shape) == (labels.shape[0], D)
                          and joint_valid.device == dev):
        raise RuntimeError("criterion: expected uint8 CUDA joint_valid [n, %d]" % D)
    _num_boxes_check("criterion", dev, num_boxes)
    args = [kind, _ptr_array(logits), _ptr_array(hand) if heads else None, _ptr_array(obj) if heads and arctic else None,
            sets, bs, Q, K, D, match.data_ptr(), int(t_max), labels.data_ptr(),
            keypoints.data_ptr() if keypoints is not None else None, offsets.data_ptr(), labels.shape[0],
            is_valid.data_ptr() if arctic else None, joint_valid.data_ptr() if jv_needed else None, int(hand_mask),
            num_boxes.data_ptr(), float(focal_alpha)]
    return args, (dev, bs, Q, K, D)


def _set_grads(what, dev, bs, queries, K, D, want_obj, grad_losses, stats, out=None):
    """Checks a backward entry's ``grad_losses`` and ``stats``; returns the (grad_logits, grad_hand, grad_obj) lists shaped
    as the predictions (``out``'s when given) and the entry's trailing C arguments."""
    sets = len(queries)
    if not (_f32_cuda(grad_losses) and tuple(grad_losses.shape) == (sets, CRIT_TERMS) and grad_losses.device == dev
            and stats.is_cuda and stats.dtype == torch.int32 and tuple(stats.shape) == (sets, 4) and stats.is_contiguous()):
        raise RuntimeError("%s: expected fp32 grad_losses and int32 stats [%d, 4]" % (what, sets))
    n_hand, n_obj = (sets if D else 0), (sets if D and want_obj else 0)
    want = [(bs, q, K) for q in queries] + [(bs, q, D) for q in queries[:n_hand]] + [(bs, q, D) for q in queries[:n_obj]]
    if out is not None:
        g_logits, g_hand, g_obj = (list(g) for g in out)
        if not (len(g_logits) == sets and len(g_hand) == n_hand and len(g_obj) == n_obj
                and all(_f32_cuda(t) and t.device == dev and tuple(t.shape) == w
                        for t, w in zip(g_logits + g_hand + g_obj, want))):
            raise RuntimeError("%s: out must hold contiguous fp32 CUDA tensors shaped as the predictions" % what)
    else:
        flat = [torch.empty(w, dtype=torch.float32, device=dev) for w in want]
        g_logits, g_hand, g_obj = flat[:sets], flat[sets:sets + n_hand], flat[sets + n_hand:]
    args = [grad_losses.data_ptr(), stats.data_ptr(), _ptr_array(g_logits), _ptr_array(g_hand) if g_hand else None,
            _ptr_array(g_obj) if g_obj else None]
    return (g_logits, g_hand, g_obj), args


def criterion_fwd(kind, logits, hand, obj, match, t_max, labels, keypoints, offsets, is_valid, joint_valid, hand_mask,
                  num_boxes, focal_alpha):
    """(losses fp32 [sets, 4], stats int32 [sets, 4]) — msda_criterion_fwd_f32 (include/msda.h).  One launch, no host
    synchronisation."""
    args, (dev, *_rest) = _crit_common(kind, logits, hand, obj, match, t_max, labels, keypoints, offsets, is_valid,
                                       joint_valid, hand_mask, num_boxes, focal_alpha)
    losses = torch.empty(len(logits), CRIT_TERMS, dtype=torch.float32, device=dev)
    stats = torch.empty(len(logits), 4, dtype=torch.int32, device=dev)
    _launch(dev, "msda_criterion_fwd_f32", "criterion_fwd", *args, losses.data_ptr(), stats.data_ptr())
    return losses, stats


def criterion_bwd(kind, logits, hand, obj, match, t_max, labels, keypoints, offsets, is_valid, joint_valid, hand_mask,
                  num_boxes, focal_alpha, grad_losses, stats):
    """(grad_logits, grad_hand, grad_obj) lists, every element written — msda_criterion_bwd_f32.  One launch."""
    args, (dev, bs, Q, K, D) = _crit_common(kind, logits, hand, obj, match, t_max, labels, keypoints, offsets, is_valid,
                                            joint_valid, hand_mask, num_boxes, focal_alpha)
    grads, g_args = _set_grads("criterion_bwd", dev, bs, [Q] * len(logits), K, D, kind == CRIT_ARCTIC, grad_losses, stats)
    _launch(dev, "msda_criterion_bwd_f32", "criterion_bwd", *args, *g_args)
    return grads


# ---- the DINO criterion's matched and denoising losses (csrc/msda_criterion_dino.hip) -----------------------------------
CRIT_DINO_CHUNK_ROWS, CRIT_DINO_PARTIAL_BYTES = 256, 64     # MSDA_CRITERION_DINO_* (include/msda.h)


def criterion_dino_workspace_bytes(bs, queries):
    """The forward's workspace (include/msda.h): one record per chunk of every set."""
    return CRIT_DINO_PARTIAL_BYTES * sum(bs * ((q + CRIT_DINO_CHUNK_ROWS - 1) // CRIT_DINO_CHUNK_ROWS) for q in queries)


def _crit_dino_common(logits, hand, obj, match_set, match, match_sets, t_max, labels, keypoints, offsets, is_valid,
                      hand_mask, num_boxes, focal_alpha, single_pad, groups):
    """Checks shared by criterion_dino_fwd / criterion_dino_bwd; returns the C arguments in order, the tensors' device and
    (bs, K, D) and the sets' query counts.  ``match_set[s]``: the set's index in the matcher's result ``match`` (of
    ``match_sets`` sets), -1 for a denoising set."""
    sets, has_kp = len(logits), keypoints is not None
    D = keypoints.shape[1] if has_kp else 0
    dev, bs, queries, K = _pred_sets_check("criterion_dino", logits, (hand, obj) if has_kp else (), D, per_set_q=True,
                                           sets_ok=len(match_set) == sets)
    _set_targets_check("criterion_dino", dev, bs, labels, keypoints, offsets)
    if any(m >= 0 for m in match_set):
        _match_buffer_check("criterion_dino", dev, match, match_sets, bs, t_max)
    _is_valid_check("criterion_dino", dev, bs, is_valid)
    _num_boxes_check("criterion_dino", dev, num_boxes)
    ints = ctypes.c_int * sets
    args = [_ptr_array(logits), _ptr_array(hand) if has_kp else None, _ptr_array(obj) if has_kp else None, ints(*queries),
            ints(*[int(m) for m in match_set]), sets, bs, K, D, int(single_pad), int(groups),
            match.data_ptr() if match is not None else None, int(match_sets), int(t_max), labels.data_ptr(),
            keypoints.data_ptr() if has_kp else None, offsets.data_ptr(), labels.shape[0], is_valid.data_ptr(),
            int(hand_mask), num_boxes.data_ptr(), float(focal_alpha)]
    return args, dev, (bs, K, D), queries


def criterion_dino_fwd(logits, hand, obj, match_set, match, match_sets, t_max, labels, keypoints, offsets, is_valid, hand_mask,
                       num_boxes, focal_alpha, single_pad, groups):
    """(losses fp32 [sets, 4], stats int32 [sets, 4]) — msda_criterion_dino_fwd_f32 (include/msda.h).  Two launches, no host
    synchronisation."""
    args, dev, (bs, _K, _D), queries = _crit_dino_common(logits, hand, obj, match_set, match, match_sets, t_max, labels,
                                                         keypoints, offsets, is_valid, hand_mask, num_boxes, focal_alpha,
                                                         single_pad, groups)
    nbytes = criterion_dino_workspace_bytes(bs, queries)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    losses = torch.empty(len(logits), CRIT_TERMS, dtype=torch.float32, device=dev)
    stats = torch.empty(len(logits), 4, dtype=torch.int32, device=dev)
    _launch(dev, "msda_criterion_dino_fwd_f32", "criterion_dino_fwd", *args, ws.data_ptr(), nbytes, losses.data_ptr(),
            stats.data_ptr())
    return losses, stats


def criterion_dino_bwd(logits, hand, obj, match_set, match, match_sets, t_max, labels, keypoints, offsets, is_valid, hand_mask,
                       num_boxes, focal_alpha, single_pad, groups, grad_losses, stats, out=None):
    """(grad_logits, grad_hand, grad_obj) lists, every element written — msda_criterion_dino_bwd_f32.  One launch.  ``out``
    (tests): the three lists, already allocated in the predictions' shapes."""
    args, dev, (bs, K, D), queries = _crit_dino_common(logits, hand, obj, match_set, match, match_sets, t_max, labels,
                                                       keypoints, offsets, is_valid, hand_mask, num_boxes, focal_alpha,
                                                       single_pad, groups)
    grads, g_args = _set_grads("criterion_dino_bwd", dev, bs, queries, K, D, True, grad_losses, stats, out)
    _launch(dev, "msda_criterion_dino_bwd_f32", "criterion_dino_bwd", *args, *g_args)
    return grads


# ---- the layers' FFN under bf16 autocast (csrc/msda_ffn_bf16.hip) ------------------------------------------------------------
def ffn_bf16_supported(C, F):
    """msda_ffn_bf16_supported (include/msda.h): 1 when the bf16-autocast FFN kernels take model width C and hidden width F."""
    return bool((_lib or load()).msda_ffn_bf16_supported(int(C), int(F)))


def ffn_bf16_workspace_bytes(M, C, F):
    """msda_ffn_bf16_workspace_bytes (include/msda.h): the backward's workspace; 0 for sizes the entries refuse."""
    return int((_lib or load()).msda_ffn_bf16_workspace_bytes(int(M), int(C), int(F)))


def ffn_forward_bf16(x2, w1, b1, w2, b2, p=0.0, seed=None):
    """msda_ffn_forward_bf16 (include/msda.h): the FFN of x2 [M, C] (contiguous fp32 or bf16) in ONE launch.  p > 0 needs a
    one-element int64 CUDA ``seed``.  Returns (xb, a, y): x2 as bf16 (x2 itself when it is bf16), a [M, F] and y [M, C], bf16."""
    M, C = x2.shape
    F = w1.shape[0]
    bf = x2.dtype == torch.bfloat16
    if p > 0 and not (torch.is_tensor(seed) and seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1):
        raise RuntimeError("ffn_forward_bf16: dropout needs a one-element int64 CUDA seed tensor")
    xb = x2 if bf else torch.empty((M, C), dtype=torch.bfloat16, device=x2.device)
    a = torch.empty((M, F), dtype=torch.bfloat16, device=x2.device)
    y = torch.empty((M, C), dtype=torch.bfloat16, device=x2.device)
    _launch(x2.device, "msda_ffn_forward_bf16", "ffn_forward_bf16", M, C, F, x2.data_ptr(), int(bf), w1.data_ptr(), b1.data_ptr(),
            w2.data_ptr(), b2.data_ptr(), float(p), seed.data_ptr() if p > 0 else None, None if bf else xb.data_ptr(),
            a.data_ptr(), y.data_ptr())
    return xb, a, y


def ffn_backward_bf16(go2, xb, a, w1, w2, p, x_dtype, need_x, need_w1, need_b1, need_w2, need_b2):
    """msda_ffn_backward_bf16 (include/msda.h): (gx, gw1, gb1, gw2, gb2) of the node, None where not needed; gx [M, C] in
    ``x_dtype``, the parameter gradients fp32.  At most 5 launches: gh, gx, two weight-gradient first stages, one second
    stage; a gradient that is not needed costs none (a bias gradient alone still computes its weight gradient)."""
    M, C = xb.shape
    F = a.shape[1]
    dev, f32 = xb.device, torch.float32
    w1g, w2g = need_w1 or need_b1, need_w2 or need_b2
    gx = torch.empty((M, C), dtype=x_dtype, device=dev) if need_x else None
    gw1 = torch.empty((F, C), dtype=f32, device=dev) if w1g else None
    gb1 = torch.empty((F,), dtype=f32, device=dev) if need_b1 else None
    gw2 = torch.empty((C, F), dtype=f32, device=dev) if w2g else None
    gb2 = torch.empty((C,), dtype=f32, device=dev) if need_b2 else None
    nbytes = ffn_bf16_workspace_bytes(M, C, F)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _launch(dev, "msda_ffn_backward_bf16", "ffn_backward_bf16", M, C, F, go2.data_ptr(), xb.data_ptr(), a.data_ptr(),
            w1.data_ptr(), w2.data_ptr(), float(p), ptr(gx), int(x_dtype == torch.bfloat16), ptr(gw1), ptr(gb1), ptr(gw2),
            ptr(gb2), ws.data_ptr(), nbytes)
    return gx, (gw1 if need_w1 else None), gb1, (gw2 if need_w2 else None), gb2


# ---- the DeformableDETR prediction heads, fp32 and bf16 autocast (csrc/msda_heads.hip, csrc/msda_heads_bf16.hip) ------------
HEADS_ARCTIC, HEADS_ASSEMBLY = 0, 1
HEADS_SHARED_CLS, HEADS_SHARED_MLP = 1, 2
HEADS_SHARED_WIDTHS = (48, 10, 3, 3, 3, 1)


def heads_supported(C):
    """msda_heads_supported (include/msda.h): 1 when the heads kernels take hidden size C."""
    return bool((_lib or load()).msda_heads_supported(int(C)))


def heads_bf16_supported(C):
    """msda_heads_bf16_supported (include/msda.h): 1 when the bf16-autocast heads kernels take hidden size C."""
    return bool((_lib or load()).msda_heads_bf16_supported(int(C)))


# The two forms of the heads entries: the C names, and the dtypes of what differs between them (hidden and the shared outputs;
# logits and keypoints by kind).  hs, the parameters, the references, sig and every parameter gradient are fp32 in both.
_BF = torch.bfloat16
_HEADS_FORMS = {
    "f32": dict(suffix="_f32", label="", ws="msda_heads_workspace_bytes", hidden=torch.float32,
                out=(torch.float32, torch.float32), grads="contiguous fp32 CUDA output gradients"),
    "bf16": dict(suffix="_bf16", label="_bf16", ws="msda_heads_bf16_workspace_bytes", hidden=_BF, out=(torch.float32, _BF),
                 grads="contiguous CUDA output gradients of the outputs' dtypes"),
}


def _heads_workspace_bytes(form, kind, L, M, C, K, n_mlp, flags):
    entry = getattr(_lib or load(), _HEADS_FORMS[form]["ws"])
    return int(entry(int(kind), int(L), int(M), int(C), int(K), int(n_mlp), int(flags)))


def _ptrs_or_none(ts):
    return _ptr_array(ts) if ts else None


def _heads_common(kind, hs, init_ref, inter_ref, cls, mlp, shared, flags):
    """hs [L, M, C]; cls = (weights, biases); mlp = (weights, biases) in (head, layer, level) order; shared likewise."""
    L, M, C = hs.shape
    K = cls[0][0].shape[0]
    n_mlp = len(mlp[0]) // (3 * (1 if flags & HEADS_SHARED_MLP else L)) if mlp[0] else 0
    R = init_ref.shape[-1] if init_ref is not None else 0
    tensors = [hs] + list(cls[0]) + list(cls[1]) + list(mlp[0]) + list(mlp[1]) + list(shared[0]) + list(shared[1])
    tensors += [t for t in (init_ref, inter_ref) if t is not None]
    _check_f32("detr_heads", hs.device, tensors)
    return [int(kind), int(L), int(M), int(C), int(K), int(n_mlp), int(R), int(flags), hs.data_ptr(),
            init_ref.data_ptr() if init_ref is not None else None, inter_ref.data_ptr() if inter_ref is not None else None,
            _ptr_array(cls[0]), _ptr_array(cls[1]), _ptrs_or_none(mlp[0]), _ptrs_or_none(mlp[1]), _ptrs_or_none(shared[0]),
            _ptrs_or_none(shared[1])], (L, M, C, K, n_mlp)


def _heads_forward(form, kind, hs, init_ref, inter_ref, cls, mlp, shared, flags):
    f = _HEADS_FORMS[form]
    args, (L, M, C, K, n_mlp) = _heads_common(kind, hs, init_ref, inter_ref, cls, mlp, shared, flags)
    D = 42 if kind == HEADS_ARCTIC else 63
    dev, out_dt = hs.device, f["out"][kind == HEADS_ASSEMBLY]
    logits = torch.empty(L, M, K, dtype=out_dt, device=dev)
    kp = [torch.empty(L, M, D, dtype=out_dt, device=dev) for _ in range(n_mlp)]
    sh = [torch.empty(L, M, n, dtype=f["hidden"], device=dev) for n in HEADS_SHARED_WIDTHS] if shared[0] else []
    hidden = torch.empty(n_mlp, 2, L, M, C, dtype=f["hidden"], device=dev)
    sig = torch.empty(n_mlp, L, M, D, dtype=torch.float32, device=dev)
    _launch(dev, "msda_heads_forward" + f["suffix"], "heads_forward" + f["label"], *args, logits.data_ptr(), _ptrs_or_none(kp),
            _ptrs_or_none(sh), hidden.data_ptr() if n_mlp else None, sig.data_ptr() if n_mlp else None)
    return logits, kp, sh, hidden, sig


def _heads_backward(form, kind, hs, init_ref, inter_ref, cls, mlp, shared, flags, hidden, sig, grad_logits, grad_kp, grad_shared):
    f = _HEADS_FORMS[form]
    args, (L, M, C, K, n_mlp) = _heads_common(kind, hs, init_ref, inter_ref, cls, mlp, shared, flags)
    dev, out_dt = hs.device, f["out"][kind == HEADS_ASSEMBLY]
    typed = [(grad_logits, out_dt)] + [(t, out_dt) for t in grad_kp] + [(t, f["hidden"]) for t in list(grad_shared) + [hidden]]
    if not all(t.is_cuda and t.dtype == dt and t.is_contiguous() and t.device == dev for t, dt in typed):
        raise RuntimeError("detr_heads: expected " + f["grads"])
    ws_bytes = _heads_workspace_bytes(form, kind, L, M, C, K, n_mlp, flags)
    ws = torch.empty(max(1, (ws_bytes + 3) // 4), dtype=torch.float32, device=dev)
    grad_hs = torch.empty_like(hs)
    g_cls = ([torch.empty_like(w) for w in cls[0]], [torch.empty_like(b) for b in cls[1]])
    g_mlp = ([torch.empty_like(w) for w in mlp[0]], [torch.empty_like(b) for b in mlp[1]])
    g_sh = ([torch.empty_like(w) for w in shared[0]], [torch.empty_like(b) for b in shared[1]])
    _launch(dev, "msda_heads_backward" + f["suffix"], "heads_backward" + f["label"], *args, hidden.data_ptr() if n_mlp else None,
            sig.data_ptr() if n_mlp else None, grad_logits.data_ptr(), _ptrs_or_none(grad_kp), _ptrs_or_none(grad_shared),
            grad_hs.data_ptr(), _ptr_array(g_cls[0]), _ptr_array(g_cls[1]), _ptrs_or_none(g_mlp[0]), _ptrs_or_none(g_mlp[1]),
            _ptrs_or_none(g_sh[0]), _ptrs_or_none(g_sh[1]), ws.data_ptr(), ws.numel() * 4)
    return grad_hs, g_cls, g_mlp, g_sh


def heads_workspace_bytes(kind, L, M, C, K, n_mlp, flags):
    return _heads_workspace_bytes("f32", kind, L, M, C, K, n_mlp, flags)


def heads_bf16_workspace_bytes(kind, L, M, C, K, n_mlp, flags):
    return _heads_workspace_bytes("bf16", kind, L, M, C, K, n_mlp, flags)


def heads_forward(*args):
    """msda_heads_forward_f32(kind, hs, init_ref, inter_ref, cls, mlp, shared, flags): (logits [L, M, K], kp outputs [L, M, D]
    per MLP head, shared outputs [L, M, n_g], hidden [n_mlp, 2, L, M, C], sig [n_mlp, L, M, D]), all fp32.  At most 3 launches,
    no host synchronisation."""
    return _heads_forward("f32", *args)


def heads_backward(*args):
    """msda_heads_backward_f32(kind, hs, init_ref, inter_ref, cls, mlp, shared, flags, hidden, sig, grad_logits, grad_kp,
    grad_shared): (grad_hs, grad cls weights / biases, grad MLP weights / biases, grad shared weights / biases), every element
    written.  At most 5 launches, no host synchronisation."""
    return _heads_backward("f32", *args)


def heads_forward_bf16(*args):
    """msda_heads_forward_bf16: heads_forward under bf16 autocast from fp32 hs / parameters / references, with autocast's
    dtypes: logits and keypoints fp32 (ARCTIC) or bf16 (AssemblyHands), shared outputs and hidden bf16, sig fp32."""
    return _heads_forward("bf16", *args)


def heads_backward_bf16(*args):
    """msda_heads_backward_bf16: heads_backward for that form; the parameter gradients and grad_hs are fp32, the output
    gradients carry the outputs' dtypes."""
    return _heads_backward("bf16", *args)


def heads_ref_backward(init_ref, inter_ref, sig, grad_kp, want_init=True, want_inter=True):
    """msda_heads_ref_backward_f32 (include/msda.h): the gradients of the ARCTIC keypoint epilogue with respect to its
    references, from the forward's saved sig [2, L, M, 42] and the two keypoint gradients [L, M, 42].  Returns
    (grad_init_ref [M, 42] or None, grad_inter_ref [L - 1, M, 42] or None); nothing of a level that is not wanted is read.
    One launch, no host synchronisation."""
    n_mlp, L, M, R = sig.shape
    want_inter = bool(want_inter) and L > 1
    tensors = [sig] + list(grad_kp) + ([init_ref] if want_init else []) + ([inter_ref] if want_inter else [])
    _check_f32("dino_heads", sig.device, tensors)
    if len(grad_kp) != n_mlp or any(tuple(g.shape) != (L, M, R) for g in grad_kp):
        raise RuntimeError("dino_heads: expected one keypoint gradient [L, M, R] per head")
    if (want_init and tuple(init_ref.shape) != (M, R)) or (want_inter and tuple(inter_ref.shape) != (L - 1, M, R)):
        raise RuntimeError("dino_heads: expected init_ref [M, R] and inter_ref [L - 1, M, R]")
    g_init = torch.empty_like(init_ref) if want_init else None
    g_inter = torch.empty_like(inter_ref) if want_inter else None
    _launch(sig.device, "msda_heads_ref_backward_f32", "heads_ref_backward", int(L), int(M), int(n_mlp), int(R),
            init_ref.data_ptr() if want_init else None, inter_ref.data_ptr() if want_inter else None, sig.data_ptr(),
            _ptr_array(grad_kp), g_init.data_ptr() if want_init else None, g_inter.data_ptr() if want_inter else None)
    return g_init, g_inter


# ---- SmoothNet: MotionSmoother modules and get_arctic_item's selection (msda_smoother.hip, msda_arctic_item.hip) ----------
SMOOTHER_MAX_MODULES, SMOOTHER_MAX_CALLS, SMOOTHER_MAX_CALLS_PER_MODULE = 6, 12, 4


def smoother_supported(T, O, H, R, num_blocks):
    """msda_smoother_supported (include/msda.h): 1 when the smoother kernels take this geometry."""
    return bool((_lib or load()).msda_smoother_supported(int(T), int(O), int(H), int(R), int(num_blocks)))


def _int_array(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _smoother_geo(dims, n_mod, call_mod, call_B, call_C):
    T, O, H, R, nb = dims
    return [int(T), int(O), int(H), int(R), int(nb), int(n_mod), len(call_mod), _int_array(call_mod), _int_array(call_B),
            _int_array(call_C)]


def smoother_workspace_bytes(dims, n_mod, call_mod, call_B, call_C, which):
    """msda_smoother_workspace_bytes: which 0 = the activation buffer, 1 = the backward workspace (0: invalid geometry)."""
    lib = _lib or load()
    return int(lib.msda_smoother_workspace_bytes(*_smoother_geo(dims, n_mod, call_mod, call_B, call_C), int(which)))


def _smoother_check(what, xs, params, call_mod, call_C, T):
    dev = xs[0].device
    _check_f32(what, dev, list(xs) + list(params))
    if len(xs) != len(call_mod) or any(x.dim() != 2 or x.shape[1] != c or x.shape[0] % T for x, c in zip(xs, call_C)):
        raise RuntimeError("%s: every input must be [B * T, C]" % what)
    return dev


def smoother_forward(dims, n_mod, call_mod, xs, params, training=False, p=0.0, seed=None):
    """msda_smoother_forward_f32.  xs: per call [B * T, C]; params: every module's parameters in parameters() order.
    Returns (outputs [B * O, C] per call, the activation buffer the backward reads).  2 nb + 3 launches, no host sync."""
    T, O = dims[0], dims[1]
    call_C = [x.shape[1] for x in xs]
    call_B = [x.shape[0] // T if T else 0 for x in xs]
    dev = _smoother_check("smoother_forward", xs, params, call_mod, call_C, T)
    geo = _smoother_geo(dims, n_mod, call_mod, call_B, call_C)
    if training and p > 0 and (seed is None or not seed.is_cuda or seed.dtype != torch.int64):
        raise RuntimeError("smoother_forward: training with p > 0 needs a one-element int64 CUDA seed")
    nbytes = smoother_workspace_bytes(dims, n_mod, call_mod, call_B, call_C, 0)
    act = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=dev)
    outs = [torch.empty(b * O, c, dtype=torch.float32, device=dev) for b, c in zip(call_B, call_C)]
    _launch(dev, "msda_smoother_forward_f32", "smoother_forward", *geo, _ptr_array(xs), _ptr_array(params), _ptr_array(outs),
            act.data_ptr(), act.numel() * 4, int(bool(training)), float(p), seed.data_ptr() if seed is not None else None)
    return outs, act


def smoother_backward(dims, n_mod, call_mod, xs, params, act, grad_outs, want_grad_x, training=False, p=0.0, seed=None):
    """msda_smoother_backward_f32: (input gradients per call — None where not wanted —, one flat buffer of every parameter's
    gradient in the order of `params`).  At most 2 nb + 5 launches, no host sync."""
    T = dims[0]
    call_C = [x.shape[1] for x in xs]
    call_B = [x.shape[0] // T for x in xs]
    dev = _smoother_check("smoother_backward", xs, params, call_mod, call_C, T)
    if not all(_f32_cuda(g) and g.device == dev for g in grad_outs):
        raise RuntimeError("smoother_backward: expected contiguous fp32 CUDA output gradients")
    geo = _smoother_geo(dims, n_mod, call_mod, call_B, call_C)
    nbytes = smoother_workspace_bytes(dims, n_mod, call_mod, call_B, call_C, 1)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=dev)
    gp = torch.empty(sum(t.numel() for t in params), dtype=torch.float32, device=dev)
    gx = [torch.empty_like(x) if w else None for x, w in zip(xs, want_grad_x)]
    gx_arr = (_VP * len(gx))(*[g.data_ptr() if g is not None else None for g in gx]) if any(want_grad_x) else None
    _launch(dev, "msda_smoother_backward_f32", "smoother_backward", *geo, _ptr_array(xs), _ptr_array(params), act.data_ptr(),
            act.numel() * 4, _ptr_array(grad_outs), gx_arr, gp.data_ptr(), int(bool(training)), float(p),
            seed.data_ptr() if seed is not None else None, ws.data_ptr(), ws.numel() * 4)
    return gx, gp


def smoother_dropout_mask(seed, problem, layer, rows, cols, p):
    """msda_smoother_dropout_mask_f32 (tests): the kernels' keep mask (1 / 0) of (problem, layer) over [rows, cols]."""
    if not (seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1):
        raise RuntimeError("smoother_dropout_mask: seed must be a one-element int64 CUDA tensor")
    dev = seed.device
    mask = torch.empty(rows, cols, dtype=torch.float32, device=dev)
    _launch(dev, "msda_smoother_dropout_mask_f32", "smoother_dropout_mask", seed.data_ptr(), int(problem), int(layer),
            int(rows), int(cols), float(p), mask.data_ptr())
    return mask


ARCTIC_ITEM_WIDTHS = (3, 3, 48, 10, 1, 3)             # hand_cam, obj_cam, mano_pose, mano_shape, obj_rad, obj_rot
ARCTIC_ITEM_OUT_SOURCES = (0, 0, 1, 2, 2, 3, 3, 5, 4)  # root_l, root_r, root_o, pose_l, pose_r, shape_l, shape_r, rot, rad


def arctic_item_forward(logits, sources, obj_end, hand_l, hand_r):
    """msda_arctic_item_forward_f32: (nine gathered outputs, idx [bs, 3] int64: left, right, object).  One launch."""
    bs, Q, K = logits.shape
    dev = logits.device
    _check_f32("arctic_item", dev, [logits] + list(sources))
    if any(tuple(s.shape) != (bs, Q, w) for s, w in zip(sources, ARCTIC_ITEM_WIDTHS)):
        raise RuntimeError("arctic_item: sources must be [bs, Q, w] with w = %s" % (ARCTIC_ITEM_WIDTHS,))
    outs = [torch.empty(bs, ARCTIC_ITEM_WIDTHS[s], dtype=torch.float32, device=dev) for s in ARCTIC_ITEM_OUT_SOURCES]
    idx = torch.empty(bs, 3, dtype=torch.int64, device=dev)
    _launch(dev, "msda_arctic_item_forward_f32", "arctic_item_forward", bs, Q, K, int(obj_end), int(hand_l), int(hand_r),
            logits.data_ptr(), _ptr_array(sources), _ptr_array(outs), idx.data_ptr())
    return outs, idx


def arctic_item_backward(idx, Q, grad_outs):
    """msda_arctic_item_backward_f32: the six source gradients [bs, Q, w], every element written.  One launch."""
    bs = idx.shape[0]
    dev = idx.device
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()):
        raise RuntimeError("arctic_item_backward: idx must be a contiguous int64 CUDA tensor")
    if not all(g is None or (_f32_cuda(g) and g.device == dev) for g in grad_outs):
        raise RuntimeError("arctic_item_backward: expected contiguous fp32 CUDA output gradients")
    gsrc = [torch.empty(bs, Q, w, dtype=torch.float32, device=dev) for w in ARCTIC_ITEM_WIDTHS]
    garr = (_VP * len(grad_outs))(*[g.data_ptr() if g is not None else None for g in grad_outs])
    _launch(dev, "msda_arctic_item_backward_f32", "arctic_item_backward", bs, int(Q), idx.data_ptr(), garr, _ptr_array(gsrc))
    return gsrc


def _arctic_item_src_dtype(what, dev, tensors):
    """The one dtype (fp32 or bf16) of contiguous CUDA tensors on `dev`."""
    dtype = tensors[0].dtype
    if dtype not in (torch.float32, torch.bfloat16) or not all(
            t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous() for t in tensors):
        raise RuntimeError("%s: expected contiguous CUDA sources on one device, all fp32 or all bf16" % what)
    return dtype


def arctic_item_many_forward(logits, sources, obj_end, hand_l, hand_r):
    """msda_arctic_item_many_forward for per-set lists: logits[s] fp32 [bs, Q, K] and sources[s] the six tensors, all fp32 or
    all bf16.  Returns (per set the nine fp32 outputs, idx [n_sets, bs, 3] int64).  One launch."""
    n = len(logits)
    bs, Q, K = logits[0].shape
    dev = logits[0].device
    _check_f32("arctic_item_many", dev, logits)
    flat = [t for grp in sources for t in grp]
    dtype = _arctic_item_src_dtype("arctic_item_many", dev, flat)
    if len(sources) != n or any(tuple(l.shape) != (bs, Q, K) for l in logits) or any(
            len(grp) != 6 or any(tuple(s.shape) != (bs, Q, w) for s, w in zip(grp, ARCTIC_ITEM_WIDTHS)) for grp in sources):
        raise RuntimeError("arctic_item_many: every set needs logits [bs, Q, K] and sources [bs, Q, w] with w = %s"
                           % (ARCTIC_ITEM_WIDTHS,))
    outs = [[torch.empty(bs, ARCTIC_ITEM_WIDTHS[s], dtype=torch.float32, device=dev) for s in ARCTIC_ITEM_OUT_SOURCES]
            for _ in range(n)]
    idx = torch.empty(n, bs, 3, dtype=torch.int64, device=dev)
    _launch(dev, "msda_arctic_item_many_forward", "arctic_item_many_forward", n, bs, Q, K, int(obj_end), int(hand_l),
            int(hand_r), int(dtype == torch.bfloat16), _ptr_array(logits), _ptr_array(flat),
            _ptr_array([t for grp in outs for t in grp]), idx.data_ptr())
    return outs, idx


def arctic_item_many_backward(idx, Q, grad_outs, dtype):
    """msda_arctic_item_many_backward: per set the six source gradients [bs, Q, w] of `dtype` (fp32 or bf16), every element
    written, from the flat list of n_sets * 9 fp32 output gradients (None: no gradient).  One launch."""
    dev = idx.device
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous() and idx.dim() == 3 and idx.shape[2] == 3
            and len(grad_outs) == 9 * idx.shape[0] and dtype in (torch.float32, torch.bfloat16)):
        raise RuntimeError("arctic_item_many_backward: idx must be a contiguous int64 CUDA tensor [n_sets, bs, 3] with nine "
                           "output gradients per set")
    n, bs = idx.shape[:2]
    if not all(g is None or (_f32_cuda(g) and g.device == dev and tuple(g.shape) == (bs, ARCTIC_ITEM_WIDTHS[ARCTIC_ITEM_OUT_SOURCES[i % 9]]))
               for i, g in enumerate(grad_outs)):
        raise RuntimeError("arctic_item_many_backward: expected contiguous fp32 CUDA output gradients [bs, w]")
    gsrc = [[torch.empty(bs, Q, w, dtype=dtype, device=dev) for w in ARCTIC_ITEM_WIDTHS] for _ in range(n)]
    _launch(dev, "msda_arctic_item_many_backward", "arctic_item_many_backward", n, bs, int(Q), int(dtype == torch.bfloat16),
            idx.data_ptr(), _ptr_table(grad_outs), _ptr_array([t for grp in gsrc for t in grp]))
    return gsrc


# ---- Swin window attention, head_dim 32, fp32 and bf16 (msda_swin.hip) ---------------------------------------------------
SWIN_MAX_WINDOW = 12


def swin_attn_supported(geo):
    """msda_swin_attn_supported: geo = (B, H, W, C, nH, ws, shift)."""
    return bool((_lib or load()).msda_swin_attn_supported(*[int(g) for g in geo]))


def swin_attn_workspace_bytes(geo, which):
    """msda_swin_attn_workspace_bytes: which 0 = the lse buffer, 1 = the backward workspace (0: unsupported geometry)."""
    return int((_lib or load()).msda_swin_attn_workspace_bytes(*[int(g) for g in geo], int(which)))


def _swin_check(what, geo, tensors):
    """qkv's dtype picks the form: fp32 (every tensor fp32) or bfloat16 (qkv, out and grad_out bfloat16, the rest fp32)."""
    dev = tensors[0].device
    qkv, bias, table = tensors[:3]
    bf16 = qkv.dtype == torch.bfloat16
    _check_f32(what, dev, [bias, table] + ([] if bf16 else [qkv]))
    acts = [t for t in tensors[3:] if t is not None]
    if len(acts) == 3:                                              # out, lse, grad_out
        _check_f32(what, dev, [acts[1]] + ([] if bf16 else [acts[0], acts[2]]))
    if bf16 and not all(t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() and t.device == dev
                        for t in [qkv] + acts[:1] + acts[2:]):
        raise RuntimeError("%s: bfloat16 qkv needs contiguous bfloat16 out and grad_out on its device" % what)
    B, H, W, C, nH, ws, _ = geo
    if tuple(qkv.shape) != (B * H * W, 3 * C) or (bias is not None and tuple(bias.shape) != (3 * C,)) \
            or tuple(table.shape) != ((2 * ws - 1) ** 2, nH):
        raise RuntimeError("%s: expected qkv [B*H*W, 3C], qkv_bias [3C], table [(2ws-1)^2, nH]" % what)
    return dev, "bf16" if bf16 else "f32"


def _vp(t):
    return t.data_ptr() if t is not None else None


def swin_attn_forward(geo, qkv, bias, table):
    """msda_swin_attn_forward_f32 / _bf16 by qkv's dtype: (out [B*H*W, C] of that dtype, lse fp32).  One launch, no host sync."""
    geo = tuple(int(g) for g in geo)
    dev, suf = _swin_check("swin_attn_forward", geo, [qkv, bias, table])
    out = torch.empty(qkv.shape[0], geo[3], dtype=qkv.dtype, device=dev)
    nbytes = swin_attn_workspace_bytes(geo, 0)
    lse = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=dev)
    _launch(dev, "msda_swin_attn_forward_" + suf, "swin_attn_forward", *geo, qkv.data_ptr(), _vp(bias), table.data_ptr(),
            out.data_ptr(), lse.data_ptr(), lse.numel() * 4)
    return out, lse


def swin_attn_backward(geo, qkv, bias, table, out, lse, grad_out):
    """msda_swin_attn_backward_f32 / _bf16 by qkv's dtype: (grad_qkv [B*H*W, 3C] of that dtype, grad_table fp32, grad_bias
    [3C] fp32 — the padded tokens' part, q part 0 — or None without a bias).  Three launches, no host sync."""
    geo = tuple(int(g) for g in geo)
    dev, suf = _swin_check("swin_attn_backward", geo, [qkv, bias, table, out, lse, grad_out])
    if tuple(out.shape) != (qkv.shape[0], geo[3]) or out.shape != grad_out.shape:
        raise RuntimeError("swin_attn_backward: expected out and grad_out [B*H*W, C]")
    gq = torch.empty_like(qkv)
    gt = torch.empty_like(table)
    gb = torch.empty_like(bias) if bias is not None else None
    nbytes = swin_attn_workspace_bytes(geo, 1)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=dev)
    _launch(dev, "msda_swin_attn_backward_" + suf, "swin_attn_backward", *geo, qkv.data_ptr(), _vp(bias), table.data_ptr(),
            out.data_ptr(), lse.data_ptr(), lse.numel() * 4, grad_out.data_ptr(), gq.data_ptr(), gt.data_ptr(), _vp(gb),
            ws.data_ptr(), ws.numel() * 4)
    return gq, gt, gb


# ---- the Swin blocks' residual / drop-path / LayerNorm glue, PatchMerging's gather + norm (msda_swin_glue.hip) -----------------
SWIN_GLUE_MAX_WIDTH = 3072


def swin_glue_supported(C):
    """msda_swin_glue_supported: C % 4 == 0 and 0 < C <= 3072."""
    return bool((_lib or load()).msda_swin_glue_supported(int(C)))


def swin_glue_workspace_bytes(rows, C):
    """msda_swin_glue_workspace_bytes: the backward's partial column sums, min(1024, max(1, ceil(rows / 16))) * 2 * C * 4."""
    return int((_lib or load()).msda_swin_glue_workspace_bytes(int(rows), int(C)))


def _glue_suffix(what, dtype, stream=torch.float32):
    """The entry's suffix: <T> for an fp32 residual stream, <T>_sbf16 for a bf16 one (bf16 T; fp32 T for norm alone)."""
    if stream not in (torch.float32, torch.bfloat16):
        raise RuntimeError("%s: the residual stream is float32 or bfloat16, got %s" % (what, stream))
    tail = "_sbf16" if stream == torch.bfloat16 else ""
    if dtype == torch.float32 and (not tail or what.startswith("swin_glue_norm_")):
        return "f32" + tail
    if dtype == torch.bfloat16:
        return "bf16" + tail
    if tail:
        raise RuntimeError("%s: a bfloat16 residual stream takes a bfloat16 branch, got %s" % (what, dtype))
    raise RuntimeError("%s: the branch / output type is float32 or bfloat16, got %s" % (what, dtype))


def _glue_check(what, dev, f32, typed=(), dtype=torch.float32, stream=(), stream_dtype=torch.float32):
    """Every tensor of `f32` contiguous fp32 on dev, every tensor of `typed` contiguous `dtype` there and every tensor of
    `stream` (the residual stream's rows) contiguous `stream_dtype` there (None entries skipped)."""
    _check_f32(what, dev, f32)
    for group, want in ((typed, dtype), (stream, stream_dtype)):
        if not all(t is None or (t.is_cuda and t.dtype == want and t.is_contiguous() and t.device == dev) for t in group):
            raise RuntimeError("%s: expected contiguous %s CUDA tensors on the rows' device" % (what, want))


def _glue_rows(what, x, others=()):
    """(rows, C) of x [..., C]; every tensor of `others` has x's shape."""
    if x.dim() < 1 or any(t is not None and t.shape != x.shape for t in others):
        raise RuntimeError("%s: expected tensors of one shape [..., C]" % what)
    C = x.shape[-1]
    return (x.numel() // C if C else 0), C


def _glue_keep(what, keep, rows, rows_per_sample):
    rows_per_sample = int(rows_per_sample)
    if keep is not None and (rows_per_sample <= 0 or keep.numel() * rows_per_sample < rows):
        raise RuntimeError("%s: keep holds %d samples of %d rows, the tensor has %d rows"
                           % (what, keep.numel(), rows_per_sample, rows))
    return rows_per_sample if keep is not None else max(1, rows)


def _glue_params(what, C, *params):
    if any(tuple(p.shape) != (C,) for p in params):
        raise RuntimeError("%s: expected LayerNorm parameters of shape [%d]" % (what, C))


def _glue_workspace(rows, C, dev):
    nbytes = max(16, swin_glue_workspace_bytes(rows, C))
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def swin_glue_norm_forward(x, weight, bias, eps, out_dtype):
    """msda_swin_glue_norm_forward_*: (z of out_dtype, mean, rstd) = LayerNorm over the last dimension of x (fp32, or bf16: the
    _sbf16 entries).  One launch."""
    what = "swin_glue_norm_forward"
    suf = _glue_suffix(what, out_dtype, x.dtype)
    _glue_check(what, x.device, [weight, bias], stream=[x], stream_dtype=x.dtype)
    rows, C = _glue_rows(what, x)
    _glue_params(what, C, weight, bias)
    z = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _launch(x.device, "msda_swin_glue_norm_forward_" + suf, what, x.data_ptr(), weight.data_ptr(), bias.data_ptr(), rows, C,
            float(eps), z.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    return z, mean, rstd


def swin_glue_norm_backward(grad_z, x, weight, mean, rstd):
    """msda_swin_glue_norm_backward_* by grad_z's and x's dtypes: (grad_x of x's type, grad_weight, grad_bias).  Two launches."""
    what = "swin_glue_norm_backward"
    suf = _glue_suffix(what, grad_z.dtype, x.dtype)
    _glue_check(what, x.device, [weight, mean, rstd], [grad_z], grad_z.dtype, [x], x.dtype)
    rows, C = _glue_rows(what, x, [grad_z])
    _glue_params(what, C, weight)
    gx = torch.empty_like(x)
    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
    ws, nbytes = _glue_workspace(rows, C, x.device)
    _launch(x.device, "msda_swin_glue_norm_backward_" + suf, what, grad_z.data_ptr(), x.data_ptr(), weight.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), rows, C, gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), nbytes)
    return gx, gw, gb


def swin_glue_add_norm_forward(x, a, keep, rows_per_sample, weight, bias, eps):
    """msda_swin_glue_add_norm_forward_* by a's dtype T and x's: (y of x's type = x + rnd_T(a * keep[row // rows_per_sample]),
    rounded once more where x is bf16; z = LN(y) as T, mean, rstd); keep [samples] of T or None.  One launch."""
    what = "swin_glue_add_norm_forward"
    suf = _glue_suffix(what, a.dtype, x.dtype)
    _glue_check(what, x.device, [weight, bias], [a, keep], a.dtype, [x], x.dtype)
    rows, C = _glue_rows(what, x, [a])
    _glue_params(what, C, weight, bias)
    rps = _glue_keep(what, keep, rows, rows_per_sample)
    y = torch.empty_like(x)
    z = torch.empty_like(a)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _launch(x.device, "msda_swin_glue_add_norm_forward_" + suf, what, x.data_ptr(), a.data_ptr(), _vp(keep), rows, rps, C,
            weight.data_ptr(), bias.data_ptr(), float(eps), y.data_ptr(), z.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    return y, z, mean, rstd


def swin_glue_add_norm_backward(grad_y, grad_z, y, keep, rows_per_sample, weight, mean, rstd):
    """msda_swin_glue_add_norm_backward_* by grad_z's dtype T and y's: (grad_x of y's type = grad_y + LN'(grad_z), grad_a of T =
    rnd_T(rnd_T(grad_x) * keep), grad_weight, grad_bias); a bf16 y rounds LN'(grad_z) and the sum (msda.h).  Where T is y's type
    and there is no keep, grad_a IS grad_x (the same tensor).  Two launches."""
    what = "swin_glue_add_norm_backward"
    suf = _glue_suffix(what, grad_z.dtype, y.dtype)
    _glue_check(what, y.device, [weight, mean, rstd], [grad_z, keep], grad_z.dtype, [grad_y, y], y.dtype)
    rows, C = _glue_rows(what, y, [grad_y, grad_z])
    _glue_params(what, C, weight)
    rps = _glue_keep(what, keep, rows, rows_per_sample)
    gx = torch.empty_like(y)
    ga = gx if (grad_z.dtype == y.dtype and keep is None) else torch.empty_like(grad_z)
    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
    ws, nbytes = _glue_workspace(rows, C, y.device)
    _launch(y.device, "msda_swin_glue_add_norm_backward_" + suf, what, grad_y.data_ptr(), grad_z.data_ptr(), y.data_ptr(),
            _vp(keep), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, rps, C, gx.data_ptr(),
            ga.data_ptr() if ga is not gx else None, gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), nbytes)
    return gx, ga, gw, gb


def swin_glue_add_forward(x, a, keep, rows_per_sample):
    """msda_swin_glue_add_forward_* by a's dtype T and x's: y of x's type = x + rnd_T(a * keep[row // rows_per_sample]).  One
    launch."""
    what = "swin_glue_add_forward"
    suf = _glue_suffix(what, a.dtype, x.dtype)
    _glue_check(what, x.device, [], [a, keep], a.dtype, [x], x.dtype)
    rows, C = _glue_rows(what, x, [a])
    rps = _glue_keep(what, keep, rows, rows_per_sample)
    y = torch.empty_like(x)
    _launch(x.device, "msda_swin_glue_add_forward_" + suf, what, x.data_ptr(), a.data_ptr(), _vp(keep), rows, rps, C, y.data_ptr())
    return y


def swin_glue_add_backward(grad_y, keep, rows_per_sample, dtype):
    """msda_swin_glue_add_backward_*: grad_a of `dtype` T = rnd_T(rnd_T(grad_y) * keep).  One launch; grad_y of type T without
    keep: grad_y itself, no launch."""
    what = "swin_glue_add_backward"
    suf = _glue_suffix(what, dtype, grad_y.dtype)
    if grad_y.dtype == dtype and keep is None:
        return grad_y
    _glue_check(what, grad_y.device, [], [keep], dtype, [grad_y], grad_y.dtype)
    rows, C = _glue_rows(what, grad_y)
    rps = _glue_keep(what, keep, rows, rows_per_sample)
    ga = torch.empty(grad_y.shape, dtype=dtype, device=grad_y.device)
    _launch(grad_y.device, "msda_swin_glue_add_backward_" + suf, what, grad_y.data_ptr(), _vp(keep), rows, rps, C, ga.data_ptr())
    return ga


def _glue_merge_dims(what, x, weight):
    if x.dim() != 4 or tuple(weight.shape) != (4 * x.shape[3],):
        raise RuntimeError("%s: expected x [B, H, W, C] and LayerNorm parameters [4C]" % what)
    B, H, W, C = x.shape
    return B, H, W, C, (H + 1) // 2 * ((W + 1) // 2)


def swin_glue_merge_norm_forward(x, weight, bias, eps, out_dtype):
    """msda_swin_glue_merge_norm_forward_*: x [B, H, W, C] fp32 or bf16 -> (z [B, ceil(H/2) ceil(W/2), 4C] of out_dtype, mean,
    rstd): PatchMerging's pad, 2 x 2 gather, concatenation and LayerNorm.  One launch."""
    what = "swin_glue_merge_norm_forward"
    suf = _glue_suffix(what, out_dtype, x.dtype)
    _glue_check(what, x.device, [weight, bias], stream=[x], stream_dtype=x.dtype)
    B, H, W, C, L2 = _glue_merge_dims(what, x, weight)
    _glue_params(what, 4 * C, bias)
    z = torch.empty((B, L2, 4 * C), dtype=out_dtype, device=x.device)
    mean = torch.empty((B * L2,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((B * L2,), dtype=torch.float32, device=x.device)
    _launch(x.device, "msda_swin_glue_merge_norm_forward_" + suf, what, x.data_ptr(), B, H, W, C, weight.data_ptr(),
            bias.data_ptr(), float(eps), z.data_ptr(), mean.data_ptr(), rstd.data_ptr())
    return z, mean, rstd


def swin_glue_merge_norm_backward(grad_z, x, weight, mean, rstd):
    """msda_swin_glue_merge_norm_backward_* by grad_z's and x's dtypes: (grad_x [B, H, W, C] of x's type, grad_weight, grad_bias).
    Two launches."""
    what = "swin_glue_merge_norm_backward"
    suf = _glue_suffix(what, grad_z.dtype, x.dtype)
    _glue_check(what, x.device, [weight, mean, rstd], [grad_z], grad_z.dtype, [x], x.dtype)
    B, H, W, C, L2 = _glue_merge_dims(what, x, weight)
    if tuple(grad_z.shape) != (B, L2, 4 * C):
        raise RuntimeError("%s: expected grad_z [B, ceil(H/2) ceil(W/2), 4C]" % what)
    gx = torch.empty_like(x)
    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
    ws, nbytes = _glue_workspace(B * L2, 4 * C, x.device)
    _launch(x.device, "msda_swin_glue_merge_norm_backward_" + suf, what, grad_z.data_ptr(), x.data_ptr(), weight.data_ptr(),
            mean.data_ptr(), rstd.data_ptr(), B, H, W, C, gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), nbytes)
    return gx, gw, gb


# ---- MANO hand layer: grouped lbs (msda_mano.hip) -----------------------------------------------------------------------------
MANO_MAX_LAYERS, MANO_MAX_GROUPS, MANO_MAX_EXTRA, MANO_MAX_BETAS, MANO_MAX_VERTS = 4, 16, 8, 16, 8192


def mano_supported(V, n_betas, n_extra):
    """msda_mano_supported (include/msda.h): 1 when the MANO kernels take this model size."""
    return bool((_lib or load()).msda_mano_supported(int(V), int(n_betas), int(n_extra)))


def _mano_geo(dims, layers, group_layer, group_B, group_bcast):
    """dims (V, n_betas, n_extra); layers: per layer (seven fp32 tensors in msda.h's order, parents + extra ids as ints)."""
    V, nb, E = dims
    tensors = [t for lay in layers for t in lay[0]]
    index = [int(i) for lay in layers for i in lay[1]]
    return [int(V), int(nb), int(E), len(layers), _ptr_array(tensors), _int_array(index), len(group_B), _int_array(group_layer),
            _int_array(group_B), _int_array(group_bcast)]


def mano_workspace_bytes(dims, group_B):
    return int((_lib or load()).msda_mano_workspace_bytes(int(dims[0]), int(dims[1]), int(dims[2]), len(group_B),
                                                          _int_array(group_B)))


def mano_forward(dims, layers, group_layer, group_bcast, inputs):
    """msda_mano_forward_f32.  inputs: per group (betas, global_orient, hand_pose, transl or None).  Returns per group
    (vertices [B, V, 3], joints [B, 16 + E, 3]).  One launch, no host sync."""
    V, _, E = dims
    dev = inputs[0][1].device
    _check_f32("mano_forward", dev, [t for lay in layers for t in lay[0]] + [t for grp in inputs for t in grp])
    group_B = [grp[1].shape[0] for grp in inputs]
    geo = _mano_geo(dims, layers, group_layer, group_B, group_bcast)
    outs = [(torch.empty(b, V, 3, dtype=torch.float32, device=dev), torch.empty(b, 16 + E, 3, dtype=torch.float32, device=dev))
            for b in group_B]
    ins = (_VP * (4 * len(inputs)))(*[_vp(t) for grp in inputs for t in grp])
    o = (_VP * (2 * len(outs)))(*[t.data_ptr() for pair in outs for t in pair])
    _launch(dev, "msda_mano_forward_f32", "mano_forward", *geo, ins, o)
    return outs


def mano_backward(dims, layers, group_layer, group_bcast, inputs, grad_outputs):
    """msda_mano_backward_f32.  grad_outputs: per group (g_vertices, g_joints), either None.  Returns per group (g_betas per
    hand [B, n_betas], g_global_orient [B, 3], g_hand_pose [B, 45], g_transl [B, 3] or None without transl).  Two launches,
    no host sync."""
    _, nb, _ = dims
    dev = inputs[0][1].device
    _check_f32("mano_backward", dev, [t for lay in layers for t in lay[0]] + [t for grp in inputs for t in grp]
                + [t for grp in grad_outputs for t in grp])
    group_B = [grp[1].shape[0] for grp in inputs]
    geo = _mano_geo(dims, layers, group_layer, group_B, group_bcast)
    nbytes = mano_workspace_bytes(dims, group_B)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=dev)
    grads = [(torch.empty(b, nb, dtype=torch.float32, device=dev), torch.empty(b, 3, dtype=torch.float32, device=dev),
              torch.empty(b, 45, dtype=torch.float32, device=dev),
              torch.empty(b, 3, dtype=torch.float32, device=dev) if grp[3] is not None else None)
             for b, grp in zip(group_B, inputs)]
    ins = (_VP * (4 * len(inputs)))(*[_vp(t) for grp in inputs for t in grp])
    gos = (_VP * (2 * len(grad_outputs)))(*[_vp(t) for grp in grad_outputs for t in grp])
    gs = (_VP * (4 * len(grads)))(*[_vp(t) for grp in grads for t in grp])
    _launch(dev, "msda_mano_backward_f32", "mano_backward", *geo, ins, gos, gs, ws.data_ptr(), ws.numel() * 4)
    return grads


# ---- ARCTIC object layer and small losses (msda_small_loss.hip) ---------------------------------------------------------------
OBJECT_MAX_GROUPS, SMALL_LOSS_MAX_SETS = 16, 8
SMALL_LOSS_TERMS, SMALL_LOSS_INPUTS, SMALL_LOSS_TARGETS = 19, 15, 25


def object_supported(n_objects, max_len, n_sub, n_bbox_top, n_bbox_bottom, n_kp_top, n_kp_bottom):
    """msda_object_supported (include/msda.h): 1 when the object kernels take this model size."""
    return bool((_lib or load()).msda_object_supported(int(n_objects), int(max_len), int(n_sub), int(n_bbox_top),
                                                       int(n_bbox_bottom), int(n_kp_top), int(n_kp_bottom)))


def _obj_geo(dims, model, inputs, lens):
    """dims (n_objects, Lm, NS, NBt, NBb, NKt, NKb); model: the 8 model tensors of msda.h; inputs: per group (obj_idx,
    angles, global_orient, transl or None); lens: per group output template rows."""
    group_B = [grp[0].shape[0] for grp in inputs]
    return [_int_array(dims), _ptr_array(model), len(inputs), _int_array(group_B), _int_array(lens),
            (_VP * (4 * len(inputs)))(*[_vp(t) for grp in inputs for t in grp])], group_B


def _obj_check(what, dev, model, tensors):
    ok = all(t.is_cuda and t.device == dev and t.is_contiguous() for t in model + [t for t in tensors if t is not None])
    if not ok or any(t is not None and t.dtype not in (torch.float32, torch.int64) for t in tensors):
        raise RuntimeError("%s: expected contiguous CUDA tensors on one device" % what)


def object_forward(dims, model, inputs, lens):
    """msda_object_forward_f32.  Returns per group (v [B, len, 3], v_sub [B, NS, 3], bbox3d [B, NBt + NBb, 3], kp3d
    [B, NKt + NKb, 3]).  One launch, no host sync."""
    dev = inputs[0][1].device
    _obj_check("object_forward", dev, list(model), [t for grp in inputs for t in grp])
    geo, group_B = _obj_geo(dims, model, inputs, lens)
    _, _, NS, NBt, NBb, NKt, NKb = dims
    e = dict(dtype=torch.float32, device=dev)
    outs = [(torch.empty(b, n, 3, **e), torch.empty(b, NS, 3, **e), torch.empty(b, NBt + NBb, 3, **e),
             torch.empty(b, NKt + NKb, 3, **e)) for b, n in zip(group_B, lens)]
    o = (_VP * (4 * len(outs)))(*[t.data_ptr() for grp in outs for t in grp])
    _launch(dev, "msda_object_forward_f32", "object_forward", *geo, o)
    return outs


def object_backward(dims, model, inputs, lens, grad_outputs, want_transl):
    """msda_object_backward_f32.  grad_outputs: per group 4 tensors or None.  Returns per group (g_angles [B], g_global_orient
    [B, 3], g_transl [B, 3] or None).  One launch, no host sync."""
    dev = inputs[0][1].device
    _obj_check("object_backward", dev, list(model), [t for grp in inputs for t in grp] + [t for grp in grad_outputs for t in grp])
    geo, group_B = _obj_geo(dims, model, inputs, lens)
    e = dict(dtype=torch.float32, device=dev)
    grads = [(torch.empty(b, **e), torch.empty(b, 3, **e), torch.empty(b, 3, **e) if w else None)
             for b, w in zip(group_B, want_transl)]
    gos = (_VP * (4 * len(grad_outputs)))(*[_vp(t) for grp in grad_outputs for t in grp])
    gs = (_VP * (3 * len(grads)))(*[_vp(t) for grp in grads for t in grp])
    _launch(dev, "msda_object_backward_f32", "object_backward", *geo, gos, gs)
    return grads


def small_loss_supported(S, B, J, NV, KO, NB, L):
    return bool((_lib or load()).msda_small_loss_supported(int(S), int(B), int(J), int(NV), int(KO), int(NB), int(L)))


def small_loss_workspace_bytes(S, B, J, NV, KO, NB, L):
    return int((_lib or load()).msda_small_loss_workspace_bytes(int(S), int(B), int(J), int(NV), int(KO), int(NB), int(L)))


def _sl_check(what, dev, tensors):
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() and t.dtype in (torch.float32, torch.int64) for t in tensors):
        raise RuntimeError("%s: expected contiguous CUDA tensors on one device" % what)


def small_loss_forward(dims, img_res, targets, inputs):
    """msda_small_loss_forward_f32.  targets: the 25 tensors of msda.h; inputs: per set 15 tensors.  Returns (losses [S, 19],
    workspace for the backward).  Two launches, no host sync."""
    dev = inputs[0][0].device
    _sl_check("small_loss_forward", dev, list(targets) + [t for grp in inputs for t in grp])
    losses = torch.empty(dims[0], SMALL_LOSS_TERMS, dtype=torch.float32, device=dev)
    nbytes = small_loss_workspace_bytes(*dims)
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=dev)
    ins = (_VP * (SMALL_LOSS_INPUTS * len(inputs)))(*[t.data_ptr() for grp in inputs for t in grp])
    _launch(dev, "msda_small_loss_forward_f32", "small_loss_forward", _int_array(dims), float(img_res), _ptr_array(targets),
            ins, losses.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    return losses, ws


def small_loss_backward(dims, img_res, targets, inputs, grad_losses, ws):
    """msda_small_loss_backward_f32.  Returns per set the 15 input gradients, shaped as the inputs.  One launch."""
    dev = inputs[0][0].device
    _sl_check("small_loss_backward", dev, list(targets) + [t for grp in inputs for t in grp] + [grad_losses, ws])
    grads = [[torch.empty_like(t) for t in grp] for grp in inputs]
    ins = (_VP * (SMALL_LOSS_INPUTS * len(inputs)))(*[t.data_ptr() for grp in inputs for t in grp])
    gs = (_VP * (SMALL_LOSS_INPUTS * len(inputs)))(*[t.data_ptr() for grp in grads for t in grp])
    _launch(dev, "msda_small_loss_backward_f32", "small_loss_backward", _int_array(dims), float(img_res),
            _ptr_array(targets), ins, grad_losses.data_ptr(), gs, ws.data_ptr(), ws.numel() * 4)
    return grads


# ---- ARCTIC evaluation: nearest neighbour and metrics (msda_arctic_eval.hip) --------------------------------------------------
NN_MAX_PAIRS = 8
ARCTIC_METRICS = 6


def nn_supported(B, N1, N2):
    """msda_nn_supported (include/msda.h): 1 when the nearest-neighbour kernels take this geometry."""
    return bool((_lib or load()).msda_nn_supported(int(B), int(N1), int(N2)))


def _nn_check(what, dev, tensors):
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() and t.dtype in (torch.float32, torch.int64) for t in tensors):
        raise RuntimeError("%s: expected contiguous fp32 CUDA tensors on one device" % what)


def nn_forward(pairs):
    """msda_nn_forward_f32.  pairs: [(src [B, N1, 3], trg [B, N2, 3])] sharing B, N1, N2.  Returns per pair (dists [B, N1] fp32
    squared, idx [B, N1] int64).  One launch, no host sync."""
    dev = pairs[0][0].device
    _nn_check("nn_forward", dev, [t for p in pairs for t in p])
    B, N1, _ = pairs[0][0].shape
    N2 = pairs[0][1].shape[1]
    outs = [(torch.empty(B, N1, dtype=torch.float32, device=dev), torch.empty(B, N1, dtype=torch.int64, device=dev)) for _ in pairs]
    _launch(dev, "msda_nn_forward_f32", "nn_forward", len(pairs), B, N1, N2, _ptr_array([p[0] for p in pairs]),
            _ptr_array([p[1] for p in pairs]), _ptr_array([o[0] for o in outs]), _ptr_array([o[1] for o in outs]))
    return outs


def nn_backward(pairs, idxs, grad_dists, want):
    """msda_nn_backward_f32.  want: per pair (want grad_src, want grad_trg).  Returns per pair (grad_src or None, grad_trg or
    None).  One launch, no atomics."""
    dev = pairs[0][0].device
    _nn_check("nn_backward", dev, [t for p in pairs for t in p] + list(idxs) + list(grad_dists))
    grads = [(torch.empty_like(s) if ws else None, torch.empty_like(t) if wt else None) for (s, t), (ws, wt) in zip(pairs, want)]
    B, N1, _ = pairs[0][0].shape
    N2 = pairs[0][1].shape[1]
    _launch(dev, "msda_nn_backward_f32", "nn_backward", len(pairs), B, N1, N2, _ptr_array([p[0] for p in pairs]),
            _ptr_array([p[1] for p in pairs]), _ptr_array(idxs), _ptr_array(grad_dists),
            (_VP * len(grads))(*[_vp(g[0]) for g in grads]), (_VP * len(grads))(*[_vp(g[1]) for g in grads]))
    return grads


def arctic_metrics_supported(B, J, NV, L_pred, L_gt, L_parts):
    return bool((_lib or load()).msda_arctic_metrics_supported(int(B), int(J), int(NV), int(L_pred), int(L_gt), int(L_parts)))


def arctic_metrics(dims, floats, longs):
    """msda_arctic_metrics_f32.  floats: the 16 fp32 tensors, longs: the 4 int64 tensors of msda.h.  Returns [6, B] fp32."""
    dev = floats[0].device
    _nn_check("arctic_metrics", dev, list(floats) + list(longs))
    out = torch.empty(ARCTIC_METRICS, dims[0], dtype=torch.float32, device=dev)
    _launch(dev, "msda_arctic_metrics_f32", "arctic_metrics", _int_array(dims), _ptr_array(floats), _ptr_array(longs),
            out.data_ptr())
    return out


def arctic_metrics_accumulate(values, total, count):
    """msda_arctic_metrics_accumulate_f32: values [6, B] fp32 into total / count (fp64 [6]), in place."""
    dev = values.device
    if not (values.is_cuda and values.is_contiguous() and values.dtype == torch.float32 and values.shape[0] == ARCTIC_METRICS
            and all(t.device == dev and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == ARCTIC_METRICS
                    for t in (total, count))):
        raise RuntimeError("arctic_metrics_accumulate: expected values [6, B] fp32 and fp64 total / count of 6 on one device")
    _launch(dev, "msda_arctic_metrics_accumulate_f32", "arctic_metrics_accumulate", values.data_ptr(), int(values.shape[1]),
            total.data_ptr(), count.data_ptr())


# ---- make_output's pose, camera and projection glue (msda_arctic_output.hip) ---------------------------------------------------
ARCTIC_PLACE_MAX_SEGMENTS = 8
ARCTIC_PLACE_MAX_ROWS = 8192


def _opt_ptr_array(ts):
    return (_VP * max(1, len(ts)))(*[_vp(t) for t in ts])


def arctic_pose_supported(n_hands, n_roots, B):
    """msda_arctic_pose_supported (include/msda.h)."""
    return bool((_lib or load()).msda_arctic_pose_supported(int(n_hands), int(n_roots), int(B)))


def arctic_place_supported(n_segments, B, max_rows):
    """msda_arctic_place_supported (include/msda.h)."""
    return bool((_lib or load()).msda_arctic_place_supported(int(n_segments), int(B), int(max_rows)))


def arctic_pose_forward(poses, roots, K, img_res):
    """msda_arctic_pose_forward_f32.  poses: [B, 48] each, roots: [B, 3] each, K [B, 3, 3].  Returns (mats [B, 16, 3, 3] per
    pose, aa [B, 48] per pose, cam_t [B, 3] per root).  One launch, no host sync."""
    dev, B = K.device, K.shape[0]
    _nn_check("arctic_pose_forward", dev, list(poses) + list(roots) + [K])
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    mats, aas, cts = [new(B, 16, 3, 3) for _ in poses], [new(B, 48) for _ in poses], [new(B, 3) for _ in roots]
    _launch(dev, "msda_arctic_pose_forward_f32", "arctic_pose_forward", len(poses), len(roots), B, float(img_res),
            _opt_ptr_array(poses), _opt_ptr_array(roots), K.data_ptr(), _opt_ptr_array(mats), _opt_ptr_array(aas),
            _opt_ptr_array(cts))
    return mats, aas, cts


def arctic_pose_backward(poses, roots, K, img_res, grad_mats, grad_aa, grad_cam_t, want_poses, want_roots):
    """msda_arctic_pose_backward_f32.  The gradient lists hold None for an output without gradient; want_*: per input.
    Returns (grad_poses, grad_roots) with None where not wanted.  One launch."""
    dev, B = K.device, K.shape[0]
    given = [g for g in list(grad_mats) + list(grad_aa) + list(grad_cam_t) if g is not None]
    _nn_check("arctic_pose_backward", dev, list(poses) + list(roots) + [K] + given)
    gp = [torch.empty_like(p) if w else None for p, w in zip(poses, want_poses)]
    gr = [torch.empty_like(r) if w else None for r, w in zip(roots, want_roots)]
    _launch(dev, "msda_arctic_pose_backward_f32", "arctic_pose_backward", len(poses), len(roots), B, float(img_res),
            _opt_ptr_array(poses), _opt_ptr_array(roots), K.data_ptr(), _opt_ptr_array(grad_mats), _opt_ptr_array(grad_aa),
            _opt_ptr_array(grad_cam_t), _opt_ptr_array(gp), _opt_ptr_array(gr))
    return gp, gr


def arctic_m2aa_forward(mats):
    """msda_arctic_m2aa_forward_f32.  mats: [B, 16, 3, 3] each (1 .. 2).  Returns aa [B, 16, 3] each.  One launch."""
    dev, B = mats[0].device, mats[0].shape[0]
    _nn_check("arctic_m2aa_forward", dev, list(mats))
    aas = [torch.empty(B, 16, 3, dtype=torch.float32, device=dev) for _ in mats]
    _launch(dev, "msda_arctic_m2aa_forward_f32", "arctic_m2aa_forward", len(mats), B, _ptr_array(mats), _ptr_array(aas))
    return aas


def arctic_m2aa_backward(mats, grad_aa, want):
    """msda_arctic_m2aa_backward_f32.  grad_aa holds None for an output without gradient.  One launch."""
    dev, B = mats[0].device, mats[0].shape[0]
    _nn_check("arctic_m2aa_backward", dev, list(mats) + [g for g in grad_aa if g is not None])
    gm = [torch.empty_like(m) if w else None for m, w in zip(mats, want)]
    _launch(dev, "msda_arctic_m2aa_backward_f32", "arctic_m2aa_backward", len(mats), B, _ptr_array(mats), _opt_ptr_array(grad_aa),
            _opt_ptr_array(gm))
    return gm


def _place_geo(points, cameras, projects):
    return (_int_array([p.shape[1] for p in points]), _int_array(cameras), _int_array([1 if p else 0 for p in projects]))


def arctic_place_forward(points, cameras, projects, cam_ts, K, img_res):
    """msda_arctic_place_forward_f32.  points: [B, n, 3] each; cam_ts: three [B, 3] or None.  Returns per segment (placed,
    norm2d or None, pix2d or None).  One launch, no host sync."""
    dev, B = points[0].device, points[0].shape[0]
    _nn_check("arctic_place_forward", dev, list(points) + [c for c in cam_ts if c is not None] + [K])
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    placed = [torch.empty_like(p) for p in points]
    n2 = [new(B, p.shape[1], 2) if pr else None for p, pr in zip(points, projects)]
    px = [new(B, p.shape[1], 2) if pr else None for p, pr in zip(points, projects)]
    _launch(dev, "msda_arctic_place_forward_f32", "arctic_place_forward", len(points), B, float(img_res),
            *_place_geo(points, cameras, projects), _ptr_array(points), _opt_ptr_array(cam_ts), K.data_ptr(), _ptr_array(placed),
            _opt_ptr_array(n2), _opt_ptr_array(px))
    return list(zip(placed, n2, px))


def arctic_place_backward(points, cameras, projects, cam_ts, K, img_res, grad_placed, grad_n2, grad_px, want_points, want_cams):
    """msda_arctic_place_backward_f32.  The gradient lists hold None for an output without gradient.  Returns (grad_points,
    grad_cam_ts) with None where not wanted.  One launch, no atomics."""
    dev, B = points[0].device, points[0].shape[0]
    given = [g for g in list(grad_placed) + list(grad_n2) + list(grad_px) if g is not None]
    _nn_check("arctic_place_backward", dev, list(points) + [c for c in cam_ts if c is not None] + [K] + given)
    gp = [torch.empty_like(p) if w else None for p, w in zip(points, want_points)]
    gc = [torch.empty(B, 3, dtype=torch.float32, device=dev) if w else None for w in want_cams]
    _launch(dev, "msda_arctic_place_backward_f32", "arctic_place_backward", len(points), B, float(img_res),
            *_place_geo(points, cameras, projects), _ptr_array(points), _opt_ptr_array(cam_ts), K.data_ptr(),
            _opt_ptr_array(grad_placed), _opt_ptr_array(grad_n2), _opt_ptr_array(grad_px), _opt_ptr_array(gp), _opt_ptr_array(gc))
    return gp, gc


# ---- the SmoothNet criterion: contact deviation and acceleration errors (msda_smooth_loss.hip) ---------------------------------
SMOOTH_LOSS_TERMS, SMOOTH_LOSS_FLOATS, SMOOTH_LOSS_LONGS, SMOOTH_LOSS_GRADS = 3, 15, 3, 5


def smooth_loss_supported(N, NV, J, L):
    """msda_smooth_loss_supported (include/msda.h): 1 when the kernels take this geometry."""
    return bool((_lib or load()).msda_smooth_loss_supported(int(N), int(NV), int(J), int(L)))


def smooth_loss_workspace_bytes(N, NV, J, L):
    return int((_lib or load()).msda_smooth_loss_workspace_bytes(int(N), int(NV), int(J), int(L)))


def smooth_loss_forward(dims, fps, floats, longs, want_frames=False):
    """msda_smooth_loss_forward_f32.  floats: the 15 fp32 tensors, longs: the 3 int64 tensors of msda.h.  Returns (losses [3],
    frames [2, N] or None, workspace for the backward).  Three launches, no host sync."""
    dev = floats[0].device
    _nn_check("smooth_loss_forward", dev, list(floats) + list(longs))
    losses = torch.empty(SMOOTH_LOSS_TERMS, dtype=torch.float32, device=dev)
    frames = torch.empty(2, dims[0], dtype=torch.float32, device=dev) if want_frames else None
    ws = torch.empty(max(1, smooth_loss_workspace_bytes(*dims) // 4), dtype=torch.float32, device=dev)
    _launch(dev, "msda_smooth_loss_forward_f32", "smooth_loss_forward", _int_array(dims), float(fps), _ptr_array(floats),
            _ptr_array(longs), losses.data_ptr(), _vp(frames), ws.data_ptr(), ws.numel() * 4)
    return losses, frames, ws


def smooth_loss_backward(dims, fps, floats, longs, grad_losses, ws, acc_grad):
    """msda_smooth_loss_backward_f32.  Returns the gradients of the prediction's five tensors (the two joint tensors: None
    without acc_grad).  One launch, no atomics."""
    dev = floats[0].device
    _nn_check("smooth_loss_backward", dev, list(floats) + list(longs) + [grad_losses, ws])
    grads = [torch.empty_like(t) if (acc_grad or i not in (2, 3)) else None for i, t in enumerate(floats[:SMOOTH_LOSS_GRADS])]
    _launch(dev, "msda_smooth_loss_backward_f32", "smooth_loss_backward", _int_array(dims), float(fps), _ptr_array(floats),
            _ptr_array(longs), grad_losses.data_ptr(), 1 if acc_grad else 0, _opt_ptr_array(grads), ws.data_ptr(), ws.numel() * 4)
    return grads


# ---- ARCTIC target preparation (msda_pre_process.hip) ---------------------------------------------------------------------------
PRE_FIT_OUTPUTS = ("R0", "T0", "transl", "j3d_cam_r", "j3d_cam_l", "cam_t_r", "cam_t_l", "cam_t_wp_r", "cam_t_wp_l", "cam_t_wp_o",
                   "off_r", "off_l")


def pre_fit_supported(B, NK, J):
    return bool((_lib or load()).msda_pre_fit_supported(int(B), int(NK), int(J)))


def dist_fields_supported(B, NV, L):
    return bool((_lib or load()).msda_dist_fields_supported(int(B), int(NV), int(L)))


def pre_fit(kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l, img_res):
    """msda_pre_fit_f32.  Returns ({name: tensor} in PRE_FIT_OUTPUTS' order, status [B] int32).  One launch, no host sync."""
    ins = [kp_full, kp_cano, kp2d_norm, K, j_full_r, j_full_l, j_cano_r, j_cano_l]
    dev = kp_full.device
    _nn_check("pre_fit", dev, ins)
    if any(t.dtype != torch.float32 for t in ins):
        raise RuntimeError("pre_fit: expected contiguous fp32 CUDA tensors on one device")
    B, NK, _ = kp_full.shape
    J = j_full_r.shape[1]
    want = [(B, NK, 3), (B, NK, 3), (B, NK, 2), (B, 3, 3)] + [(B, J, 3)] * 4
    if any(tuple(t.shape) != s for t, s in zip(ins, want)):
        raise RuntimeError("pre_fit: expected kp [B, NK, 3], kp2d [B, NK, 2], K [B, 3, 3] and joints [B, J, 3]")
    shapes = [(B, 3, 3), (B, 3), (B, 3), (B, J, 3), (B, J, 3)] + [(B, 3)] * 7
    outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _launch(dev, "msda_pre_fit_f32", "pre_fit", B, NK, J, float(img_res), _ptr_array(ins), _ptr_array(outs), status.data_ptr())
    return dict(zip(PRE_FIT_OUTPUTS, outs)), status


def dist_fields(hand_r, hand_l, obj, v_len, dist_min, dist_max):
    """msda_dist_fields_f32.  Returns (dists, idx): four tensors each, in the order ro, lo [B, NV], or, ol [B, L].  One launch."""
    dev = hand_r.device
    _nn_check("dist_fields", dev, [hand_r, hand_l, obj, v_len])
    B, NV, _ = hand_r.shape
    L = obj.shape[1]
    if any(t.dtype != torch.float32 for t in (hand_r, hand_l, obj)) or v_len.dtype != torch.int64 \
            or tuple(hand_l.shape) != (B, NV, 3) or tuple(obj.shape) != (B, L, 3) or tuple(v_len.shape) != (B,):
        raise RuntimeError("dist_fields: expected fp32 hands [B, NV, 3], obj [B, L, 3] and int64 v_len [B]")
    dists = [torch.empty(B, n, dtype=torch.float32, device=dev) for n in (NV, NV, L, L)]
    idx = [torch.empty(B, n, dtype=torch.int64, device=dev) for n in (NV, NV, L, L)]
    _launch(dev, "msda_dist_fields_f32", "dist_fields", B, NV, L, hand_r.data_ptr(), hand_l.data_ptr(), obj.data_ptr(),
            v_len.data_ptr(), float(dist_min), float(dist_max), _ptr_array(dists), _ptr_array(idx))
    return dists, idx


# ---- the tail of the step: gradient norm, clip and AdamW as multi-tensor launches (csrc/msda_optim.hip) ----
OPTIM_MAX_GROUPS = 8


def optim_supported(n_tensors, n_groups):
    return bool((_lib or load()).msda_optim_supported(int(n_tensors), int(n_groups)))


def optim_chunk_elems():
    return int((_lib or load()).msda_optim_chunk_elems())


def optim_chunks(numels):
    """msda_optim_chunks: (chunk_start as a list of len(numels) + 1 ints, the chunk count).  Host logic, nothing is launched."""
    lib = _lib or load()
    n = len(numels)
    numel = (ctypes.c_longlong * max(1, n))(*numels)
    start = (ctypes.c_longlong * (n + 1))()
    total = int(lib.msda_optim_chunks(n, ctypes.cast(numel, _VP), ctypes.cast(start, _VP)))
    if total < 0:
        _raise(lib, 1, "optim_chunks")
    return list(start), total


def grad_sumsq(dev, n, n_chunks, g, numel, chunk_start, partials):
    """msda_grad_sumsq_f32 over device tables given as addresses; partials: fp32 [n_chunks].  One launch."""
    _launch(dev, "msda_grad_sumsq_f32", "grad_sumsq", n, n_chunks, g, numel, chunk_start, partials.data_ptr())


def grad_norm_finish(dev, n_chunks, partials, max_norm, out):
    """msda_grad_norm_finish_f32: out (fp32 [2]) = total norm, clip coefficient.  One launch."""
    _launch(dev, "msda_grad_norm_finish_f32", "grad_norm_finish", n_chunks, partials.data_ptr(), float(max_norm), out.data_ptr())


def grad_scale(dev, n, n_chunks, g, numel, chunk_start, coef):
    """msda_grad_scale_f32: every gradient of the table *= the device scalar at address `coef`.  One launch."""
    _launch(dev, "msda_grad_scale_f32", "grad_scale", n, n_chunks, g, numel, chunk_start, coef)


def adamw_step(dev, n, n_chunks, p, g, exp_avg, exp_avg_sq, numel, chunk_start, group, step_offset, hyper, global_step, coef):
    """msda_adamw_step_f32.  Tables as device addresses; hyper: per group (lr, weight_decay, beta1, beta2, eps); coef: the
    address of the device clip coefficient or None.  One launch."""
    ng = len(hyper)
    cols = [(ctypes.c_double * ng)(*[float(h[k]) for h in hyper]) for k in range(5)]
    _launch(dev, "msda_adamw_step_f32", "adamw_step", n, n_chunks, p, g, exp_avg, exp_avg_sq, numel, chunk_start, group,
            step_offset, ng, *[ctypes.cast(c, _VP) for c in cols], int(global_step), coef)


def optim_advance(dev, n, step):
    """msda_optim_advance_f32: every 0-d fp32 device step of the pointer table at address `step` += 1.  One launch."""
    _launch(dev, "msda_optim_advance_f32", "optim_advance", n, step)


def grad_norm_finish_dev(dev, n_chunks, partials, max_norm, out, n, step, skip_nonfinite, status):
    """msda_grad_norm_finish_dev_f32: grad_norm_finish, then status (address of int32 [2] or None) = (skipped, += skipped) and,
    unless skipped, every step of the table += 1.  One launch."""
    _launch(dev, "msda_grad_norm_finish_dev_f32", "grad_norm_finish_dev", n_chunks, partials.data_ptr(), float(max_norm),
            out.data_ptr(), n, step, int(bool(skip_nonfinite)), status)


def adamw_step_dev(dev, n, n_chunks, p, g, exp_avg, exp_avg_sq, numel, chunk_start, group, step, n_groups, hyper, coef, skip):
    """msda_adamw_step_dev_f32.  Every table a device address; hyper: fp64 [n_groups][5] on the device; coef, skip: the addresses
    of the device clip coefficient and skip flag, or None.  One launch."""
    _launch(dev, "msda_adamw_step_dev_f32", "adamw_step_dev", n, n_chunks, p, g, exp_avg, exp_avg_sq, numel, chunk_start, group,
            step, n_groups, hyper, coef, skip)
