"""Drop-in DeformableDETR models: ``ArcticDeformableDETR`` (models/actic_detr.py:38-363) and ``AssemblyDeformableDETR``
(models/assembly_detr.py:34-247).

Constructor, submodule names and creation order, parameter init, the heads attached to ``transformer.decoder`` and the
output dict are the reference's, so a reference checkpoint loads with ``strict=True`` and one seed builds a bit-identical
``state_dict``.  The per-level heads after the transformer run as one autograd node (``functions.heads_func.detr_heads``):
on CUDA fp32, three forward and five backward HIP launches instead of the reference's per-level Linears and stacks.

One deliberate change: ARCTIC's ``local_fm`` path builds its all-false masks on the device (``torch.zeros(..., device=)``)
instead of ``torch.zeros(...).to(device)``, which costs a host-to-device copy per level; the values are identical.

The backbone path's ``input_proj`` loop (Conv2d, GroupNorm, ARCTIC's training feature mask) runs through
``functions.neck_func.input_proj_levels``: the convolutions stay torch's, everything after them is one HIP launch for all
levels (``csrc/msda_neck.hip``)."""
import copy
import math

import torch
import torch.nn.functional as F
from torch import nn

from ..functions.heads_func import ARCTIC, ASSEMBLY, detr_heads, inverse_sigmoid
from ..functions.neck_func import input_proj_levels, output_shapes

__all__ = ["ArcticDeformableDETR", "AssemblyDeformableDETR", "MLP", "NestedTensor", "inverse_sigmoid"]


def _get_clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for i in range(N)])


class MLP(nn.Module):
    """Very simple multi-layer perceptron (models/actic_detr.py:572-583)."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


class NestedTensor:
    """util/misc.py NestedTensor: a batch of images and its padding mask."""

    def __init__(self, tensors, mask):
        self.tensors = tensors
        self.mask = mask

    def decompose(self):
        return self.tensors, self.mask


def nested_tensor_from_tensor_list(tensor_list):
    """util/misc.py nested_tensor_from_tensor_list for [C, H, W] images: zero-padded batch, True on padded pixels."""
    max_size = [max(s) for s in zip(*[img.shape for img in tensor_list])]
    b, (c, h, w) = len(tensor_list), max_size
    tensor = torch.zeros((b, c, h, w), dtype=tensor_list[0].dtype, device=tensor_list[0].device)
    mask = torch.ones((b, h, w), dtype=torch.bool, device=tensor_list[0].device)
    for img, pad_img, m in zip(tensor_list, tensor, mask):
        pad_img[:img.shape[0], :img.shape[1], :img.shape[2]].copy_(img)
        m[:img.shape[1], :img.shape[2]] = False
    return NestedTensor(tensor, mask)


def _is_nested(samples):
    return hasattr(samples, "decompose") and hasattr(samples, "mask")


def _input_proj(backbone, hidden_dim, num_feature_levels):
    if num_feature_levels > 1:
        num_backbone_outs = len(backbone.strides)
        input_proj_list = []
        for _ in range(num_backbone_outs):
            in_channels = backbone.num_channels[_]
            input_proj_list.append(nn.Sequential(
                nn.Conv2d(in_channels, hidden_dim, kernel_size=1),
                nn.GroupNorm(32, hidden_dim),
            ))
        for _ in range(num_feature_levels - num_backbone_outs):
            input_proj_list.append(nn.Sequential(
                nn.Conv2d(in_channels, hidden_dim, kernel_size=3, stride=2, padding=1),
                nn.GroupNorm(32, hidden_dim),
            ))
            in_channels = hidden_dim
        return nn.ModuleList(input_proj_list)
    return nn.ModuleList([
        nn.Sequential(
            nn.Conv2d(backbone.num_channels[0], hidden_dim, kernel_size=1),
            nn.GroupNorm(32, hidden_dim),
        )])


def _backbone_inputs(model, samples, random_mask):
    """The multi-scale inputs of the backbone path (models/actic_detr.py:189-230, models/assembly_detr.py:145-171).

    The input_proj loop runs through ``functions.neck_func.input_proj_levels``: on CUDA fp32 the GroupNorm and the 30 %
    feature mask of all levels are one HIP launch (two backward); ``MSDA_NECK_FUSED=0`` or any other dtype / device is the
    reference's composition.  The masks are drawn from the same generator, in the same order and with the same shapes as the
    reference's, so one seed gives the same masks.  The extra levels' positional encoding is built from the masked
    projection where the reference passes the unmasked one: the encodings (sine, learned) read its shape, device and mask
    only."""
    if not _is_nested(samples):
        samples = nested_tensor_from_tensor_list(samples)
    features, pos = model.backbone(samples)
    masked = random_mask and model.training
    n_backbone = len(features)

    def project(first, xs):
        # levels first .. first + len(xs) - 1 in one call of the neck node; the uniforms are drawn per level in level order,
        # as the reference's torch.cuda.FloatTensor(shape).uniform_() after each projection draws them (the projections
        # themselves take nothing from the generator)
        convs = [model.input_proj[first + i][0] for i in range(len(xs))]
        norms = [model.input_proj[first + i][1] for i in range(len(xs))]
        uniforms = None
        if masked:
            uniforms = [torch.empty(shape, device=x.device).uniform_() for shape, x in zip(output_shapes(xs, convs), xs)]
        return input_proj_levels(xs, convs, norms, uniforms)

    # every level whose conv input is a backbone feature goes in one call: the backbone's own levels and the first extra
    # one, which reads features[-1].tensors; a later extra level reads the previous (masked) output, in a call of its own
    xs = [feat.tensors for feat in features]
    if model.num_feature_levels > n_backbone:
        xs.append(features[-1].tensors)
    srcs = project(0, xs)
    masks = []
    for feat in features:
        assert feat.mask is not None
        masks.append(feat.mask)
    for l in range(n_backbone, model.num_feature_levels):
        if l > n_backbone:
            srcs += project(l, [srcs[-1]])
        src = srcs[l]
        m = samples.mask
        mask = F.interpolate(m[None].float(), size=src.shape[-2:]).to(torch.bool)[0]
        pos_l = model.backbone[1](NestedTensor(src, mask)).to(src.dtype)
        masks.append(mask)
        pos.append(pos_l)
    return srcs, masks, pos


class ArcticDeformableDETR(nn.Module):
    """models/actic_detr.py DeformableDETR."""

    def __init__(self, backbone, transformer, num_classes, num_queries, num_feature_levels,
                 aux_loss=True, with_box_refine=False, two_stage=False, cfg=None,
                 method=None, window_size=None, feature_type='local_fm'):
        super().__init__()
        self.num_queries = num_queries
        self.transformer = transformer
        self.hidden_dim = transformer.d_model
        self.method = method
        self.window_size = window_size
        self.feature_type = feature_type

        self.cls_embed = nn.Linear(self.hidden_dim, num_classes)
        self.mano_pose_embed = nn.Linear(self.hidden_dim, 48)
        self.mano_beta_embed = nn.Linear(self.hidden_dim, 10)
        self.hand_cam = nn.Linear(self.hidden_dim, 3)
        self.obj_cam = nn.Linear(self.hidden_dim, 3)
        self.obj_rot = nn.Linear(self.hidden_dim, 3)
        self.obj_rad = nn.Linear(self.hidden_dim, 1)

        self.num_feature_levels = num_feature_levels
        self.cfg = cfg

        self.query_embed = nn.Embedding(num_queries, self.hidden_dim * 2)
        if self.feature_type == 'origin':
            self.input_proj = _input_proj(backbone, self.hidden_dim, num_feature_levels)
            for proj in self.input_proj:
                nn.init.xavier_uniform_(proj[0].weight, gain=1)
                nn.init.constant_(proj[0].bias, 0)
            self.backbone = backbone
        else:
            self.backbone = backbone[1]                 # only the positional encoding

        self.aux_loss = aux_loss
        self.with_box_refine = with_box_refine
        self.two_stage = two_stage

        prior_prob = 0.01
        bias_value = -math.log((1 - prior_prob) / prior_prob)
        self.cls_embed.bias.data = torch.ones(num_classes) * bias_value

        for lin in (self.mano_pose_embed, self.mano_beta_embed, self.hand_cam, self.obj_cam, self.obj_rot, self.obj_rad):
            nn.init.xavier_uniform_(lin.weight, gain=1)
            nn.init.constant_(lin.bias.data, 0)

        num_pred = (transformer.decoder.num_layers + 1) if two_stage else transformer.decoder.num_layers
        if with_box_refine:
            assert two_stage, "Not implemented! You should use 'with_box_refine' and 'two_stage' option simultaneously."
            self.cls_embed = _get_clones(self.cls_embed, num_pred)
            self.key_embed = MLP(self.hidden_dim, self.hidden_dim, 42, 3)
            self.obj_key_embed = MLP(self.hidden_dim, self.hidden_dim, 42, 3)
            nn.init.xavier_uniform_(self.key_embed.layers[-1].weight.data, gain=1)
            nn.init.constant_(self.key_embed.layers[-1].bias.data, 0)
            nn.init.xavier_uniform_(self.obj_key_embed.layers[-1].weight.data, gain=1)
            nn.init.constant_(self.obj_key_embed.layers[-1].bias.data, 0)
            self.key_embed = _get_clones(self.key_embed, num_pred)
            self.obj_key_embed = _get_clones(self.obj_key_embed, num_pred)
            self.transformer.decoder.cls_embed = self.cls_embed
            self.transformer.decoder.key_embed = self.key_embed
            self.transformer.decoder.obj_key_embed = self.obj_key_embed
        else:
            self.cls_embed = nn.ModuleList([self.cls_embed for _ in range(num_pred)])
        self.mano_pose_embed = nn.ModuleList([self.mano_pose_embed for _ in range(num_pred)])
        self.mano_beta_embed = nn.ModuleList([self.mano_beta_embed for _ in range(num_pred)])
        self.hand_cam = nn.ModuleList([self.hand_cam for _ in range(num_pred)])
        self.obj_cam = nn.ModuleList([self.obj_cam for _ in range(num_pred)])
        self.obj_rot = nn.ModuleList([self.obj_rot for _ in range(num_pred)])
        self.obj_rad = nn.ModuleList([self.obj_rad for _ in range(num_pred)])

    def forward(self, samples, is_extract=False):
        if self.feature_type == 'origin':
            if is_extract:
                if not _is_nested(samples):
                    samples = nested_tensor_from_tensor_list(samples)
                return self.backbone(samples)[0]
            srcs, masks, pos = _backbone_inputs(self, samples, random_mask=True)
        else:
            srcs, masks, pos = [], [], []
            for i in range(self.num_feature_levels):
                B, N, C, W, H = samples[i].shape
                device = samples[i].device
                src = samples[i].view(B * N, C, W, H)
                mask = torch.zeros(B * N, W, H, dtype=torch.bool, device=device)
                pos_l = self.backbone(NestedTensor(src, mask)).to(src.dtype)
                srcs.append(src)
                masks.append(mask)
                pos.append(pos_l)

        query_embeds = self.query_embed.weight
        hs, init_reference, inter_references, enc_outputs_class, enc_outputs_hand_coord_unact, \
            enc_outputs_obj_coord_unact = self.transformer(srcs, masks, pos, query_embeds)
        return self.heads(hs, init_reference, inter_references, enc_outputs_class, enc_outputs_hand_coord_unact,
                          enc_outputs_obj_coord_unact)

    def heads(self, hs, init_reference, inter_references, enc_outputs_class=None, enc_outputs_hand_coord_unact=None,
              enc_outputs_obj_coord_unact=None):
        """Everything the reference's forward does after the transformer (models/actic_detr.py:234-325)."""
        levels = hs.shape[0]
        shared = [self.mano_pose_embed[0], self.mano_beta_embed[0], self.hand_cam[0], self.obj_cam[0], self.obj_rot[0],
                  self.obj_rad[0]]
        mlps = [self.key_embed, self.obj_key_embed] if self.two_stage else []
        outputs_class, keys, (pose, beta, hand_cam, obj_cam, obj_rot, obj_rad) = detr_heads(
            ARCTIC, hs, init_reference, inter_references, self.cls_embed, mlps, shared)
        if self.two_stage:
            outputs_hand_coord, outputs_obj_coord = keys
        else:
            outputs_hand_coord = torch.zeros(levels)
            outputs_obj_coord = torch.zeros(levels)
        outputs_mano_params = [pose, beta]
        outputs_obj_params = [obj_rad, obj_rot]
        outputs_cams = [hand_cam, obj_cam]

        out = {
            'pred_logits': outputs_class[-1], 'pred_hand_key': outputs_hand_coord[-1], 'pred_obj_key': outputs_obj_coord[-1],
            'pred_mano_params': [outputs_mano_params[0][-1], outputs_mano_params[1][-1]],
            'pred_obj_params': [outputs_obj_params[0][-1], outputs_obj_params[1][-1]],
            'pred_cams': [outputs_cams[0][-1], outputs_cams[1][-1]]
        }
        if self.aux_loss:
            out['aux_outputs'] = self._set_aux_loss(outputs_class, outputs_hand_coord, outputs_obj_coord,
                                                    outputs_mano_params, outputs_obj_params, outputs_cams)
        if self.two_stage:
            enc_outputs_hand_coord = enc_outputs_hand_coord_unact.sigmoid() * 2 - 1
            enc_outputs_obj_coord = enc_outputs_obj_coord_unact.sigmoid() * 2 - 1
            out['interm_outputs'] = {
                'pred_logits': enc_outputs_class,
                'pred_hand_key': enc_outputs_hand_coord,
                'pred_obj_key': enc_outputs_obj_coord
            }
        return out

    @torch.jit.unused
    def _set_aux_loss(self, outputs_class, outputs_hand_coord, outputs_obj_coord,
                      outputs_mano_params, outputs_obj_params, outputs_cams):
        return [
            {
                'pred_logits': c, 'pred_hand_key': hk, 'pred_obj_key': ok,
                'pred_mano_params': [s, p], 'pred_obj_params': [ra, ro], 'pred_cams': [hc, oc]
            }
            for c, hk, ok, s, p, ra, ro, hc, oc in zip(
                outputs_class[:-1], outputs_hand_coord[:-1], outputs_obj_coord[:-1],
                outputs_mano_params[0][:-1], outputs_mano_params[1][:-1],
                outputs_obj_params[0][:-1], outputs_obj_params[1][:-1],
                outputs_cams[0][:-1], outputs_cams[1][:-1])
        ]


class AssemblyDeformableDETR(nn.Module):
    """models/assembly_detr.py DeformableDETR."""

    def __init__(self, backbone, transformer, num_classes, num_queries, num_feature_levels,
                 aux_loss=True, with_box_refine=False, two_stage=False, cfg=None):
        super().__init__()
        self.num_queries = num_queries
        self.transformer = transformer
        self.hidden_dim = transformer.d_model
        self.cls_embed = nn.Linear(self.hidden_dim, num_classes)
        self.keypoint_embed = MLP(self.hidden_dim, self.hidden_dim, 63, 3)
        self.obj_keypoint_embed = MLP(self.hidden_dim, self.hidden_dim, 63, 3)
        self.num_feature_levels = num_feature_levels
        self.cfg = cfg

        self.query_embed = nn.Embedding(num_queries, self.hidden_dim * 2)
        self.input_proj = _input_proj(backbone, self.hidden_dim, num_feature_levels)
        self.backbone = backbone
        self.aux_loss = aux_loss
        self.with_box_refine = with_box_refine
        self.two_stage = two_stage

        prior_prob = 0.01
        bias_value = -math.log((1 - prior_prob) / prior_prob)
        self.cls_embed.bias.data = torch.ones(num_classes) * bias_value
        nn.init.constant_(self.keypoint_embed.layers[-1].weight.data, 0)
        nn.init.constant_(self.keypoint_embed.layers[-1].bias.data, 0)
        nn.init.constant_(self.obj_keypoint_embed.layers[-1].weight.data, 0)
        nn.init.constant_(self.obj_keypoint_embed.layers[-1].bias.data, 0)
        for proj in self.input_proj:
            nn.init.xavier_uniform_(proj[0].weight, gain=1)
            nn.init.constant_(proj[0].bias, 0)

        num_pred = (transformer.decoder.num_layers + 1) if two_stage else transformer.decoder.num_layers
        if with_box_refine:
            self.cls_embed = _get_clones(self.cls_embed, num_pred)
            self.keypoint_embed = _get_clones(self.keypoint_embed, num_pred)
            self.obj_keypoint_embed = _get_clones(self.obj_keypoint_embed, num_pred)
            self.transformer.decoder.cls_embed = self.cls_embed
            self.transformer.decoder.keypoint_embed = self.keypoint_embed
            self.transformer.decoder.obj_keypoint_embed = self.obj_keypoint_embed
        else:
            self.cls_embed = nn.ModuleList([self.cls_embed for _ in range(num_pred)])
            self.keypoint_embed = nn.ModuleList([self.keypoint_embed for _ in range(num_pred)])
            self.obj_keypoint_embed = nn.ModuleList([self.obj_keypoint_embed for _ in range(num_pred)])
            self.transformer.decoder.keypoint_embed = None
            self.transformer.decoder.obj_keypoint_embed = None
        if two_stage:
            self.transformer.decoder.cls_embed = self.cls_embed

    def forward(self, samples):
        srcs, masks, pos = _backbone_inputs(self, samples, random_mask=False)
        query_embeds = self.query_embed.weight
        hs, init_reference, inter_references, enc_outputs_class, enc_outputs_hand_coord_unact, \
            enc_outputs_obj_coord_unact = self.transformer(srcs, masks, pos, query_embeds)
        return self.heads(hs, init_reference, inter_references, enc_outputs_class, enc_outputs_hand_coord_unact,
                          enc_outputs_obj_coord_unact)

    def heads(self, hs, init_reference, inter_references, enc_outputs_class=None, enc_outputs_hand_coord_unact=None,
              enc_outputs_obj_coord_unact=None):
        """Everything the reference's forward does after the transformer (models/assembly_detr.py:169-222)."""
        outputs_class, (outputs_keypoints,), _ = detr_heads(ASSEMBLY, hs, init_reference, inter_references,
                                                             self.cls_embed, [self.keypoint_embed])
        out = {'pred_logits': outputs_class[-1], 'pred_keypoints': outputs_keypoints[-1]}
        if self.aux_loss:
            out['aux_outputs'] = self._set_aux_loss(outputs_class, outputs_keypoints)
        if self.two_stage:
            enc_outputs_hand_coord = enc_outputs_hand_coord_unact.sigmoid()
            out['enc_outputs'] = {'pred_logits': enc_outputs_class, 'pred_keypoints': enc_outputs_hand_coord}
        return out

    @torch.jit.unused
    def _set_aux_loss(self, outputs_class, outputs_keypoints):
        return [{'pred_logits': a, 'pred_keypoints': b}
                for a, b in zip(outputs_class[:-1], outputs_keypoints[:-1])]
